"""What a residual-fused decoder layer is made of, whatever its family: the hand-over of a quantised input from one layer to the next (``_HandOver``), the probe of a
layer class's forward against a closed formula (``probe_named_flow``), the run-time class that derives from a fused kind AND from the layer's original class
(``fused_class``) with its copy protocol, the argument handling of the two groups of kinds — children found by name (``NamedFusedLayer``) and children found by a
recorded plan (``FlowPlan``) — and the walk over the ``ModuleList`` stacks of a model that converts and links the layers (``fuse_stacks``).  ``llama``, ``gemma``,
``olmo`` and ``gptlike`` hold what is specific to a family: its norm modules, its eligibility rules and the kernel sequence of its forward."""
from __future__ import annotations

import inspect

import torch
from torch import nn


# ---------------------------------------------------------------- the hand-over between two layers of a chain
class _HandOver:
    """The quantised input one layer computed for the next (K1a's second use per layer), keyed by the identity of the tensor it belongs to and that tensor's version
    counter.  take() empties it whatever the outcome; a copy — deep or pickled — starts empty."""
    __slots__ = ("_key", "_version", "_q")

    def __init__(self):
        self.clear()

    @staticmethod
    def _version_of(t):
        try:
            return t._version
        except Exception:          # noqa: BLE001  (inference tensors track no version counter)
            return None

    def put(self, key: torch.Tensor, q):
        self._key, self._version, self._q = key, self._version_of(key), q

    def take(self, x):
        key, version, q = self._key, self._version, self._q
        self.clear()
        return q if key is not None and key is x and version == self._version_of(x) else None

    def clear(self):
        self._key, self._version, self._q = None, None, None

    @property
    def pending(self) -> bool:
        return self._key is not None

    def __deepcopy__(self, memo):
        return _HandOver()

    def __reduce__(self):
        return (_HandOver, ())


def _rf_clear_hook(mod, args, output):
    for layer in mod._rf_layers:          # (looked up on the module, not captured: a deep copy of the model clears its own layers)
        layer._rf_inbox.clear()


def _link_chain(owner: nn.Module, stack: nn.ModuleList, fresh: list, kind: type) -> None:
    """After `fresh` layers of `stack` became `kind` (a fused kind: llama.ResidualFusedLayer, gptlike.ParallelFusedBlock, ...): (re)link the chain — a layer hands over
    to its successor in the stack when that one is of the same kind; anything else ends the chain — and give the owner of the stack its clearing hook, once."""
    for i, layer in enumerate(stack):
        if isinstance(layer, kind):
            nxt = stack[i + 1] if i + 1 < len(stack) else None
            layer._rf_next = [nxt if isinstance(nxt, kind) else None]          # (a list: the next layer is registered once, in the stack)
    if fresh:
        if not hasattr(owner, "_rf_layers"):
            owner._rf_layers = []
            owner.register_forward_hook(_rf_clear_hook, always_call=True)          # the owner's forward ended (exceptions included): nothing stays pending
        owner._rf_layers.extend(fresh)


def _hooked(m: nn.Module) -> bool:
    return bool(m._forward_hooks) or bool(m._forward_pre_hooks)


# ---------------------------------------------------------------- is it this data flow?  (children found by name)
class _ProbeRefused(Exception):
    pass


class _ProbeLayer:
    """Stand-in for `self` in a decoder layer class's own forward: the children of the probed flow are recording functions, every other attribute is read from the real
    layer — except another module (a dropout, a third norm): a forward that touches one is not the probed data flow."""

    def __init__(self, layer: nn.Module, children: dict):
        self.__dict__["_layer"] = layer
        self.__dict__.update(children)

    def __getattr__(self, name):
        v = getattr(self.__dict__["_layer"], name)
        if isinstance(v, nn.Module):
            raise _ProbeRefused(f"forward reads the submodule {name!r}")
        return v


def _forward_extra_params(cls) -> tuple:
    """(names of the positional parameters of cls.forward after hidden_states, whether it takes **kwargs)"""
    ps = list(inspect.signature(cls.forward).parameters.values())[2:]          # (self, hidden_states, ...)
    names = tuple(p.name for p in ps if p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD))
    return names, any(p.kind == p.VAR_KEYWORD for p in ps)


class attention:
    """Marks the entry of a probe_named_flow table that stands in for the attention: called with the hidden state and the layer's keyword arguments, returns (f(h), None)."""

    def __init__(self, f):
        self.f = f


def probe_named_flow(layer: nn.Module, cls, children: dict, want, attn_positional: bool = False) -> bool:
    """True iff `cls.forward`, run on a stand-in of `layer`, computes want(x) on x = arange(-6, 6).reshape(1, 3, 4).  `children` maps, in order, the name of every
    child of the flow to an exact function on small integers, the attention's wrapped in attention(); each must be called once, every keyword argument of the layer
    (a sentinel per extra parameter of the forward, one more under `pq_probe_extra` when it takes **kwargs) must reach the attention unchanged and by identity, no
    other submodule may be touched and a tensor of want(x)'s shape, dtype and values returned.  The attention must be given its input as `hidden_states=`;
    attn_positional also accepts it as the first and only positional argument.  Whatever the forward raises on the stand-in is a refusal."""
    try:
        names, var_kw = _forward_extra_params(cls)
    except (TypeError, ValueError, AttributeError):
        return False
    given = {n: object() for n in names}
    if var_kw:
        given["pq_probe_extra"] = object()
    calls = dict.fromkeys(children, 0)
    seen = {}

    def standin(name, f):
        if isinstance(f, attention):
            def attn(*a, **kw):
                calls[name] += 1
                by_name = "hidden_states" in kw or not attn_positional
                h = kw.pop("hidden_states") if by_name else a[0]
                seen["positional"], seen["kwargs"] = len(a) - (0 if by_name else 1), kw
                return f.f(h), None
            return attn

        def run(t):
            calls[name] += 1
            return f(t)
        return run

    x = torch.arange(-6, 6, dtype=torch.float32).reshape(1, 3, 4)            # small integers: every operation below is exact
    probe = _ProbeLayer(layer, {name: standin(name, f) for name, f in children.items()})
    try:
        with torch.no_grad():
            out = cls.forward(probe, x.clone(), **given)
    except Exception:          # noqa: BLE001  (whatever the forward raises on the stand-in: refused)
        return False
    if not isinstance(out, torch.Tensor) or any(n != 1 for n in calls.values()):
        return False
    kw = seen["kwargs"]
    if seen["positional"] != 0 or set(kw) != set(given) or any(kw[k] is not given[k] for k in given):
        return False
    expected = want(x)
    return out.shape == expected.shape and out.dtype == expected.dtype and torch.equal(out, expected)


# ---------------------------------------------------------------- the class of a fused layer and its copies
class FusedLayer(nn.Module):
    """Base of every fused kind.  A layer becomes one by getting the class fused_class(kind, its original class): the object, its children under their names
    (state_dict keys), its other attributes, its hooks and every isinstance check on it stay as they were.  `_pq_prefix` names that class."""
    _pq_prefix = "Fused"

    def __reduce_ex__(self, protocol):          # (the class is made at run time: a copy — deep or pickled — makes it again from the original class)
        return _rebuild_fused, type(self).__bases__, self.__dict__


_FUSED_CLASSES: dict = {}


def fused_class(kind, cls):
    """the class named kind._pq_prefix + cls.__name__ that derives from `kind` and from `cls`, made once"""
    if (kind, cls) not in _FUSED_CLASSES:
        _FUSED_CLASSES[kind, cls] = type(kind._pq_prefix + cls.__name__, (kind, cls), {"__doc__": kind.__doc__})
    return _FUSED_CLASSES[kind, cls]


def _rebuild_fused(kind, cls):
    fused = fused_class(kind, cls)
    return fused.__new__(fused)


class NamedFusedLayer(FusedLayer):
    """A fused kind whose forward finds the children by their names and hands every argument but the hidden state to the attention by keyword."""

    def _fold_positional(self, args, kwargs) -> None:
        """the positional arguments of the original forward into `kwargs`, by its own parameter names (_rf_argnames)"""
        if len(args) > len(self._rf_argnames):
            raise TypeError(f"{type(self).__name__}.forward takes at most {len(self._rf_argnames) + 1} positional arguments")
        kwargs.update(zip(self._rf_argnames, args))


_H = "pq:norm-output"          # the place of the norm's output in the recorded attention call


class FlowPlan:
    """What the probe of a block class's forward recorded, whatever the flow: the attention call to replay — for every positional and keyword argument either _H,
    ("param", name of the block's own parameter handed on) or ("const", value) — whether the block's **kwargs go to the attention, the block parameters the attention
    never saw (`withheld`: a call that sets one of them runs the original forward) and the stateless children (dropouts) that the eval-mode probe found to be no-ops on
    the stream (a call in training mode runs the original forward).  A subclass adds the names of the roles; `attn` is the attention's."""

    def __init__(self, cls, args, kwargs, var_kw, withheld, defaults, stateless):
        self.cls, self.args, self.kwargs, self.var_kw = cls, tuple(args), dict(kwargs), var_kw
        self.withheld, self.defaults, self.stateless = tuple(withheld), dict(defaults), tuple(stateless)
        self.signature = inspect.signature(cls.forward)
        ps = list(self.signature.parameters.values())
        self.first = ps[1].name
        self.var_kw_name = next((p.name for p in ps if p.kind == p.VAR_KEYWORD), None)

    def bind(self, block, args, kwargs):
        """The arguments of one call of the fused block: (given — every parameter of the original forward by name, defaults applied —, the extra keyword arguments,
        None).  A call the probe did not cover — training mode with a stateless child on the stream, a hidden state that is no tensor, extras the attention would not
        get, a withheld parameter off its default — drops the pending hand-over and runs the original forward: (None, None, its result)."""
        bound = self.signature.bind(block, *args, **kwargs)          # (a TypeError here is the one the original forward would raise)
        bound.apply_defaults()
        given = bound.arguments
        extras = given.get(self.var_kw_name, {}) if self.var_kw_name else {}
        if ((block.training and self.stateless) or not isinstance(given[self.first], torch.Tensor) or (extras and not self.var_kw)
                or any(given[n] is not self.defaults[n] for n in self.withheld)):
            block._rf_inbox.clear()
            return None, None, self.cls.forward(block, *args, **kwargs)
        return given, extras, None

    def replay(self, block, h, given, extras):
        """the attention called the way the block's own forward calls it, with `h` in the norm output's place"""
        value = lambda e: h if e == _H else given[e[1]] if e[0] == "param" else e[1]          # noqa: E731
        return getattr(block, self.attn)(*(value(e) for e in self.args), **{k: value(e) for k, e in self.kwargs.items()}, **extras)


# ---------------------------------------------------------------- every stack of a model
def fuse_stacks(model: nn.Module, kind: type, convert) -> int:
    """For every member of every ModuleList child of every module of `model`: convert(layer) returns None, or prepares what the kind's forward reads from the layer
    and returns the layer's class — the layer then gets its inbox and the class fused_class(kind, that class).  Every stack is (re)linked (_link_chain).  Returns the
    number of layers converted."""
    n = 0
    for owner in list(model.modules()):
        for _, stack in list(owner.named_children()):
            if not isinstance(stack, nn.ModuleList):
                continue
            fresh = []
            for layer in stack:
                cls = convert(layer)
                if cls is None:
                    continue
                layer._rf_inbox, layer._rf_next = _HandOver(), [None]
                layer.__class__ = fused_class(kind, cls)
                fresh.append(layer)
            _link_chain(owner, stack, fresh, kind)          # (a chain that ends, ends with the kind's own closing step)
            n += len(fresh)
    return n
