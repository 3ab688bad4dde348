"""Call-site integration for decoders built from LayerNorm (with bias) and a plain two-linear MLP with a unary activation — GPT-2, StarCoder2, GPT-NeoX /
Pythia, and whatever else passes the same probes:

* a LayerNorm whose output only feeds int8 projections becomes ``LayerNormQuant`` (``layernorm_quantize``, kernel K1l: the normalised activation never
  reaches HBM; one quantisation serves every projection that reads it);
* the activation between the two projections of the MLP becomes ``ActQuant`` (``act_quantize``, kernel K1u), installed IN PLACE of the MLP's activation
  attribute: the model's own MLP forward, ``c_proj(act(c_fc(x)))``, keeps running — ``qlinear.forward`` accepts the per-token ``QTensor`` — and every
  state-dict key survives.

``swap_linears(model)`` must have run first.  Nothing is recognised by class name or by import: a block's own forward is run on the CPU against stand-ins
(``_Standin``) whose projections are recorders, and a replacement happens only where that run shows the data flow the fused form needs.  A refusal leaves
the module objects untouched.  Composes with ``fuse_llama_layers`` (StarCoder2's q / k / v) in either call order.

``fuse_layernorm_residual(model)`` (opt-in, run after ``fuse_layernorm_layers``) also takes the two residual adds of a sequential pre-norm block into the LayerNorm that follows
them (``add_layernorm_quantize``, kernel K1al: the residual stream is stored once and normalised from registers): see ``ResidualFusedBlock``.

``fuse_parallel_residual(model)`` (opt-in, an entry of its own, run after ``fuse_layernorm_layers``) does the same for the PARALLEL residual of GPT-NeoX / Pythia
(``use_parallel_residual=True``) and Phi, which the entry above refuses by design: the three-way sum ``x + attn + mlp`` and the norm(s) of the next block run in one
kernel (``add2_layernorm_quantize``, K1pl; the first block of a two-norm stack reads its input once, ``layernorm_quantize2``, K1l2): see ``ParallelFusedBlock``."""
from __future__ import annotations

import copy
import inspect
import types

import torch
from torch import nn

from . import _lib as L
from .llama import _FusedSlice
from .qlinear import FusedQLinear, qlinear
from .qtensor import act_quantize, add2_layernorm_quantize, add_layernorm_quantize, layernorm_quantize, layernorm_quantize2
from .residual_flow import _H, FlowPlan, FusedLayer, _hooked, _ProbeRefused, fuse_stacks


class LayerNormQuant(nn.Module):
    """LayerNorm whose output is the per-token int8 quantisation of the normalised activation (QSPEC L1-L6 then Q1-Q6)."""

    def __init__(self, weight: torch.Tensor, bias: torch.Tensor | None, eps: float):
        super().__init__()
        if weight is None:
            raise ValueError("LayerNormQuant: a LayerNorm without affine parameters (elementwise_affine=False) is not supported")
        self.weight = nn.Parameter(weight.detach().clone(), requires_grad=False)
        if bias is not None:
            self.bias = nn.Parameter(bias.detach().clone(), requires_grad=False)
        else:
            self.register_parameter("bias", None)
        self.eps = float(eps)

    def forward(self, x: torch.Tensor, residual: torch.Tensor | None = None):
        """Without `residual`: the QTensor of LayerNorm(x).  With it: (QTensor of LayerNorm(residual + x), residual + x) from one kernel (K1al) — the bits of the
        torch add followed by the call without `residual`."""
        if residual is None:
            return layernorm_quantize(x, self.weight, self.bias, self.eps)
        return add_layernorm_quantize(x, residual, self.weight, self.bias, self.eps)

    def extra_repr(self):
        return f"{tuple(self.weight.shape)}, eps={self.eps}, bias={self.bias is not None} -> int8 per-token QTensor"


class ActQuant(nn.Module):
    """A unary activation whose output is the per-token int8 quantisation of act(x) (QSPEC U1-U4 then Q1-Q6); kind: "relu", "gelu_tanh" or "gelu_erf"."""

    def __init__(self, kind: str):
        super().__init__()
        if kind not in L.ACT_KINDS:
            raise ValueError(f"ActQuant: unknown kind {kind!r}, expected one of {sorted(L.ACT_KINDS)}")
        self.kind = kind

    def forward(self, x: torch.Tensor):
        return act_quantize(x, self.kind)

    def extra_repr(self):
        return f"{self.kind} -> int8 per-token QTensor"


# ---------------------------------------------------------------- which activation is it?  (by behaviour)
def _act_f64(x: torch.Tensor, kind: str) -> torch.Tensor:
    if kind == "relu":
        return torch.relu(x)
    if kind == "gelu_tanh":
        return 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))
    return 0.5 * x * torch.erfc(-x * 0.7071067811865476)


def activation_kind(act) -> str | None:
    """"relu" / "gelu_tanh" / "gelu_erf" when `act` — a module without parameters or buffers, or a plain function — computes that function: it is evaluated in
    float64 on a fixed CPU grid and must agree to 1e-9 (the tanh and the erf GELU differ by 5e-4, quick_gelu by 2e-2, so nothing is confused).  None for
    everything else (quick_gelu, gelu_10, relu^2, silu, anything that raises, anything with state)."""
    if isinstance(act, nn.Module) and (any(True for _ in act.parameters()) or any(True for _ in act.buffers())):
        return None
    if not callable(act):
        return None
    x = torch.cat([torch.linspace(-12.0, 12.0, 481, dtype=torch.float64), torch.tensor([-30.0, -0.0, 0.0, 1e-8, -1e-8, 30.0], dtype=torch.float64)])
    try:
        with torch.no_grad():
            y = act(x.clone())
    except Exception:          # noqa: BLE001
        return None
    if not isinstance(y, torch.Tensor) or y.shape != x.shape or y.dtype != torch.float64:
        return None
    for kind in ("relu", "gelu_tanh", "gelu_erf"):
        if torch.allclose(y, _act_f64(x, kind), rtol=0.0, atol=1e-9):
            return kind
    return None


# ---------------------------------------------------------------- the probe
class _Probed:
    """What a fused norm or activation returns under the probe: the metadata surface of a per-token QTensor (shape, device) and nothing else.  Any other attribute
    is a refusal; arithmetic and torch functions fail on it by themselves."""
    __slots__ = ("shape", "device", "tag", "uses")

    def __init__(self, shape, tag):
        self.shape, self.device, self.tag, self.uses = torch.Size(shape), torch.device("cpu"), tag, 0

    def __getattr__(self, name):
        raise _ProbeRefused(f"the output of {self.tag!r} is read for .{name}")


def _is_eligible_layernorm(m) -> bool:
    return (isinstance(m, nn.LayerNorm) and type(m).forward is nn.LayerNorm.forward and len(m.normalized_shape) == 1 and m.elementwise_affine
            and isinstance(m.weight, torch.Tensor) and m.weight.dim() == 1)


def _is_int8_proj(m) -> bool:
    return isinstance(m, (qlinear, FusedQLinear, _FusedSlice))


def _stateless(m: nn.Module) -> bool:
    return not any(True for _ in m.parameters()) and not any(True for _ in m.buffers())


class _Record:
    def __init__(self):
        self.norm_calls: dict = {}          # name -> [tokens]
        self.act_calls: list = []           # (input, token)
        self.proj_outputs: list = []        # tensors a projection recorder returned


class _Standin:
    """Stand-in for `self` in a module class's own forward.  Children: an int8 projection is a recorder (takes a tensor or a _Probed, returns zeros of the output
    shape on the CPU — no weight is touched); the candidates named in `norms` / `acts` return a _Probed; a module without parameters or buffers (dropout, an
    activation) is the real one; any other module is a nested stand-in running ITS class's forward.  Every other attribute is the real module's, methods re-bound
    to the stand-in."""

    def __init__(self, mod: nn.Module, rec: _Record, norms=(), acts=(), cpu_state: bool = False):
        d = self.__dict__
        d["_mod"], d["_rec"], d["_norms"], d["_acts"], d["_kids"], d["_cpu_state"] = mod, rec, dict(norms), dict(acts), {}, cpu_state

    def __getattr__(self, name):
        v = getattr(self.__dict__["_mod"], name)
        if self.__dict__["_cpu_state"] and isinstance(v, torch.Tensor) and v.device.type != "cpu":
            return v.detach().cpu()          # (cpu_state: a parameter the forward reads itself — Gemma-3's q_norm weight — meets the probe's CPU tensors as a CPU copy)
        if isinstance(v, nn.Module):
            kids = self.__dict__["_kids"]
            if name not in kids:
                kids[name] = self._child(name, v)
            return kids[name]
        if isinstance(v, types.MethodType) and v.__self__ is self.__dict__["_mod"]:
            return types.MethodType(v.__func__, self)
        return v

    def __call__(self, *a, **kw):
        return type(self.__dict__["_mod"]).forward(self, *a, **kw)

    def _child(self, name, v):
        rec = self.__dict__["_rec"]
        if self.__dict__["_norms"].get(name) == "plain":          # a norm that is not under test in this run: a tensor of its input's shape
            return lambda x: torch.zeros(x.shape)
        if name in self.__dict__["_norms"] or isinstance(v, LayerNormQuant):
            def norm(x, _name=name):
                if not isinstance(x, torch.Tensor):
                    raise _ProbeRefused(f"{_name} is called with {type(x).__name__}")
                tok = _Probed(x.shape, _name)
                rec.norm_calls.setdefault(_name, []).append(tok)
                return tok
            return norm
        if name in self.__dict__["_acts"] or isinstance(v, ActQuant):
            def act(x, _name=name):
                if not isinstance(x, torch.Tensor):
                    raise _ProbeRefused(f"{_name} is called with {type(x).__name__}")
                tok = _Probed(x.shape, _name)
                rec.act_calls.append((x, tok))
                return tok
            return act
        if _is_int8_proj(v):
            def proj(x, _v=v):
                if isinstance(x, _Probed):
                    x.uses += 1
                elif not isinstance(x, torch.Tensor):
                    raise _ProbeRefused(f"a projection is called with {type(x).__name__}")
                lead = tuple(x.shape[:-1])
                if isinstance(_v, FusedQLinear):
                    out = tuple(torch.zeros(lead + (n,)) for n in _v.splits)
                    rec.proj_outputs.extend(out)
                    return out
                n = _v._shared[0].fused.splits[_v.index] if isinstance(_v, _FusedSlice) else _v.out_features
                out = torch.zeros(lead + (n,))
                rec.proj_outputs.append(out)
                return out
            return proj
        if isinstance(v, (nn.ModuleList, nn.ModuleDict, nn.Sequential)):
            raise _ProbeRefused(f"forward reads the container {name!r}")
        if _stateless(v):
            return v
        return _Standin(v, rec, cpu_state=self.__dict__["_cpu_state"])


def _leaks(out) -> bool:
    if isinstance(out, _Probed):
        return True
    if isinstance(out, dict):
        return any(_leaks(v) for v in out.values())
    if isinstance(out, (tuple, list)):
        return any(_leaks(v) for v in out)
    return False


def _run_probe(mod: nn.Module, rec: _Record, norms=(), acts=(), width: int | None = None, cpu_state: bool = False):
    """type(mod).forward on a stand-in of `mod` with a [1, 3, width] CPU tensor of zeros; parameters of the forward that have no default get None, one named
    position_embeddings gets a (cos, sin) pair that broadcasts against any head size.  Raises whatever the forward raises.  cpu_state: tensors that the stand-ins
    hand out as attributes of a module on another device are CPU copies (the default hands out the module's own: such a forward raises and is refused)."""
    ps = list(inspect.signature(type(mod).forward).parameters.values())[1:]
    if not ps:
        raise _ProbeRefused("forward takes no input")
    x = torch.zeros(1, 3, width)
    kw = {}
    for p in ps[1:]:
        if p.name == "position_embeddings":
            kw[p.name] = (torch.ones(1, 3, 1), torch.zeros(1, 3, 1))
        elif p.default is p.empty and p.kind in (p.POSITIONAL_OR_KEYWORD, p.KEYWORD_ONLY):
            kw[p.name] = None
    with torch.no_grad(), torch.random.fork_rng(devices=[]):
        return _Standin(mod, rec, norms, acts, cpu_state)(x, **kw)


def fusable_norms(block: nn.Module, candidate=None) -> list:
    """Names of the LayerNorm children of `block` that may become LayerNormQuant: each is an nn.LayerNorm with nn.LayerNorm's own forward, a 1-D
    normalized_shape and affine parameters, AND the block's own forward, run on the CPU against stand-ins, calls it exactly once, uses its output for nothing but
    .shape / .device and as the input of int8 projections (at least one), and does not return it.  All candidates of a block are probed in one run; when that run does not accept all of them, each is probed
    alone (its siblings returning plain tensors) and the survivors once more together.
    candidate (default: the LayerNorm test above): another predicate on a child module — gemma.is_gemma_rmsnorm — selects the norms to probe instead; a candidate
    has a 1-D `weight`, whose length is the probe's width.  With a candidate the probe also reads the state of a model that lives on a GPU through CPU copies
    (Gemma-3's attention applies q_norm / k_norm, modules with a weight of their own): the same answer wherever the model is."""
    cands = {n: m for n, m in block.named_children() if (_is_eligible_layernorm(m) if candidate is None else candidate(m))}
    if not cands:
        return []
    width = next(iter(cands.values())).weight.shape[0]

    def run(under_test):
        rec = _Record()
        try:
            out = _run_probe(block, rec, norms={n: ("probe" if n in under_test else "plain") for n in cands}, width=width, cpu_state=candidate is not None)
        except Exception:          # noqa: BLE001  (whatever the forward raises on the stand-in: refused)
            return []
        if _leaks(out):
            return []
        return [n for n in under_test if len(rec.norm_calls.get(n, [])) == 1 and rec.norm_calls[n][0].uses >= 1]

    good = run(list(cands))
    if len(good) == len(cands) or len(cands) == 1:
        return good
    # one norm's misuse must not cost its sibling: each candidate alone, the others standing in as plain tensors — and then the survivors together
    alone = [n for n in cands if run([n]) == [n]]
    return alone if len(alone) <= 1 or run(alone) == alone else []


def fusable_activation(mlp: nn.Module):
    """(attribute name, kind) when `mlp` is act between two int8 projections: exactly one child module is an activation activation_kind() names, the MLP's own
    forward, run on the CPU against stand-ins, calls it once on the very tensor a projection returned, hands its output to exactly one projection and uses it for
    nothing else (a dropout between the two is a refusal).  None otherwise."""
    if not any(isinstance(c, qlinear) for c in mlp.children()):
        return None
    cands = [(n, activation_kind(m)) for n, m in mlp.named_children() if not _is_int8_proj(m) and not isinstance(m, (nn.Dropout, ActQuant, LayerNormQuant)) and _stateless(m)]
    cands = [(n, k) for n, k in cands if k is not None]
    if len(cands) != 1:
        return None
    name, kind = cands[0]
    first = next(c for c in mlp.children() if isinstance(c, qlinear))
    rec = _Record()
    try:
        out = _run_probe(mlp, rec, acts={name: kind}, width=first.in_features)
    except Exception:          # noqa: BLE001
        return None
    if _leaks(out) or len(rec.act_calls) != 1:
        return None
    x, tok = rec.act_calls[0]
    if tok.uses != 1 or not any(x is o for o in rec.proj_outputs):
        return None
    return name, kind


# ---------------------------------------------------------------- the residual adds fused into the norms that follow them (opt-in)
_CONSTANTS = (type(None), bool, int, float, str)


class ResidualPlan(FlowPlan):
    """What the probe of a block class's forward recorded (residual_flow_plan): the names of the four roles, and the replay of the attention call, the withheld
    parameters, the defaults and the stateless children of a FlowPlan."""

    def __init__(self, cls, n1, attn, n2, mlp, *replay):
        super().__init__(cls, *replay)
        self.n1, self.attn, self.n2, self.mlp = n1, attn, n2, mlp


class _ProbeBlock:
    """Stand-in for `self` in a block class's own forward.  The two LayerNormQuant children and every child that holds parameters or buffers are recorders (the
    roles are told apart by what they are called with); a child without state is an eval-mode copy of the real one; every other attribute is the real block's,
    methods re-bound to the stand-in."""

    def __init__(self, block, run):
        self.__dict__["_block"], self.__dict__["_run"], self.__dict__["_kids"] = block, run, {}

    def __getattr__(self, name):
        v = getattr(self.__dict__["_block"], name)
        if isinstance(v, nn.Module):
            kids = self.__dict__["_kids"]
            if name not in kids:
                kids[name] = self.__dict__["_run"].child(name, v)
            return kids[name]
        if isinstance(v, types.MethodType) and v.__self__ is self.__dict__["_block"]:
            return types.MethodType(v.__func__, self)
        return v


class _ProbeRun:
    """One run of a block forward on exact small integers: the first norm called returns 2 t, the second t / 2 - 3; the child called with the first norm's output
    is the attention and returns (h + 1, None), the child called with the second norm's output is the MLP and returns h * h.  Anything else is a refusal.
    poison: one element of the attention's and one of the MLP's output are +Inf — a use of either that is invisible on finite values (times zero) gives a NaN."""

    def __init__(self, norm_names, poison=False):
        self.poison = poison
        self.norm_names, self.norms, self.norm_out = set(norm_names), [], []          # norms: names in call order; norm_out: the tensors they returned
        self.attn, self.mlp, self.attn_call, self.stateless = None, None, None, []

    def child(self, name, v):
        if name in self.norm_names:
            def norm(t, _name=name):
                if _name in self.norms or len(self.norms) >= 2 or not isinstance(t, torch.Tensor):
                    raise _ProbeRefused(f"{_name} is called twice, or not with a tensor")
                self.norms.append(_name)
                out = t * 2.0 if len(self.norms) == 1 else t * 0.5 - 3.0
                self.norm_out.append(out)
                return out
            return norm
        if isinstance(v, (nn.ModuleList, nn.ModuleDict, nn.Sequential)):
            raise _ProbeRefused(f"forward reads the container {name!r}")
        if _stateless(v):
            self.stateless.append(name)
            return copy.deepcopy(v).eval()

        def callee(*a, _name=name, **kw):
            given = list(a) + list(kw.values())
            if self.norm_out and any(g is self.norm_out[0] for g in given):
                if self.attn is not None:
                    raise _ProbeRefused("the first norm's output is used twice")
                self.attn, self.attn_call = _name, (a, kw)
                return self.poisoned(self.norm_out[0] + 1.0, 0), None
            if len(self.norm_out) == 2 and len(a) == 1 and not kw and a[0] is self.norm_out[1]:
                if self.mlp is not None:
                    raise _ProbeRefused("the second norm's output is used twice")
                self.mlp = _name
                return self.poisoned(a[0] * a[0], -1)
            raise _ProbeRefused(f"{_name} is called with something that is not a norm's output")
        return callee

    def poisoned(self, t, at):
        if self.poison:
            t = t.clone()
            t.view(-1)[at] = float("inf")
        return t


def _probe_block_once(block, cls, norm_names, given, poison=False):
    """cls.forward on a stand-in with the keyword arguments `given`; (run, the formula holds) or raises"""
    run = _ProbeRun(norm_names, poison)
    x = torch.arange(-6, 6, dtype=torch.float32).reshape(1, 3, 4)            # small integers: every operation below is exact
    xin = x.clone()
    with torch.no_grad(), torch.random.fork_rng(devices=[]):
        out = cls.forward(_ProbeBlock(block, run), xin, **given)
    r1 = x + run.poisoned(x * 2.0 + 1.0, 0)
    n2 = r1 * 0.5 - 3.0
    want = r1 + run.poisoned(n2 * n2, -1)
    ok = (isinstance(out, torch.Tensor) and len(run.norms) == 2 and run.attn is not None and run.mlp is not None and out.shape == want.shape
          and out.dtype == want.dtype and torch.equal(out, want) and torch.equal(xin, x))          # (a forward that writes into its input is refused)
    return run, ok


def residual_flow_plan(block: nn.Module, cls=None):
    """A ResidualPlan iff `cls.forward` (default: the block's own class) IS the sequential pre-norm data flow on this block:

        r1 = x + A(N1(x), ...)[0];   out = r1 + M(N2(r1))

    with N1, N2 the block's two LayerNormQuant children, A and M two other children, each of the four called once, nothing else done to the stream (a child
    without state — a dropout — may sit on it as long as the result still EQUALS the formula with that child in eval mode) and a tensor returned.  Probed, not
    pattern-matched: the class's forward runs on a stand-in whose children are cheap exact functions on a tiny CPU tensor.  Every parameter of the forward is given
    a sentinel object; where one arrives in the attention call — positionally or by keyword — is recorded, and so are the constants of that call.  A parameter
    whose sentinel breaks the flow (GPT-2's encoder_hidden_states selects a cross-attention branch) is withheld: left at its default in the probe, and a call that
    sets it runs the original forward.  A second run with every default, and a +Inf planted in the attention's and in the MLP's output, must show the same flow and
    the same call.  None for everything else — a parallel residual
    (GPT-NeoX, Falcon, Phi), a scaled residual, a post-norm, a third norm, an attention output used twice, a forward that writes into its input or that raises."""
    cls = cls or type(block)
    norm_names = [n for n, m in block.named_children() if isinstance(m, LayerNormQuant)]
    if len(norm_names) != 2:
        return None
    found = _probe_flow(block, cls, norm_names, _probe_block_once, lambda run: run.norm_out[0], lambda run: (run.norms, run.attn, run.mlp))
    if found is None:
        return None
    run, run2, args, kwargs, forwards_extra, withheld, defaults, _ = found
    return ResidualPlan(cls, run.norms[0], run.attn, run.norms[1], run.mlp, args, kwargs, forwards_extra, withheld, defaults, sorted(set(run.stateless) | set(run2.stateless)))


def _probe_flow(block, cls, norm_names, probe_once, attn_input, roles):
    """The part of a flow probe that does not depend on the flow: probe_once(block, cls, norm_names, given, poison=...) -> (run, the formula holds) is run with a
    sentinel for every parameter of cls.forward (else with one parameter withheld, else with every parameter that has a default withheld), the attention call of that
    run is recorded entry by entry — attn_input(run) is the tensor that stands in the norm output's place — and a second run with every default and a +Inf planted in
    the attention's and the MLP's output must show the same roles(run) and the same call.  Returns (run, run2, args, kwargs, the block's **kwargs reach the attention,
    withheld, defaults, the keyword arguments of the first run) or None."""
    try:
        ps = list(inspect.signature(cls.forward).parameters.values())[2:]          # (self, hidden_states, ...)
    except (TypeError, ValueError, AttributeError):
        return None
    named = [p for p in ps if p.kind in (p.POSITIONAL_OR_KEYWORD, p.KEYWORD_ONLY)]
    if any(p.kind in (p.POSITIONAL_ONLY, p.VAR_POSITIONAL) for p in ps):
        return None
    var_kw = any(p.kind == p.VAR_KEYWORD for p in ps)
    defaults = {p.name: p.default for p in named if p.default is not p.empty}
    sentinels = {p.name: object() for p in named}
    extra = object()

    def attempt(withhold):
        given = {n: s for n, s in sentinels.items() if n not in withhold}
        if var_kw:
            given["pq_probe_extra"] = extra
        try:
            run, ok = probe_once(block, cls, norm_names, given)
        except Exception:          # noqa: BLE001  (whatever the forward raises on the stand-in: refused)
            return None, None
        return (run, given) if ok else (None, None)

    # every parameter given; else one parameter withheld; else every parameter that has a default withheld
    tries = [()] + [(n,) for n in defaults] + [tuple(defaults)]
    run, given1 = None, None
    for withheld in tries:
        run, given1 = attempt(withheld)
        if run is not None:
            break
    if run is None:
        return None
    by_id = {id(s): n for n, s in sentinels.items()}
    h1 = attn_input(run)

    def entry(v):
        if v is h1:
            return _H
        if id(v) in by_id:
            return ("param", by_id[id(v)])
        if isinstance(v, _CONSTANTS):
            return ("const", v)
        raise _ProbeRefused("the attention is called with something the probe cannot replay")

    a, kw = run.attn_call
    kw = dict(kw)
    forwards_extra = var_kw and kw.pop("pq_probe_extra", None) is extra
    try:
        args, kwargs = [entry(v) for v in a], {k: entry(v) for k, v in kw.items()}
    except _ProbeRefused:
        return None
    if sum(e == _H for e in args) + sum(e == _H for e in kwargs.values()) != 1:
        return None
    seen = {e[1] for e in list(args) + list(kwargs.values()) if e != _H and e[0] == "param"}
    withheld = tuple(n for n in sentinels if n not in seen)
    if any(n not in defaults for n in withheld):          # a required parameter the attention never sees: nothing to fall back on
        return None
    # the same flow with every default (a parameter tested for truth must not change the stream): the recorded call must be the one made there too
    try:
        run2, ok2 = probe_once(block, cls, norm_names, {n: s for n, s in sentinels.items() if n not in defaults}, poison=True)
    except Exception:          # noqa: BLE001
        return None
    if not ok2 or roles(run2) != roles(run):
        return None
    a2, kw2 = run2.attn_call
    h2 = attn_input(run2)

    def same(e, v):
        if e == _H:
            return v is h2
        if e[0] == "param":
            return v is (defaults[e[1]] if e[1] in defaults else sentinels[e[1]])
        return type(v) is type(e[1]) and v == e[1]

    if len(a2) != len(args) or set(kw2) != set(kwargs) or not all(same(e, v) for e, v in zip(args, a2)) or not all(same(kwargs[k], kw2[k]) for k in kwargs):
        return None
    return run, run2, args, kwargs, forwards_extra, withheld, defaults, given1


class ResidualFusedBlock(FusedLayer):
    """A sequential pre-norm decoder block whose two residual adds run inside the LayerNorm + quantisation kernels that follow them (K1al, add_layernorm_quantize):

        h          = the QTensor handed over for this very tensor, else N1(hidden)
        attn_out   = A(...)[0], called the way the block's own forward calls it (ResidualPlan), with h in the norm output's place
        hq, resid  = N2(attn_out, residual=hidden)                               # add + norm + quant, one launch
        m          = M(hq)
        last of the chain:  return resid + m                                     # a torch add
        otherwise:          hq2, out = NEXT block's N1(m, residual=resid);  hand hq2 to the next block;  return out

    What the block returns is the real summed tensor (the bits of the two torch adds: QSPEC A1), so hooks, output_hidden_states and the final norm see what they
    saw.  fuse_layernorm_residual(model) makes a block one by giving the object a class that derives from this one AND from its original class: the object,
    its children under their names (state_dict keys), its other attributes, its hooks and every isinstance check on it stay as they were.  The tensor the block was
    called with is never written; the hand-over is consumed at the next block's entry and never served for another tensor or a tensor changed in place since.
    Whatever the probe did not see — an argument the attention never receives set to something else than its default (GPT-2's encoder_hidden_states), training
    mode with a dropout on the stream — runs the original class's forward for that call."""
    _pq_prefix, _pq_residual_fused = "ResidualFused", True

    def forward(self, *args, **kwargs):
        plan = self._rfb_plan
        given, extras, out = plan.bind(self, args, kwargs)
        if given is None:          # (a call the probe did not cover: the original forward ran)
            return out
        hidden = given[plan.first]
        h = self._rf_inbox.take(hidden)
        if h is None:
            h = getattr(self, plan.n1)(hidden)
        attn_out = plan.replay(self, h, given, extras)[0]
        hq, resid = getattr(self, plan.n2)(attn_out, residual=hidden)
        m = getattr(self, plan.mlp)(hq)
        nxt = self._rf_next[0]
        if nxt is None:
            return resid + m
        hq2, out = getattr(nxt, nxt._rfb_plan.n1)(m, residual=resid)
        nxt._rf_inbox.put(out, hq2)
        return out


def fuse_layernorm_residual(model: nn.Module) -> int:
    """Opt-in, after fuse_layernorm_layers (which it leaves exactly as it was: a separate entry, so nothing changes for a caller who does not ask): every block of a
    ModuleList that has exactly two LayerNormQuant children and whose class's forward passes residual_flow_plan becomes a ResidualFusedBlock (in place).  A refused
    block keeps the fusions it has and breaks the chain (its predecessor ends with a torch add); the model's final norm is not touched.  The module that owns the
    ModuleList gets an always-called forward hook that drops every pending hand-over when its forward ends.  Returns the number of blocks changed by THIS call (a
    second call finds nothing left to change); residual_fused_blocks(model) counts them over all calls.  Composes with fuse_llama_layers in any order."""
    def convert(block):
        if getattr(type(block), "_pq_residual_fused", False):
            return None
        plan = residual_flow_plan(block)
        if plan is None:
            return None
        block._rfb_plan = plan
        return plan.cls
    return fuse_stacks(model, ResidualFusedBlock, convert)          # (a chain that ends, ends with a torch add)


def residual_fused_blocks(model: nn.Module) -> int:
    """the number of ResidualFusedBlock modules in `model` (what fuse_layernorm_residual made, over all calls)"""
    return sum(1 for m in model.modules() if isinstance(m, ResidualFusedBlock))


def fuse_layernorm_layers(model: nn.Module, fuse_norms: bool = True, fuse_act: bool = True) -> int:
    """Apply the two fusions above to every block of `model` (in place) that passes the probes; returns the number of blocks changed.  A block is a module with at
    least one LayerNorm child; its MLP is looked for among its descendants.  Run after swap_linears: a block whose projections are still nn.Linear is left alone,
    as is everything the probes refuse (fusable_norms, fusable_activation say what they require).

    The residual adds of the blocks are a separate, opt-in step: fuse_layernorm_residual(model), afterwards."""
    changed = 0
    for block in reversed(list(model.modules())):          # inner blocks first: an MLP belongs to the innermost block around it
        if not any(isinstance(c, nn.LayerNorm) or isinstance(c, LayerNormQuant) for c in block.children()):
            continue
        did = False
        if fuse_norms:
            for name in fusable_norms(block):
                ln = getattr(block, name)
                setattr(block, name, LayerNormQuant(ln.weight, ln.bias, ln.eps))
                did = True
        if fuse_act:
            for mlp in list(block.modules()):          # (the block itself included: OPT's layers hold fc1 / activation_fn / fc2 themselves)
                found = fusable_activation(mlp)
                if found is not None:
                    setattr(mlp, found[0], ActQuant(found[1]))
                    did = True
        changed += int(did)
    return changed


# ---------------------------------------------------------------- the parallel residual fused into the norm(s) of the next block (opt-in)
_P24 = 16777216.0          # 2^24: in binary32, 2^24 + 1 rounds back to 2^24 — what tells the three groupings of a three-way sum apart


def _assoc_operands():
    """x, attention output, MLP output of the association run: the triple (2^24, -2^24, 1) rotated over three elements.  The three groupings of x + a + m give
    three different vectors: (x + a) + m = [1, 0, 1], (a + m) + x = [1, 1, 0], (x + m) + a = [0, 1, 1] (per group of three elements)."""
    t = torch.tensor([_P24, -_P24, 1.0])
    rot = lambda k: torch.roll(t, k).repeat(4).reshape(1, 3, 4)          # noqa: E731
    return {"x": rot(0), "a": rot(2), "m": rot(1)}


def _rounding_operands():
    """x, attention output, MLP output of the last run: seeded binary32 values of mixed magnitudes, on which every add rounds — a sum that only equals a grouping of
    x + a + m in exact arithmetic (x / 2 + a + m + x / 2) does not give that grouping's bits here"""
    g = torch.Generator().manual_seed(20)
    return {k: torch.randn(1, 3, 4, generator=g) * torch.tensor([1.0, 37.0, 0.01, 1000.0]) for k in ("x", "a", "m")}


_PAIRS = (("x", "a", "m"), ("a", "m", "x"), ("x", "m", "a"))          # (the pair added first, then the third operand)


class ParallelPlan(FlowPlan):
    """What the probe of a block class's forward recorded (parallel_flow_plan): the attention and the MLP, the norm each of them reads (the same one in a block with
    a single norm), `order` — the operands of the three-way sum ("x": the block's input, "a": the attention's output, "m": the MLP's) with the pair that the block
    adds FIRST in front — and the replay of the attention call, the withheld parameters, the defaults and the stateless children of a FlowPlan."""

    def __init__(self, cls, attn, mlp, attn_norm, mlp_norm, order, *replay):
        super().__init__(cls, *replay)
        self.attn, self.mlp, self.attn_norm, self.mlp_norm, self.order = attn, mlp, attn_norm, mlp_norm, tuple(order)
        self.norms = (attn_norm,) if attn_norm == mlp_norm else (attn_norm, mlp_norm)


class _ParallelRun:
    """One run of a block forward for the parallel flow.  Every norm must be called once, WITH THE BLOCK'S INPUT ITSELF: the first one called returns 2 t, the second
    t / 2 - 3.  A child that holds state and is called with a norm's output and nothing else is the MLP and returns h * h; called with a norm's output among other
    arguments it is the attention and returns (h + 1, None).  Anything else is a refusal.  poison: as in _ProbeRun.  fixed: the association run — the attention and the
    MLP return these tensors whatever they are called with."""

    def __init__(self, norm_names, poison=False, fixed=None):
        self.poison, self.fixed, self.x = poison, fixed, None
        self.norm_names, self.norms, self.norm_out = set(norm_names), [], {}          # norms: names in call order; norm_out: name -> the tensor returned
        self.attn, self.mlp, self.attn_call, self.attn_norm, self.mlp_norm, self.stateless = None, None, None, None, None, []

    poisoned = _ProbeRun.poisoned

    def child(self, name, v):
        if name in self.norm_names:
            def norm(t, _name=name):
                if _name in self.norms or t is not self.x:
                    raise _ProbeRefused(f"{_name} is called twice, or with something that is not the block's input")
                self.norms.append(_name)
                out = t * 2.0 if len(self.norms) == 1 else t * 0.5 - 3.0
                self.norm_out[_name] = out
                return out
            return norm
        if isinstance(v, (nn.ModuleList, nn.ModuleDict, nn.Sequential)):
            raise _ProbeRefused(f"forward reads the container {name!r}")
        if _stateless(v):
            self.stateless.append(name)
            return copy.deepcopy(v).eval()

        def callee(*a, _name=name, **kw):
            given = list(a) + list(kw.values())
            hit = [n for n, o in self.norm_out.items() if any(g is o for g in given)]
            if len(hit) != 1:
                raise _ProbeRefused(f"{_name} is called with something that is not one norm's output")
            h = self.norm_out[hit[0]]
            if len(a) == 1 and not kw:
                if self.mlp is not None:
                    raise _ProbeRefused("a second child is called the way the MLP is")
                self.mlp, self.mlp_norm = _name, hit[0]
                return self.fixed["m"].clone() if self.fixed else self.poisoned(h * h, -1)
            if self.attn is not None:
                raise _ProbeRefused("a second child is called the way the attention is")
            self.attn, self.attn_call, self.attn_norm = _name, (a, kw), hit[0]
            return (self.fixed["a"].clone() if self.fixed else self.poisoned(h + 1.0, 0)), None
        return callee

    def roles(self):
        return self.norms, self.attn, self.mlp, self.attn_norm, self.mlp_norm


def _probe_parallel_once(block, cls, norm_names, given, poison=False, fixed=None):
    """cls.forward on a stand-in with the keyword arguments `given`; (run, the formula holds) or raises.  With `fixed` the run records run.orders instead: the
    groupings of the three-way sum that give the block's output bit for bit (not ok when none of the three does)."""
    run = _ParallelRun(norm_names, poison, fixed)
    x = fixed["x"].clone() if fixed else torch.arange(-6, 6, dtype=torch.float32).reshape(1, 3, 4)          # small integers: every operation is exact
    run.x = xin = x.clone()
    with torch.no_grad(), torch.random.fork_rng(devices=[]):
        out = cls.forward(_ProbeBlock(block, run), xin, **given)
    if (not isinstance(out, torch.Tensor) or len(run.norms) != len(run.norm_names) or run.attn is None or run.mlp is None or out.shape != x.shape
            or out.dtype != x.dtype or not torch.equal(xin, x)):          # (a forward that writes into its input is refused)
        return run, False
    if fixed:
        run.orders = [o for o in _PAIRS if torch.equal(out, (fixed[o[0]] + fixed[o[1]]) + fixed[o[2]])]
        return run, bool(run.orders)
    ha, hm = run.norm_out[run.attn_norm], run.norm_out[run.mlp_norm]
    want = (x + run.poisoned(ha + 1.0, 0)) + run.poisoned(hm * hm, -1)          # exact: every grouping gives these bits
    return run, torch.equal(out, want)


def parallel_flow_plan(block: nn.Module, cls=None):
    """A ParallelPlan iff `cls.forward` (default: the block's own class) IS the parallel-residual data flow on this block:

        out = x + A(N1(x), ...)[0] + M(N2(x))          (N2 may be N1: Phi)

    with N1 (N2) the block's one or two LayerNormQuant children, each called once with the block's input itself, A the child called with a norm's output among other
    arguments (it returns a tuple) and M the child called with a norm's output and nothing else, each called once; nothing else done to the stream (a child without
    state — a dropout — may sit on it as long as the result still EQUALS the formula with that child in eval mode) and a tensor returned.  Probed, never matched by
    name, with the machinery of residual_flow_plan: sentinels for the parameters, withheld parameters, a second run with every default and +Inf planted in both
    outputs.  The ASSOCIATION of the three-way sum is probed as well — on exact small integers every grouping gives the same bits, so one more run has the attention
    and the MLP return values that tell the groupings apart in binary32 (_assoc_operands), and a last one values on which every add rounds (_rounding_operands); the
    plan records which pair is added first, and a flow that does not give the bits of one and the same grouping in both runs is refused.  None for everything else: a sequential residual, a scaled sum, a norm applied to anything but the input, a block that returns a
    tuple, a norm that carries a forward or forward-pre hook (the fused block reads the norm's parameters and no longer calls it)."""
    cls = cls or type(block)
    norms = {n: m for n, m in block.named_children() if isinstance(m, LayerNormQuant)}
    if len(norms) not in (1, 2) or any(_hooked(m) for m in norms.values()):
        return None
    found = _probe_flow(block, cls, list(norms), _probe_parallel_once, lambda run: run.norm_out[run.attn_norm], _ParallelRun.roles)
    if found is None:
        return None
    run, run2, args, kwargs, forwards_extra, withheld, defaults, given = found
    try:
        run3, ok3 = _probe_parallel_once(block, cls, list(norms), given, fixed=_assoc_operands())
    except Exception:          # noqa: BLE001
        return None
    if not ok3 or run3.roles() != run.roles() or len(run3.orders) != 1:
        return None
    try:          # the grouping found must also be what the block computes where every add rounds
        run4, ok4 = _probe_parallel_once(block, cls, list(norms), given, fixed=_rounding_operands())
    except Exception:          # noqa: BLE001
        return None
    if not ok4 or run4.roles() != run.roles() or run3.orders[0] not in run4.orders:
        return None
    stateless = sorted(set(run.stateless) | set(run2.stateless) | set(run3.stateless) | set(run4.stateless))
    return ParallelPlan(cls, run.attn, run.mlp, run.attn_norm, run.mlp_norm, run3.orders[0], args, kwargs, forwards_extra, withheld, defaults, stateless)


class ParallelFusedBlock(FusedLayer):
    """A parallel-residual decoder block (GPT-NeoX with use_parallel_residual, Phi) whose three-way sum runs inside the LayerNorm + quantisation kernel of the NEXT
    block (K1pl, add2_layernorm_quantize):

        ha, hm     = the QTensors handed over for this very tensor, else N1 and N2 of hidden in one launch (K1l2, layernorm_quantize2; one norm: K1l)
        attn_out   = A(...)[0], called the way the block's own forward calls it (ParallelPlan), with ha in the norm output's place
        m          = M(hm)
        last of the chain:  return the two torch adds, in the association the probe recorded
        otherwise:          q1[, q2], out = add2_layernorm_quantize(the three operands in that association, the NEXT block's norm parameters);
                            hand the QTensor(s) to the next block;  return out

    What the block returns is the real summed tensor (the bits of the two torch adds in the block's own association: QSPEC A2), so hooks, output_hidden_states and
    the final norm see what they saw.  The norm modules stay the model's, object for object, but are no longer called: only weight / bias / eps are read (which is why
    a block whose norm carries a hook is not converted).  Installed like ResidualFusedBlock — a run-time class deriving from this one and from the original class —
    with the same hand-over discipline and the same fallbacks to the original forward."""
    _pq_prefix, _pq_parallel_fused = "ParallelFused", True

    def forward(self, *args, **kwargs):
        plan = self._pfb_plan
        given, extras, out = plan.bind(self, args, kwargs)
        if given is None:          # (a call the probe did not cover: the original forward ran)
            return out
        hidden = given[plan.first]
        handed = self._rf_inbox.take(hidden)
        if handed is not None:
            ha, hm = handed
        elif len(plan.norms) == 1:
            n1 = getattr(self, plan.attn_norm)
            ha = hm = layernorm_quantize(hidden, n1.weight, n1.bias, n1.eps)
        else:
            n1, n2 = getattr(self, plan.attn_norm), getattr(self, plan.mlp_norm)
            ha, hm = layernorm_quantize2(hidden, n1.weight, n1.bias, n2.weight, n2.bias, n1.eps, n2.eps)
        attn_out = plan.replay(self, ha, given, extras)[0]
        m = getattr(self, plan.mlp)(hm)
        operand = {"x": hidden, "a": attn_out, "m": m}
        p, q, r = (operand[k] for k in plan.order)
        nxt = self._rf_next[0]
        if nxt is None:
            return (p + q) + r
        np_ = nxt._pfb_plan
        n1 = getattr(nxt, np_.attn_norm)
        if len(np_.norms) == 1:
            q1, out = add2_layernorm_quantize(p, q, r, n1.weight, n1.bias, n1.eps)
            q2 = q1
        else:
            n2 = getattr(nxt, np_.mlp_norm)
            q1, q2, out = add2_layernorm_quantize(p, q, r, n1.weight, n1.bias, n1.eps, n2.weight, n2.bias, n2.eps)
        nxt._rf_inbox.put(out, (q1, q2))
        return out


def fuse_parallel_residual(model: nn.Module) -> int:
    """Opt-in, after fuse_layernorm_layers (which it leaves exactly as it was, as it does fuse_layernorm_residual: an entry of its own): every block of a ModuleList
    that has one or two LayerNormQuant children and whose class's forward passes parallel_flow_plan becomes a ParallelFusedBlock (in place).  A refused block keeps
    the fusions it has and breaks the chain (its predecessor ends with the two torch adds); the model's final norm is not touched.  The module that owns the
    ModuleList gets the always-called forward hook that drops every pending hand-over when its forward ends.  Returns the number of blocks changed by THIS call (a
    second call finds nothing left to change); parallel_fused_blocks(model) counts them over all calls.  Families whose norms fuse_layernorm_layers does not turn into
    LayerNormQuant (GPT-J, Falcon, Cohere) have nothing to probe: 0, every module object left alone."""
    def convert(block):
        if getattr(type(block), "_pq_parallel_fused", False) or getattr(type(block), "_pq_residual_fused", False):
            return None
        plan = parallel_flow_plan(block)
        if plan is None:
            return None
        block._pfb_plan = plan
        return plan.cls
    return fuse_stacks(model, ParallelFusedBlock, convert)          # (a chain that ends, ends with the two torch adds)


def parallel_fused_blocks(model: nn.Module) -> int:
    """the number of ParallelFusedBlock modules in `model` (what fuse_parallel_residual made, over all calls)"""
    return sum(1 for m in model.modules() if isinstance(m, ParallelFusedBlock))
