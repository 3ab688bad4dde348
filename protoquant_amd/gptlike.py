"""Call-site integration for decoders built from LayerNorm (with bias) and a plain two-linear MLP with a unary activation — GPT-2, StarCoder2, GPT-NeoX /
Pythia, and whatever else passes the same probes:

* a LayerNorm whose output only feeds int8 projections becomes ``LayerNormQuant`` (``layernorm_quantize``, kernel K1l: the normalised activation never
  reaches HBM; one quantisation serves every projection that reads it);
* the activation between the two projections of the MLP becomes ``ActQuant`` (``act_quantize``, kernel K1u), installed IN PLACE of the MLP's activation
  attribute: the model's own MLP forward, ``c_proj(act(c_fc(x)))``, keeps running — ``qlinear.forward`` accepts the per-token ``QTensor`` — and every
  state-dict key survives.

``swap_linears(model)`` must have run first.  Nothing is recognised by class name or by import: a block's own forward is run on the CPU against stand-ins
(``_Standin``) whose projections are recorders, and a replacement happens only where that run shows the data flow the fused form needs.  A refusal leaves
the module objects untouched.  Composes with ``fuse_llama_layers`` (StarCoder2's q / k / v) in either call order."""
from __future__ import annotations

import inspect
import types

import torch
from torch import nn

from . import _lib as L
from .llama import _FusedSlice
from .qlinear import FusedQLinear, qlinear
from .qtensor import act_quantize, layernorm_quantize


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

    def forward(self, x: torch.Tensor):
        return layernorm_quantize(x, self.weight, self.bias, self.eps)

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
class _ProbeRefused(Exception):
    pass


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

    def __init__(self, mod: nn.Module, rec: _Record, norms=(), acts=()):
        d = self.__dict__
        d["_mod"], d["_rec"], d["_norms"], d["_acts"], d["_kids"] = mod, rec, dict(norms), dict(acts), {}

    def __getattr__(self, name):
        v = getattr(self.__dict__["_mod"], name)
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
        return _Standin(v, rec)


def _leaks(out) -> bool:
    if isinstance(out, _Probed):
        return True
    if isinstance(out, dict):
        return any(_leaks(v) for v in out.values())
    if isinstance(out, (tuple, list)):
        return any(_leaks(v) for v in out)
    return False


def _run_probe(mod: nn.Module, rec: _Record, norms=(), acts=(), width: int | None = None):
    """type(mod).forward on a stand-in of `mod` with a [1, 3, width] CPU tensor of zeros; parameters of the forward that have no default get None, one named
    position_embeddings gets a (cos, sin) pair that broadcasts against any head size.  Raises whatever the forward raises."""
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
        return _Standin(mod, rec, norms, acts)(x, **kw)


def fusable_norms(block: nn.Module) -> list:
    """Names of the LayerNorm children of `block` that may become LayerNormQuant: each is an nn.LayerNorm with nn.LayerNorm's own forward, a 1-D
    normalized_shape and affine parameters, AND the block's own forward, run on the CPU against stand-ins, calls it exactly once, uses its output for nothing but
    .shape / .device and as the input of int8 projections (at least one), and does not return it.  All candidates of a block are probed in one run; when that run does not accept all of them, each is probed
    alone (its siblings returning plain tensors) and the survivors once more together."""
    cands = {n: m for n, m in block.named_children() if _is_eligible_layernorm(m)}
    if not cands:
        return []
    width = next(iter(cands.values())).normalized_shape[0]

    def run(under_test):
        rec = _Record()
        try:
            out = _run_probe(block, rec, norms={n: ("probe" if n in under_test else "plain") for n in cands}, width=width)
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


def fuse_layernorm_layers(model: nn.Module, fuse_norms: bool = True, fuse_act: bool = True) -> int:
    """Apply the two fusions above to every block of `model` (in place) that passes the probes; returns the number of blocks changed.  A block is a module with at
    least one LayerNorm child; its MLP is looked for among its descendants.  Run after swap_linears: a block whose projections are still nn.Linear is left alone,
    as is everything the probes refuse (fusable_norms, fusable_activation say what they require)."""
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
