"""-m gpu: fuse_gemma_layers on whole Gemma, Gemma-2 and Gemma-3 (text) decoders, held to BITS.  tests/gemma_twin.py builds tiny models in code.

a. the fused model equals an unfused TWIN (gemma_twin.twin: the fusable norms return the stored h of gemma_rmsnorm_quantize, the MLP is down(quantize(stored h of
   gelu_mul_quantize)) over separate gate / up projections), bit for bit: logits, every hidden state, greedy generation with the KV cache — Gemma at the `aligned` and
   `ragged` geometries in bf16 and fp16 and once in f32, Gemma-2 and Gemma-3 at `aligned` in bf16; Gemma with fuse_residual=True against the same model without it and
   against the twin;
b. every call the library's modules receive during a prefill and two decode steps, recomputed on the CPU from the recorded inputs and the float weights — the norms
   and the GeGLU by tests/gemma_spec.py, the GEMMs by the C oracle — and the data flow between the calls;
c. the per-layer module call counts: two norm kernels, one q/k/v GEMM, o, gate+up, one K1gg, down; with fuse_residual 2L - 1 K1ang calls and one K1ng per forward;
d. the cosine of all logits to the unquantised bf16 model, >= 0.99.  Measured on an MI355X (2 layers, `aligned`, ids [2, 96]): Gemma 0.99995, Gemma-2 0.99948,
   Gemma-3 0.99946."""
import copy
import importlib

import numpy as np
import pytest
import torch

from oracle import c_oracle as C
from tests import addnorm_spec as A
from tests import gemma_spec as G
from tests import gemma_twin as T
from tests.gpu_util import bits, same, same_f

pytestmark = pytest.mark.gpu
tr = pytest.importorskip("transformers")

DT = {"bf16": (torch.bfloat16, 0), "fp16": (torch.float16, 1), "f32": (torch.float32, 2)}


@pytest.fixture(scope="module")
def pq():
    import protoquant_amd
    from protoquant_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available()
    return protoquant_amd


def _models(pq, family, dt, geometry, layers, seed=0):
    """(built, twin, fused, fused with fuse_residual): models on one set of weights"""
    from protoquant_amd.llama import ResidualFusedLayer, residual_fused_layers
    b = T.build(family, DT[dt][0], geometry, layers=layers, seed=seed)
    swapped = pq.swap_linears(b.model)
    tw, fused, fres = T.twin(swapped, family), copy.deepcopy(swapped), copy.deepcopy(swapped)
    assert pq.fuse_gemma_layers(fused) == layers and residual_fused_layers(fused) == 0
    assert pq.fuse_gemma_layers(fres, fuse_residual=True) == layers
    assert residual_fused_layers(fres) == (layers if family == "gemma" else 0)          # Gemma-2 and Gemma-3 are refused and run as before
    for m in (fused, fres):
        for l in T.decoder_layers(m):
            assert [n for n in T.ALL_NORMS if isinstance(getattr(l, n, None), pq.GemmaRMSNormQuant)] == list(T.FUSED_NORMS[family])
            assert isinstance(l.mlp, pq.GatedMLP) and l.mlp.act == "gelu_tanh"
    if family == "gemma":
        assert all(isinstance(l, ResidualFusedLayer) for l in T.decoder_layers(fres))
    return b, tw, fused, fres


def _same_bits(a: torch.Tensor, b: torch.Tensor, what):
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} elements differ, max |d| {float((a.float() - b.float()).abs().max())}"


def _forward_all(models, ids, what):
    """one forward of the twin and of every fused model; logits and every hidden state equal the twin's bits.  Returns the twin's logits."""
    with torch.no_grad():
        outs = [m(ids, output_hidden_states=True) for m in models]
    for name, o in zip(("fused", "fused + residual"), outs[1:]):
        _same_bits(o.logits, outs[0].logits, f"{what}: {name} logits")
        assert len(o.hidden_states) == len(outs[0].hidden_states)
        for i, (h, hw) in enumerate(zip(o.hidden_states, outs[0].hidden_states)):
            _same_bits(h, hw, f"{what}: {name} hidden state {i}")
    return outs[0].logits


CASES_A = ([("gemma", dt, g) for dt in ("bf16", "fp16") for g in ("aligned", "ragged")] + [("gemma", "f32", "aligned"), ("gemma2", "bf16", "aligned"),
                                                                                           ("gemma3", "bf16", "aligned")])


@pytest.mark.parametrize("family,dt,geometry", CASES_A, ids=["-".join(c) for c in CASES_A])
def test_fused_models_equal_the_twin_bit_for_bit(pq, family, dt, geometry):
    layers = 3          # (a first, a middle and a last link of the fuse_residual chain)
    b, tw, fused, fres = _models(pq, family, dt, geometry, layers)
    models = (tw, fused, fres)
    g = torch.Generator().manual_seed(11)
    batches = [torch.randint(0, T.VOCAB, s, generator=g).cuda() for s in ((2, 96), (1, 1), (3, 7))]          # M = 192, 1 and 21 rows
    first = [_forward_all(models, ids, f"ids {tuple(ids.shape)}") for ids in batches]
    assert all(torch.isfinite(l.float()).all() for l in first)
    # the same ids objects, other hidden states: nothing computed for the first forward may be served again
    with torch.no_grad():
        for m in models:
            m.model.embed_tokens.weight.mul_(1.5)
    for ids, l1 in zip(batches, first):
        l2 = _forward_all(models, ids, f"ids {tuple(ids.shape)} after the embedding changed in place")
        assert not torch.equal(l1, l2)
    # decode: one token per step against the KV cache
    with torch.no_grad():
        gen = [m.generate(batches[0][:, :16], max_new_tokens=16, min_new_tokens=16, do_sample=False, use_cache=True, pad_token_id=0) for m in models]
    assert gen[0].shape == (2, 32)
    assert torch.equal(gen[1], gen[0]) and torch.equal(gen[2], gen[0]), "greedy generation differs from the twin's"
    for m in (fused, fres):
        assert all(l.self_attn.qkv_fused._outs is None and l.self_attn.qkv_fused._key is None for l in T.decoder_layers(m))
    if family == "gemma":
        assert not any(l._rf_inbox.pending for l in T.decoder_layers(fres))


# ---------------------------------------------------------------- b. every library call of a real forward against the specification
def _rows(t: torch.Tensor) -> torch.Tensor:
    return t.reshape(-1, t.shape[-1])


class _Oracle:
    """the float weights of the model, quantised per output channel by the C oracle (Q1-Q6), by projection names under a layer"""

    def __init__(self, built, code):
        self.W, self.code, self.eps = built.weights, code, float(built.config.rms_norm_eps)
        self.cache = {}

    def lin(self, layer, *names):
        key = (layer, names)
        if key not in self.cache:
            pre = f"model.layers.{layer}."
            assert not any((pre + n + ".bias") in self.W for n in names)
            parts = [C.quant_rowwise(bits(self.W[pre + n + ".weight"]), self.code) for n in names]
            self.cache[key] = (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))
        return self.cache[key]

    def gemm(self, codes, scales, layer, *names):
        wq, ws = self.lin(layer, *names)
        return C.qlinear_s8(np.ascontiguousarray(codes), np.ascontiguousarray(scales), wq, ws, None, self.code)

    def norm_weight(self, layer, name):
        return self.W[f"model.layers.{layer}.{name}.weight"]


def _qt_equal(a: dict, b: dict, what):
    assert a["orig_dtype"] == b["orig_dtype"] and torch.equal(a["int_data"], b["int_data"]) and torch.equal(a["scale"], b["scale"]), what


ROLES = ("", "input_layernorm", "post_attention_layernorm", "self_attn.qkv_fused.fused", "self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj",
         "mlp.gate_up", "mlp.down")


def _audit(calls, built, code, fuse_residual, layers, dtype):
    """One forward's recorded calls of a Gemma (v1) model: every module's outputs recomputed from ITS recorded inputs, and every input traced to the output it must be."""
    orc = _Oracle(built, code)
    H, I, heads, kv, hd = built.geometry
    widths = (heads * hd, kv * hd, kv * hd)
    per = {}
    for c in calls:
        per.setdefault(c.layer, {}).setdefault(c.role, []).append(c)
    assert sorted(per) == list(range(layers))
    for i in range(layers):
        assert {r: len(v) for r, v in per[i].items()} == {r: 1 for r in ROLES}, (i, {r: len(v) for r, v in per[i].items()})

    def plain_norm(c, x_want, name):
        assert "residual" not in c.inputs, f"{c.path}: a fused add-norm where a plain norm belongs"
        assert torch.equal(c.inputs["x"], x_want), f"{c.path}: did not see the tensor that precedes it"
        q, s, _ = G.gemma_rmsnorm_quantize_t(_rows(x_want), orc.norm_weight(c.layer, name), orc.eps)
        assert c.output["orig_dtype"] == dtype
        same(_rows(c.output["int_data"]), q, c.path + " codes"); same(c.output["scale"], s, c.path + " scales")
        return c.output

    def add_norm(c, x_want, r_want, name):
        assert "residual" in c.inputs, f"{c.path}: a plain norm where the fused add-norm (K1ang) belongs"
        assert torch.equal(c.inputs["x"], x_want) and torch.equal(c.inputs["residual"], r_want), f"{c.path}: did not see the two tensors that precede it"
        qt, summed = c.output
        q, s, sb, _ = G.add_gemma_rmsnorm_quantize(_rows(x_want), _rows(r_want), orc.norm_weight(c.layer, name), orc.eps)
        assert qt["orig_dtype"] == dtype and summed.shape == x_want.shape
        same(_rows(qt["int_data"]), q, c.path + " codes"); same(qt["scale"], s, c.path + " scales"); same(_rows(summed), sb, c.path + " sum")
        assert torch.equal(summed, r_want + x_want), f"{c.path}: the returned sum is not the torch add of its inputs"
        return qt, summed

    prev_out, handed = None, None
    for i in range(layers):
        r = {k: v[0] for k, v in per[i].items()}
        x_in = r[""].inputs["x"]
        if prev_out is not None:
            assert torch.equal(x_in, prev_out), f"layer {i} did not receive layer {i - 1}'s output"
        hq = handed if handed is not None else plain_norm(r["input_layernorm"], x_in, "input_layernorm")
        c = r["self_attn.qkv_fused.fused"]
        _qt_equal(c.inputs["x"], hq, f"{c.path}: did not consume the first norm's codes")
        want = orc.gemm(_rows(hq["int_data"]).numpy(), hq["scale"].numpy(), i, "self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj")
        assert tuple(o.shape[-1] for o in c.output) == widths, (c.path, [tuple(o.shape) for o in c.output])
        same_f(_rows(torch.cat(c.output, dim=-1)), want, code, c.path)
        lo = 0
        for idx, (n, wd) in enumerate(zip("qkv", widths)):
            s = r[f"self_attn.{n}_proj"]
            assert s.inputs["index"] == idx
            _qt_equal(s.inputs["x"], hq, f"{s.path}: called with another tensor than the fused GEMM")
            same_f(_rows(s.output), want[:, lo:lo + wd], code, f"{s.path} = columns [{lo}, {lo + wd}) of the fused GEMM")
            lo += wd
        c = r["self_attn.o_proj"]
        a_out = c.inputs["x"]
        assert a_out.dtype == dtype and a_out.shape[-1] == heads * hd
        oq, os_ = C.quant_rowwise(bits(_rows(a_out)), code)
        same_f(_rows(c.output), orc.gemm(oq, os_, i, "self_attn.o_proj"), code, c.path)
        o_out = c.output
        if fuse_residual:
            hq2, resid = add_norm(r["post_attention_layernorm"], o_out, x_in, "post_attention_layernorm")
        else:
            resid = A.add_a1(o_out, x_in)
            hq2 = plain_norm(r["post_attention_layernorm"], resid, "post_attention_layernorm")
        # the MLP: gate+up on those codes, gelu_tanh * mul fused into the quantisation of down's input (K1gg), down
        c = r["mlp.gate_up"]
        _qt_equal(c.inputs["x"], hq2, f"{c.path}: did not consume the second norm's codes")
        want = orc.gemm(_rows(hq2["int_data"]).numpy(), hq2["scale"].numpy(), i, "mlp.gate_proj", "mlp.up_proj")
        gate, up = c.output
        assert gate.shape[-1] == up.shape[-1] == I
        same_f(_rows(torch.cat((gate, up), dim=-1)), want, code, c.path)
        c = r["mlp.down"]
        sq, ss, _ = G.gelu_mul_quantize_t(_rows(gate).contiguous(), _rows(up).contiguous())
        assert c.inputs["x"]["orig_dtype"] == dtype
        same(_rows(c.inputs["x"]["int_data"]), sq, c.path + " input codes"); same(c.inputs["x"]["scale"], ss, c.path + " input scales")
        same_f(_rows(c.output), orc.gemm(sq, ss, i, "mlp.down_proj"), code, c.path)
        d_out = c.output
        if fuse_residual and i + 1 < layers:
            handed, out_want = add_norm(per[i + 1]["input_layernorm"][0], d_out, resid, "input_layernorm")
        else:
            handed, out_want = None, A.add_a1(d_out, resid)
        assert torch.equal(r[""].output, out_want), f"layer {i}'s output is not its residual stream"
        prev_out = r[""].output


CASES_B = [("bf16", "aligned", False), ("bf16", "aligned", True), ("bf16", "ragged", True), ("fp16", "ragged", False)]


@pytest.mark.parametrize("dt,geometry,fuse_residual", CASES_B, ids=[f"{d}-{g}-" + ("fuse_residual" if f else "adds-in-torch") for d, g, f in CASES_B])
def test_every_library_call_of_a_forward_matches_the_spec(pq, dt, geometry, fuse_residual):
    layers = 3
    dtype, code = DT[dt]
    b = T.build("gemma", dtype, geometry, layers=layers, seed=3)
    m = pq.swap_linears(b.model)
    assert pq.fuse_gemma_layers(m, fuse_residual=fuse_residual) == layers
    ids = torch.randint(0, T.VOCAB, (2, 40), device="cuda")
    with torch.no_grad(), T.record(m) as calls:
        out = m(ids, use_cache=True)
    assert calls[0].inputs["x"].shape[:2] == (2, 40)
    _audit(calls, b, code, fuse_residual, layers, dtype)
    for step in range(2):          # decode rows: one token per sequence against the cache
        tok = out.logits[:, -1].argmax(dim=-1, keepdim=True)
        with torch.no_grad(), T.record(m) as calls:
            out = m(tok, past_key_values=out.past_key_values, use_cache=True)
        assert calls[0].inputs["x"].shape[:2] == (2, 1), f"decode step {step}"
        _audit(calls, b, code, fuse_residual, layers, dtype)


# ---------------------------------------------------------------- c. call counts
@pytest.mark.parametrize("fuse_residual", [False, True], ids=["adds-in-torch", "fuse_residual"])
def test_call_counts_on_gemma(pq, monkeypatch, fuse_residual):
    """per forward and layer: two norm kernels, ONE fused q/k/v GEMM (the three slices launch none of their own), o, one gate+up, ONE K1gg, one down; with
    fuse_residual 2L - 1 fused add-norms (K1ang) and one plain norm (K1ng), without it 2L plain norms"""
    QL = importlib.import_module("protoquant_amd.qlinear")          # (the module: the package's attribute of that name is the class)
    GM = importlib.import_module("protoquant_amd.gemma")
    L = 4
    b = T.build("gemma", torch.bfloat16, "ragged", layers=L, seed=1)
    m = pq.swap_linears(b.model)
    assert pq.fuse_gemma_layers(m, fuse_residual=fuse_residual) == L
    kernels = {"K1gg": 0, "K1ng": 0, "K1ang": 0, "K1s": 0}

    def counting(name, fn):
        def run(*a, **kw):
            kernels[name] += 1
            return fn(*a, **kw)
        return run
    monkeypatch.setattr(QL, "gelu_mul_quantize", counting("K1gg", QL.gelu_mul_quantize))
    monkeypatch.setattr(QL, "silu_mul_quantize", counting("K1s", QL.silu_mul_quantize))
    monkeypatch.setattr(GM, "gemma_rmsnorm_quantize", counting("K1ng", GM.gemma_rmsnorm_quantize))
    monkeypatch.setattr(GM, "add_gemma_rmsnorm_quantize", counting("K1ang", GM.add_gemma_rmsnorm_quantize))
    ids = torch.randint(0, T.VOCAB, (1, 40), device="cuda")
    for rep in range(2):          # (the second forward: nothing was left over from the first)
        for k in kernels:
            kernels[k] = 0
        with torch.no_grad(), T.record(m) as calls:
            m(ids)
        n = {}
        for c in calls:
            k = c.kind + ("+residual" if c.kind == "norm" and "residual" in c.inputs else "")
            n[k] = n.get(k, 0) + 1
        want = {"layer": L, "qkv": L, "slice": 3 * L, "o_proj": L, "gate_up": L, "down": L}
        want.update({"norm+residual": 2 * L - 1, "norm": 1} if fuse_residual else {"norm": 2 * L})
        assert n == want, (rep, n)
        assert kernels == ({"K1gg": L, "K1ng": 1, "K1ang": 2 * L - 1, "K1s": 0} if fuse_residual else {"K1gg": L, "K1ng": 2 * L, "K1ang": 0, "K1s": 0}), (rep, kernels)


# ---------------------------------------------------------------- d. against the unquantised model
@pytest.mark.parametrize("family", list(T.FAMILIES))
def test_cosine_of_all_logits_to_the_unquantised_model(pq, family):
    b = T.build(family, torch.bfloat16, "aligned", layers=2, seed=0)
    ref = copy.deepcopy(b.model)
    m = pq.swap_linears(b.model)
    assert pq.fuse_gemma_layers(m, fuse_residual=True) == 2
    ids = torch.randint(0, T.VOCAB, (2, 96), generator=torch.Generator().manual_seed(5)).cuda()
    with torch.no_grad():
        a, f = ref(ids).logits.float().flatten(), m(ids).logits.float().flatten()
    cos = float(torch.dot(a, f) / (a.norm() * f.norm()))
    print(f"{family}: cosine of all logits, fused int8 model against the unquantised bf16 model: {cos:.5f}")
    assert cos >= 0.99
