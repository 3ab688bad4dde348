"""-m gpu: fuse_llama_layers on dense decoders (BASELINE configs[3] and [4]), held to BITS.  tests/llama_twin.py builds tiny Llama / Mistral / Qwen2 / Qwen3 models in code.

a. the fused model — with and without fuse_residual — equals an unfused TWIN whose two norms per layer are the QSPEC norm (llama_twin.twin), bit for bit: logits, every
   hidden state, greedy generation with the KV cache; bf16 / fp16 / f32, q/k/v and MLP biases, GQA with unequal q and kv widths, hidden and intermediate sizes that are
   not multiples of 128 (_padded_forward with a QTensor input inside a real model), the vector row layouts at H = 1024;
b. every call the library's modules receive during a real forward — prefill and decode rows — recomputed on the CPU by the C oracle from the recorded inputs and the float
   weights, and the data flow between the calls (what a module consumed is what the one before it produced);
c. the eager comparison (HF's own norm, which sums in torch's order): identical bits for most seeds, int8 noise behind one flipped rounding for the others — its level
   bounded by four times what was measured, its worst logit by the 3e-2 of tests/test_gpu_llama.py;
d. launch counts: one fused q/k/v GEMM per attention forward, 2L - 1 fused add-norms and one plain norm with fuse_residual.

A mismatch in a. or b. is a bug in llama.py, qlinear.py or a kernel: b.'s message names the module path of the first call that differs."""
import copy
import importlib
import math
import re

import numpy as np
import pytest
import torch

from oracle import c_oracle as C
from tests import addnorm_spec as A
from tests import llama_twin as T
from tests.gpu_util import bits, same, same_f

pytestmark = pytest.mark.gpu
tr = pytest.importorskip("transformers")

DT = {"bf16": (torch.bfloat16, 0), "fp16": (torch.float16, 1), "f32": (torch.float32, 2)}
BIASES = {"attention_bias": True, "mlp_bias": True}


@pytest.fixture(scope="module")
def pq():
    import protoquant_amd
    from protoquant_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available()
    return protoquant_amd


def _trio(pq, family, dt, geometry, layers, seed=0, **cfg):
    """(built, twin, fused, fused with fuse_residual): three models on one set of weights"""
    from protoquant_amd.llama import ResidualFusedLayer, RMSNormQuant, fuse_llama_layers, residual_fused_layers
    b = T.build(family, DT[dt][0], geometry, layers=layers, seed=seed, **cfg)
    swapped = pq.swap_linears(b.model, fuse_gated_mlp=True)
    keys = list(swapped.state_dict().keys())
    tw, fused, fres = T.twin(swapped), copy.deepcopy(swapped), copy.deepcopy(swapped)
    assert fuse_llama_layers(fused) == layers and residual_fused_layers(fused) == 0
    assert fuse_llama_layers(fres, fuse_residual=True) == layers and residual_fused_layers(fres) == layers
    assert all(isinstance(getattr(l, n), RMSNormQuant) for m in (fused, fres) for l in T.decoder_layers(m) for n in T.NORMS)
    assert all(isinstance(l, ResidualFusedLayer) for l in T.decoder_layers(fres))
    # state dict: the twin keeps the swapped model's keys; the fused model holds q / k / v as ONE module and is otherwise the swapped model; fuse_residual adds nothing
    assert list(tw.state_dict().keys()) == keys
    want = [re.sub(r"self_attn\.[qkv]_proj\.(wq|ws|bias)$", r"self_attn.qkv_fused.fused.\1", k) for k in keys]
    fk = list(fused.state_dict().keys())
    assert len(fk) == len(set(fk)) and set(fk) == set(want) and len(set(want)) < len(keys)
    assert list(fres.state_dict().keys()) == fk
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


CASES_A = ([(f, dt, g, {}) for f in T.FAMILIES for dt in ("bf16", "fp16") for g in ("aligned", "ragged")]
           + [("llama", "f32", "aligned", {}), ("llama", "f32", "ragged", {}), ("llama", "bf16", "ragged", BIASES), ("llama", "fp16", "aligned", BIASES),
              ("llama", "bf16", "wide", {})])


@pytest.mark.parametrize("family,dt,geometry,cfg", CASES_A, ids=[f"{f}-{dt}-{g}" + ("-biases" if c else "") for f, dt, g, c in CASES_A])
def test_fused_models_equal_the_qspec_twin_bit_for_bit(pq, family, dt, geometry, cfg):
    layers = 2 if geometry == "wide" else 3          # (3: a first, a middle and a last link of the fuse_residual chain)
    b, tw, fused, fres = _trio(pq, family, dt, geometry, layers, **cfg)
    models = (tw, fused, fres)
    g = torch.Generator().manual_seed(11)
    batches = [torch.randint(0, T.VOCAB, s, generator=g).cuda() for s in ((2, 96), (1, 1), (3, 7), (4, 128))]          # M = 192, 1, 21 and 512 rows
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
    assert not any(l._rf_inbox.pending for l in T.decoder_layers(fres))


def test_a_hidden_state_changed_in_place_between_two_layers_is_normalised_again(pq):
    """a hook that scales layer 0's output IN PLACE (same tensor object, new version): the hand-over layer 0 made for it (fuse_residual) belongs to the old values and
    must not be served — every model sees the changed tensor"""
    b, tw, fused, fres = _trio(pq, "llama", "bf16", "ragged", 3)
    ids = torch.randint(0, T.VOCAB, (2, 24), device="cuda")
    before = _forward_all((tw, fused, fres), ids, "untouched")

    def scale(mod, args, out):
        (out[0] if isinstance(out, tuple) else out).mul_(1.25)
    hs = [T.decoder_layers(m)[0].register_forward_hook(scale) for m in (tw, fused, fres)]
    after = _forward_all((tw, fused, fres), ids, "layer 0's output scaled in place")
    for h in hs:
        h.remove()
    assert not torch.equal(before, after)
    assert not any(l._rf_inbox.pending for l in T.decoder_layers(fres))


def test_a_slice_called_with_another_tensor_inside_the_attention_forward_computes_its_own(pq):
    """while the attention forward holds the fused q/k/v result of ITS hidden states, k_proj / v_proj called with another QTensor (a hook, a recompute) return that
    tensor's projection, not the shared one"""
    from protoquant_amd.qtensor import quantize
    b, tw, fused, fres = _trio(pq, "qwen2", "bf16", "ragged", 2)
    attn = T.decoder_layers(fused)[0].self_attn
    H = b.geometry[0]
    other = quantize(torch.randn(2, 24, H, device="cuda").to(torch.bfloat16))
    with torch.no_grad():
        want = attn.qkv_fused.fused(other)
    got = {}

    def inside(mod, args):
        assert attn.qkv_fused._outs is not None          # (the attention forward is under way)
        got.update(q=attn.q_proj(other), k=attn.k_proj(other), v=attn.v_proj(other))
    h = attn.o_proj.register_forward_pre_hook(inside)
    ids = torch.randint(0, T.VOCAB, (2, 24), device="cuda")          # the same [2, 24] shape: a stale result would pass every shape check
    with torch.no_grad():
        lf = fused(ids).logits
        lt = tw(ids).logits
    h.remove()
    _same_bits(lf, lt, "logits")
    for i, n in enumerate("qkv"):
        _same_bits(got[n].contiguous(), want[i].contiguous(), f"{n}_proj(other) inside the attention forward")


# ---------------------------------------------------------------- b. every library call of a real forward against the C oracle
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
            parts = [C.quant_rowwise(bits(self.W[pre + n + ".weight"]), self.code) for n in names]
            has_bias = [(pre + n + ".bias") in self.W for n in names]
            assert all(has_bias) or not any(has_bias)
            bias = np.concatenate([bits(self.W[pre + n + ".bias"]) for n in names]) if all(has_bias) else None
            self.cache[key] = (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), bias)
        return self.cache[key]

    def gemm(self, codes, scales, layer, *names):
        wq, ws, bias = self.lin(layer, *names)
        return C.qlinear_s8(np.ascontiguousarray(codes), np.ascontiguousarray(scales), wq, ws, bias, self.code)

    def norm_weight(self, layer, name):
        return self.W[f"model.layers.{layer}.{name}.weight"]


def _qt_equal(a: dict, b: dict, what):
    assert a["orig_dtype"] == b["orig_dtype"] and torch.equal(a["int_data"], b["int_data"]) and torch.equal(a["scale"], b["scale"]), what


ROLES = ("", "input_layernorm", "post_attention_layernorm", "self_attn.qkv_fused.fused", "self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj",
         "mlp.gate_up", "mlp.down")


def _audit(calls, built, code, fuse_residual, layers, dtype):
    """One forward's recorded calls: every module's outputs recomputed from ITS recorded inputs by the oracle, and every input traced to the output it must be."""
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
        q, s, _, _ = C.rmsnorm_quant_rowwise(bits(_rows(x_want)), bits(orc.norm_weight(c.layer, name)), orc.eps, code)
        assert c.output["orig_dtype"] == dtype
        same(_rows(c.output["int_data"]), q, c.path + " codes"); same(c.output["scale"], s, c.path + " scales")
        return c.output

    def add_norm(c, x_want, r_want, name):
        assert "residual" in c.inputs, f"{c.path}: a plain norm where the fused add-norm (K1a) belongs"
        assert torch.equal(c.inputs["x"], x_want) and torch.equal(c.inputs["residual"], r_want), f"{c.path}: did not see the two tensors that precede it"
        qt, summed = c.output
        q, s, sb, _ = A.add_rmsnorm_quantize(_rows(x_want), _rows(r_want), orc.norm_weight(c.layer, name), orc.eps)
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
        # the first norm: a plain one on the layer's input — or, in a fuse_residual chain, the add-norm the PREVIOUS layer ran for this one (audited there)
        hq = handed if handed is not None else plain_norm(r["input_layernorm"], x_in, "input_layernorm")
        # q / k / v: one GEMM on those codes; the three projections are its column ranges
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
            assert s.output.shape[-1] == wd, (s.path, tuple(s.output.shape))
            same_f(_rows(s.output), want[:, lo:lo + wd], code, f"{s.path} = columns [{lo}, {lo + wd}) of the fused GEMM")
            lo += wd
        # o_proj: quantises the attention output it is handed (K1) and multiplies
        c = r["self_attn.o_proj"]
        a_out = c.inputs["x"]
        assert a_out.dtype == dtype and a_out.shape[-1] == heads * hd
        oq, os_ = C.quant_rowwise(bits(_rows(a_out)), code)
        same_f(_rows(c.output), orc.gemm(oq, os_, i, "self_attn.o_proj"), code, c.path)
        o_out = c.output
        # the second norm, on the residual stream after the attention
        if fuse_residual:
            hq2, resid = add_norm(r["post_attention_layernorm"], o_out, x_in, "post_attention_layernorm")
        else:
            resid = A.add_a1(o_out, x_in)
            hq2 = plain_norm(r["post_attention_layernorm"], resid, "post_attention_layernorm")
        # the MLP: gate+up on those codes, silu * mul fused into the quantisation of down's input, down
        c = r["mlp.gate_up"]
        _qt_equal(c.inputs["x"], hq2, f"{c.path}: did not consume the second norm's codes")
        want = orc.gemm(_rows(hq2["int_data"]).numpy(), hq2["scale"].numpy(), i, "mlp.gate_proj", "mlp.up_proj")
        gate, up = c.output
        assert gate.shape[-1] == up.shape[-1] == I
        same_f(_rows(torch.cat((gate, up), dim=-1)), want, code, c.path)
        c = r["mlp.down"]
        sq, ss, _ = C.silu_mul_quant_rowwise(bits(_rows(gate)), bits(_rows(up)), code, want_h=False)
        assert c.inputs["x"]["orig_dtype"] == dtype
        same(_rows(c.inputs["x"]["int_data"]), sq, c.path + " input codes"); same(c.inputs["x"]["scale"], ss, c.path + " input scales")
        same_f(_rows(c.output), orc.gemm(sq, ss, i, "mlp.down_proj"), code, c.path)
        d_out = c.output
        # the layer's output: the residual stream after the MLP — from the next layer's add-norm in a fuse_residual chain, a torch add otherwise
        if fuse_residual and i + 1 < layers:
            handed, out_want = add_norm(per[i + 1]["input_layernorm"][0], d_out, resid, "input_layernorm")
        else:
            handed, out_want = None, A.add_a1(d_out, resid)
        assert torch.equal(r[""].output, out_want), f"layer {i}'s output is not its residual stream"
        prev_out = r[""].output


def _check_padded_operands(monkeypatch, geometry):
    """_KPadded's promise, looked at where the GEMM is called: when in_features is not a multiple of 128 BOTH operands arrive zero-tailed (either tail alone keeps the sums
    exact; each is the other's safety net).  Returns the list the number of padded calls is counted in."""
    QL = importlib.import_module("protoquant_amd.qlinear")          # (the module: the package's attribute of that name is the class)
    H, I = T.GEOMETRIES[geometry][:2]
    true_k = {QL._round_k(k): k for k in (H, I) if k % 128}
    seen = []
    real = QL.qlinear_s8

    def checked(xq, xs, wq, ws, bias, out_dtype, out=None):
        k = true_k.get(xq.shape[-1])
        if k is not None:
            assert wq.shape[-1] == xq.shape[-1]
            assert int(torch.count_nonzero(xq[..., k:])) == 0, f"activation codes [{tuple(xq.shape)}]: the padded tail beyond column {k} is not zero"
            assert int(torch.count_nonzero(wq[..., k:])) == 0, f"weight codes [{tuple(wq.shape)}]: the padded tail beyond column {k} is not zero"
            seen.append(k)
        return real(xq, xs, wq, ws, bias, out_dtype, out)
    monkeypatch.setattr(QL, "qlinear_s8", checked)
    return seen, true_k


@pytest.mark.parametrize("fuse_residual", [False, True], ids=["adds-in-torch", "fuse_residual"])
@pytest.mark.parametrize("geometry", ["ragged", "aligned"])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("family", ["llama", "qwen2"])
def test_every_library_call_of_a_forward_matches_the_oracle(pq, monkeypatch, family, dt, geometry, fuse_residual):
    from protoquant_amd.llama import fuse_llama_layers
    layers = 3
    dtype, code = DT[dt]
    b = T.build(family, dtype, geometry, layers=layers, seed=3)
    m = pq.swap_linears(b.model, fuse_gated_mlp=True)
    assert fuse_llama_layers(m, fuse_residual=fuse_residual) == layers
    padded, true_k = _check_padded_operands(monkeypatch, geometry)
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
    # ragged: q/k/v, o, gate_up (K = 320) and down (K = 696) of every layer and the lm_head took the padded path, three forwards; aligned: nobody did
    assert len(padded) == (3 * (4 * layers + 1) if true_k else 0), (len(padded), true_k)


# ---------------------------------------------------------------- c. against HF's own norm
# Measured on an MI355X (Llama, bf16, `aligned`, 2 layers, ids [2, 96]) over seeds 0 .. 31.  The difference is all or nothing: 29 seeds are bit-identical; in three, ONE
# row of one norm rounds another way (HF's RMSNorm sums in torch's order, QSPEC N1-N3 in a pinned one), and from that row on — causally: the later positions of that
# sequence only — every int8 quantisation downstream re-rounds, so those rows carry fresh quantisation noise.  Its size does not depend on the seed:
#
#   seed   max |d|    in bf16 ulps of max |logit|   rms of d over the rows that differ   logits that differ   rows that differ (of 192), from position
#     5    0.01953    2.50                          0.00413                              7.1 %                16, from 79 of sequence 0
#    25    0.01758    2.25                          0.00418                              10.3 %               23, from 57 of sequence 1
#    27    0.02100    2.69                          0.00405                              34.6 %               78, from 15 of sequence 0
#   the other 29:  0
#
# rms 0.0041 is 1.3 % of the logits' standard deviation (0.32 - 0.33; max |logit| 1.25 - 1.63), and the largest of ~10^4 differing logits sits five of those deviations
# out: 0.02 is the tail of int8 noise on the rows behind one flipped rounding, not "a few ulps of a one-code perturbation" — in ulps of the logit's own binade the
# differences run past 8.  So the old absolute bound, 3e-2, was about 1.4 times the honest worst case, and what it could not see is what a. and b. now hold to bits.
# Asserted below: the noise LEVEL at no more than four times what was measured, and the worst logit still within the 3e-2 this repository has held since round 6 (four
# times the worst measured maximum would be 0.084: looser than the bound it replaces).
EAGER_SEEDS = (0, 1, 2, 3, 5, 6, 25, 27)
EAGER_WORST_RMS = 0.00418
EAGER_WORST_MAX = 0.02100


def eager_vs_fused(pq, seed):
    """(max |d|, max |d| in bf16 ulps of max |logit|, max |logit|, share of logits that differ, rms of d over the rows that differ) between the fused model and the
    swapped model with HF's own RMSNorm"""
    from protoquant_amd.llama import fuse_llama_layers
    b = T.build("llama", torch.bfloat16, "aligned", layers=2, seed=seed)
    eager = pq.swap_linears(b.model, fuse_gated_mlp=True)
    fused = copy.deepcopy(eager)
    assert fuse_llama_layers(fused) == 2
    ids = torch.randint(0, T.VOCAB, (2, 96), device="cuda")
    with torch.no_grad():
        a, f = eager(ids).logits.float(), fused(ids).logits.float()
    d = (a - f).abs()
    top, rows = float(a.abs().max()), (d > 0).any(dim=-1)
    ulp = 2.0 ** (math.floor(math.log2(top)) - 7)          # bf16: 8 significant bits
    rms = float(d[rows].pow(2).mean().sqrt()) if bool(rows.any()) else 0.0
    return float(d.max()), float(d.max()) / ulp, top, float((d > 0).float().mean()), rms


def test_fused_model_stays_within_the_measured_distance_of_the_eager_norm(pq):
    seen = {seed: eager_vs_fused(pq, seed) for seed in EAGER_SEEDS}
    for seed, (dmax, ulps, top, share, rms) in seen.items():
        assert rms <= 4 * EAGER_WORST_RMS and dmax <= min(4 * EAGER_WORST_MAX, 3e-2), (seed, seen)
        assert 1.0 < top < 2.0          # (the logits are where they were measured: the figures above mean what they say)


# ---------------------------------------------------------------- d. launch counts
@pytest.mark.parametrize("fuse_residual", [False, True], ids=["adds-in-torch", "fuse_residual"])
def test_launch_counts_on_qwen2(pq, fuse_residual):
    """per forward: ONE fused q/k/v GEMM per attention (the three slices launch none of their own), one gate_up and one down per MLP; with fuse_residual 2L - 1 fused
    add-norms and one plain norm, without it 2L plain norms"""
    from protoquant_amd.llama import fuse_llama_layers
    L = 4
    b = T.build("qwen2", torch.bfloat16, "ragged", layers=L, seed=1)
    m = pq.swap_linears(b.model, fuse_gated_mlp=True)
    assert fuse_llama_layers(m, fuse_residual=fuse_residual) == L
    ids = torch.randint(0, T.VOCAB, (1, 40), device="cuda")
    for rep in range(2):          # (the second forward: nothing was left over from the first)
        with torch.no_grad(), T.record(m) as calls:
            m(ids)
        n = {}
        for c in calls:
            k = c.kind + ("+residual" if c.kind == "norm" and "residual" in c.inputs else "")
            n[k] = n.get(k, 0) + 1
        want = {"layer": L, "qkv": L, "slice": 3 * L, "o_proj": L, "gate_up": L, "down": L}
        want.update({"norm+residual": 2 * L - 1, "norm": 1} if fuse_residual else {"norm": 2 * L})
        assert n == want, (rep, n)
