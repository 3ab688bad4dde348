"""CPU: the host side of K1a (pq_add_rmsnorm_quant_rowwise / add_rmsnorm_quantize) and of fuse_llama_layers(fuse_residual=True): the symbol is declared, exported and
bound; every bad argument is refused and named before any HIP call; empty problems are no-ops; the Python entry has no CPU path; the code object holds every row
layout without scratch; the decoder-layer probe accepts the Llama data flow and nothing else."""
import importlib
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import addnorm_spec as A
from tests.code_objects import kernels_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYM = "pq_add_rmsnorm_quant_rowwise"


def test_symbol_declared_exported_and_bound():
    from protoquant_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pq_hip.h")).read(), flags=re.S)
    L = _lib.lib()
    assert re.search(r"\b%s\s*\(" % SYM, hdr), f"pq_hip.h does not declare {SYM}"
    assert hasattr(L, SYM) and SYM in _lib.EXPORTS and len(getattr(L, SYM).argtypes) == 17
    assert L.pq_version() == 1                                          # an addition: the ABI version stays
    import protoquant_amd as pq
    assert "add_rmsnorm_quantize" in pq.__all__ and callable(pq.add_rmsnorm_quantize)


def _call(L, **kw):
    """the entry with plausible (never dereferenced) operands, bf16 4 x 128, some arguments overridden"""
    a = dict(x=0x10000, ldx=128, r=0x20000, ldr=128, s=0x30000, lds=128, w=0x40000, eps=1e-6, dtype=0, rows=4, cols=128, q=0x50000, ldq=128, scale=0x60000, h=None, ldh=0)
    a.update(kw)
    return L.pq_add_rmsnorm_quant_rowwise(a["x"], a["ldx"], a["r"], a["ldr"], a["s"], a["lds"], a["w"], a["eps"], a["dtype"], a["rows"], a["cols"], a["q"], a["ldq"],
                                          a["scale"], a["h"], a["ldh"], None)


ROW = 128 * 2          # bytes of one bf16 row


@pytest.mark.parametrize("kw,named", [
    (dict(s=None), b"sum_out is null"), (dict(x=None), b"x is null"), (dict(r=None), b"residual is null"), (dict(w=None), b"weight is null"), (dict(q=None), b"q is null"),
    (dict(scale=None), b"scale is null"), (dict(dtype=3), b"dtype"), (dict(dtype=-1), b"dtype"), (dict(rows=-1), b"rows"), (dict(cols=-1), b"cols"),
    (dict(cols=1 << 24, ldx=1 << 24, ldr=1 << 24, lds=1 << 24, ldq=1 << 24), b"cols"),
    (dict(ldx=64), b"ld_x"), (dict(ldr=64), b"ld_r"), (dict(lds=64), b"ld_s"), (dict(ldq=64), b"ld_q"), (dict(h=0x70000, ldh=64), b"ld_h"),
    (dict(eps=float("nan")), b"eps"), (dict(eps=float("inf")), b"eps"), (dict(eps=-1e-6), b"eps"),
    # sum_out: exactly x / residual is fine (below); anything else that overlaps them is not
    (dict(s=0x10000 + 16), b"sum_out overlaps x"), (dict(s=0x10000 + ROW), b"sum_out overlaps x"), (dict(s=0x10000 - ROW), b"sum_out overlaps x"),
    (dict(s=0x10000, lds=256, ldx=128), b"sum_out overlaps x"),                      # the same pointer, another leading dimension
    (dict(s=0x20000 + 2 * ROW), b"sum_out overlaps residual"), (dict(s=0x40000), b"sum_out overlaps weight"),
    # q, scale, h_out: nothing may overlap them
    (dict(q=0x10000), b"q overlaps x"), (dict(q=0x20000 + 100), b"q overlaps residual"), (dict(q=0x40000 + 8), b"q overlaps weight"), (dict(q=0x30000 + 64), b"q overlaps sum_out"),
    (dict(scale=0x10000 + 4), b"scale overlaps x"), (dict(scale=0x30000), b"scale overlaps sum_out"), (dict(scale=0x50000 + 128), b"q overlaps scale"),
    (dict(h=0x10000, ldh=128), b"h_out overlaps x"), (dict(h=0x20000 + ROW, ldh=128), b"h_out overlaps residual"), (dict(h=0x30000, ldh=128), b"h_out overlaps sum_out"),
    (dict(h=0x50000 + 256, ldh=128), b"q overlaps h_out"), (dict(h=0x60000 - 64, ldh=128), b"scale overlaps h_out"),
])
def test_bad_arguments_are_named_without_a_gpu(kw, named):
    from protoquant_amd import _lib
    L = _lib.lib()
    assert _call(L, **kw) == 1, kw
    err = L.pq_last_error()
    assert SYM.encode() in err and named in err, (kw, err)


def test_allowed_aliases_and_column_blocks_pass_the_checks():
    """sum_out == x, sum_out == residual (same pointer and leading dimension) and disjoint column blocks of one buffer get PAST the argument checks: on a machine without
    a GPU the launch then fails (status 3, not 1); on one with a GPU these never-dereferenced addresses must not be launched, so only the no-GPU case is exercised."""
    from protoquant_amd import _lib
    L = _lib.lib()
    if torch.cuda.is_available():
        pytest.skip("argument-check-only test: needs a machine without a GPU (the operands are not real memory)")
    for kw in (dict(s=0x10000), dict(s=0x20000), dict(x=0x10000, ldx=256, s=0x10000 + ROW, lds=256), dict(x=0x10000, ldx=256, s=0x10000, lds=256)):
        st = _call(L, **kw)
        assert st == 3 and b"overlaps" not in L.pq_last_error(), (kw, st, L.pq_last_error())


def test_empty_problems_are_no_ops_without_a_gpu():
    from protoquant_amd import _lib
    L = _lib.lib()
    assert _call(L, rows=0) == 0
    assert _call(L, cols=0, ldx=0, ldr=0, lds=0, ldq=0) == 0
    assert _call(L, rows=0, x=None, r=None, s=None, w=None, q=None, scale=None) == 0


def test_python_entry_has_no_cpu_fallback_and_checks_its_operands():
    import protoquant_amd as pq
    from protoquant_amd import _lib
    x = torch.zeros(4, 64, dtype=torch.bfloat16)
    w = torch.ones(64, dtype=torch.bfloat16)
    with pytest.raises(_lib.PQError):
        pq.add_rmsnorm_quantize(x, x.clone(), w)
    sig = inspect.signature(pq.add_rmsnorm_quantize)
    assert list(sig.parameters) == ["x", "residual", "weight", "eps", "out", "return_h"]
    assert sig.parameters["eps"].default == 1e-6 and sig.parameters["out"].default is None and sig.parameters["return_h"].default is False


def test_python_entry_refuses_mismatched_operands():
    """the shape / dtype / layout checks, which come after the device check: played on CPU tensors with the device check stubbed out (every case raises before any call
    into the library)"""
    import protoquant_amd as pq
    from protoquant_amd import _lib, qtensor
    x = torch.zeros(4, 64, dtype=torch.bfloat16)
    w = torch.ones(64, dtype=torch.bfloat16)
    orig = _lib.require_gpu
    _lib.require_gpu = lambda t, name: None
    try:
        for bad in (dict(residual=torch.zeros(4, 32, dtype=torch.bfloat16)), dict(residual=torch.zeros(4, 64, dtype=torch.float16)), dict(weight=torch.ones(32, dtype=torch.bfloat16)),
                    dict(weight=torch.ones(64, dtype=torch.float32)), dict(out=torch.zeros(4, 32, dtype=torch.bfloat16)), dict(out=torch.zeros(4, 64, dtype=torch.float16)),
                    dict(out=torch.zeros(64, 4, dtype=torch.bfloat16).t())):
            a = dict(x=x, residual=x.clone(), weight=w)
            a.update(bad)
            with pytest.raises(ValueError):
                pq.add_rmsnorm_quantize(**a)
    finally:
        _lib.require_gpu = orig
    assert qtensor.L.require_gpu is orig


def test_spec_is_the_add_then_the_oracle():
    """tests/addnorm_spec.py: A1 is one binary32 add and one storage rounding — the value torch's eager add stores — and the rest is the existing oracle on the stored sum"""
    from oracle import c_oracle as C
    g = torch.Generator().manual_seed(1)
    for dt, code in ((torch.bfloat16, 0), (torch.float16, 1), (torch.float32, 2)):
        x = torch.randn(5, 96, generator=g).to(dt)
        r = (torch.randn(5, 96, generator=g) * 4).to(dt)
        w = (1 + 0.1 * torch.randn(96, generator=g)).to(dt)
        s = A.add_a1(x, r)
        assert torch.equal(s, r + x) and torch.equal(s, x + r)                       # torch's eager CPU add of two tensors of the storage dtype
        q, sc, sb, h = A.add_rmsnorm_quantize(x, r, w, 1e-5)
        q2, sc2, h2, _ = C.rmsnorm_quant_rowwise(A.to_bits(s), A.to_bits(w), 1e-5, code)
        assert np.array_equal(q, q2) and np.array_equal(sc, sc2) and np.array_equal(h, h2) and np.array_equal(sb, A.to_bits(s))
    # every pair of 16-bit patterns cannot be enumerated; every pattern against a handful can: the f32 add + rounding is what torch stores
    pats = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    for dt in (torch.bfloat16, torch.float16):
        a = pats.view(dt)
        for other in (1.0, -0.5, 3.140625, 1e-3, 300.0, 65504.0, float("inf"), 0.0, -0.0):
            b = torch.full_like(a, other)
            got, want = A.add_a1(a, b), a + b
            nan = torch.isnan(want.float())
            assert torch.equal(torch.isnan(got.float()), nan) and torch.equal(got.view(torch.int16)[~nan], want.view(torch.int16)[~nan]), (dt, other)


def test_code_object_has_every_layout_and_no_scratch():
    """as `make spillcheck` reads the GEMM objects: rmsnorm_quant_rows<.., 64 | 256, .., ADD = true, LlamaGain, QUANT = true> / rmsnorm_quant_generic<.., true, LlamaGain, true> (no multiplier argument) for all three dtypes, with and
    without h_out, none with scratch or spills"""
    kernels, dis = kernels_of("addnorm_kernels", disassembly=True)
    for dt in range(3):
        # wave: 1, 2, 4, 8 vectors per lane; vec: 1, 2, 4, 8, 16 per thread; each with and without h_out; one generic kernel
        assert len([k for k in kernels if re.search(r"\d+rmsnorm_quant_rowsILi%dELi\d+ELi64ELb[01]ELb1ENS_9LlamaGainELb1EJEEE" % dt, k)]) == 4 * 2, dt
        assert len([k for k in kernels if re.search(r"\d+rmsnorm_quant_rowsILi%dELi\d+ELi256ELb[01]ELb1ENS_9LlamaGainELb1EJEEE" % dt, k)]) == 5 * 2, dt
        assert len([k for k in kernels if re.search(r"\d+rmsnorm_quant_genericILi%dELb1ENS_9LlamaGainELb1EJEEE" % dt, k)]) == 1, dt
    assert len(kernels) == 3 * (8 + 10 + 1)
    for k, v in kernels.items():
        assert v.get("private_segment_fixed_size", 1) == 0 and v.get("vgpr_spill_count", 1) == 0 and v.get("sgpr_spill_count", 1) == 0, (k, v)
    assert "global_load_dwordx4" in dis and "global_store_dwordx4" in dis and "v_pk_add_f32" in dis and "scratch_" not in dis


# ---------------------------------------------------------------------------------------------------------------- the decoder-layer probe
def _layer(mod, cfgname, layername, **kw):
    m = pytest.importorskip(f"transformers.models.{mod}.modeling_{mod}")
    c = importlib.import_module(f"transformers.models.{mod}.configuration_{mod}")
    cfg = getattr(c, cfgname)(hidden_size=64, intermediate_size=128, num_attention_heads=4, num_key_value_heads=2, num_hidden_layers=2, vocab_size=128, pad_token_id=0,
                              eos_token_id=1, bos_token_id=2, **kw)
    return getattr(m, layername)(cfg, 0)


ACCEPTED = [("llama", "LlamaConfig", "LlamaDecoderLayer", {}), ("mistral", "MistralConfig", "MistralDecoderLayer", {}), ("qwen2", "Qwen2Config", "Qwen2DecoderLayer", {}),
            ("qwen3", "Qwen3Config", "Qwen3DecoderLayer", {})]
REFUSED = [("granite", "GraniteConfig", "GraniteDecoderLayer", {"residual_multiplier": 0.22}), ("gemma2", "Gemma2Config", "Gemma2DecoderLayer", {"head_dim": 16}),
           ("olmo2", "Olmo2Config", "Olmo2DecoderLayer", {}), ("phi3", "Phi3Config", "Phi3DecoderLayer", {}), ("cohere", "CohereConfig", "CohereDecoderLayer", {})]


@pytest.mark.parametrize("mod,cfgname,layername,kw", ACCEPTED, ids=[a[0] for a in ACCEPTED])
def test_probe_accepts_the_llama_data_flow(mod, cfgname, layername, kw):
    from protoquant_amd.llama import residual_flow_is_llama
    assert residual_flow_is_llama(_layer(mod, cfgname, layername, **kw))


@pytest.mark.parametrize("mod,cfgname,layername,kw", REFUSED, ids=[a[0] for a in REFUSED])
def test_probe_refuses_everything_else(mod, cfgname, layername, kw):
    from protoquant_amd.llama import residual_flow_is_llama
    assert not residual_flow_is_llama(_layer(mod, cfgname, layername, **kw))


def test_probe_refuses_hand_written_variants():
    from torch import nn

    from protoquant_amd.llama import residual_flow_is_llama

    class Base(nn.Module):
        def __init__(self):
            super().__init__()
            self.input_layernorm, self.post_attention_layernorm, self.self_attn, self.mlp = nn.Identity(), nn.Identity(), nn.Identity(), nn.Identity()
            self.drop = nn.Dropout(0.0)

    class Llama(Base):
        def forward(self, hidden_states, attention_mask=None, **kwargs):
            r = hidden_states
            hidden_states = r + self.self_attn(hidden_states=self.input_layernorm(hidden_states), attention_mask=attention_mask, **kwargs)[0]
            return hidden_states + self.mlp(self.post_attention_layernorm(hidden_states))

    class Tuple(Llama):
        def forward(self, hidden_states, attention_mask=None, **kwargs):
            return (super().forward(hidden_states, attention_mask, **kwargs),)

    class Scaled(Llama):
        def forward(self, hidden_states, attention_mask=None, **kwargs):
            return super().forward(hidden_states, attention_mask, **kwargs) * 1.0009765625

    class DropsKwargs(Base):
        def forward(self, hidden_states, attention_mask=None, **kwargs):
            hidden_states = hidden_states + self.self_attn(hidden_states=self.input_layernorm(hidden_states))[0]
            return hidden_states + self.mlp(self.post_attention_layernorm(hidden_states))

    class Dropout(Base):
        def forward(self, hidden_states, **kwargs):
            hidden_states = hidden_states + self.drop(self.self_attn(hidden_states=self.input_layernorm(hidden_states), **kwargs)[0])
            return hidden_states + self.mlp(self.post_attention_layernorm(hidden_states))

    class NormTwice(Base):
        def forward(self, hidden_states, **kwargs):
            hidden_states = hidden_states + self.self_attn(hidden_states=self.input_layernorm(hidden_states), **kwargs)[0]
            return hidden_states + self.mlp(self.post_attention_layernorm(self.post_attention_layernorm(hidden_states)) * 2.0 + 3.0)

    class Raises(Base):
        def forward(self, hidden_states, **kwargs):
            raise RuntimeError("no")

    assert residual_flow_is_llama(Llama())
    for cls in (Tuple, Scaled, DropsKwargs, Dropout, NormTwice, Raises):
        assert not residual_flow_is_llama(cls()), cls.__name__


def test_fuse_residual_is_opt_in_and_probing_changes_nothing():
    from protoquant_amd import llama
    sig = inspect.signature(llama.fuse_llama_layers)
    assert list(sig.parameters) == ["model", "fuse_norms", "fuse_qkv", "fuse_residual"] and sig.parameters["fuse_residual"].default is False
    assert list(inspect.signature(llama.RMSNormQuant.forward).parameters) == ["self", "x", "residual"]
    layer = _layer("llama", "LlamaConfig", "LlamaDecoderLayer")
    before = {k: v.clone() for k, v in layer.state_dict().items()}
    assert llama.residual_flow_is_llama(layer) and type(layer).__name__ == "LlamaDecoderLayer"
    assert all(torch.equal(v, layer.state_dict()[k]) for k, v in before.items())
    # a model whose norms are not RMSNormQuant (nothing was swapped) has nothing to fuse: no layer changes, no hook is installed
    tr = pytest.importorskip("transformers")
    cfg = tr.LlamaConfig(vocab_size=64, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=2)
    model = tr.LlamaModel(cfg)
    assert llama.fuse_llama_layers(model, fuse_residual=True) == 0 and llama.residual_fused_layers(model) == 0 and not hasattr(model, "_rf_layers")


def test_hand_over_is_keyed_consumed_and_never_copied():
    import copy
    import pickle

    from protoquant_amd.llama import _HandOver
    h = _HandOver()
    t, other = torch.zeros(3), torch.zeros(3)
    h.put(t, "q")
    assert h.pending and h.take(other) is None and not h.pending          # another tensor: not served, and gone
    h.put(t, "q")
    assert h.take(t) == "q" and not h.pending and h.take(t) is None      # served once
    h.put(t, "q")
    t.add_(1)                                                             # changed in place since: the version counter moved
    assert h.take(t) is None
    h.put(t, "q")
    assert not copy.deepcopy(h).pending and not pickle.loads(pickle.dumps(h)).pending and h.pending
    with torch.inference_mode():
        u = torch.ones(2)
        h.put(u, "q2")
        assert h.take(u) == "q2"                                          # inference tensors have no version counter: identity alone
