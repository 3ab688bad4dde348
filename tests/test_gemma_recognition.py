"""CPU: what protoquant_amd/gemma.py recognises, on tiny random-init Gemma, Gemma-2 and Gemma-3 (text) models whose linears were replaced by empty int8 modules
(serialize.prepare_for_int8: no GPU, no quantisation): which norms fuse_gemma_layers replaces and which it leaves alone, object for object; the MLP becoming
GatedMLP(act="gelu_tanh"); the residual fusion accepting Gemma and refusing Gemma-2 and Gemma-3; the norm probe; and that the Llama and the Gemma entry points leave
each other's models alone."""
import pytest
import torch
from torch import nn

tr = pytest.importorskip("transformers")

FAMILIES = {"gemma": ("GemmaConfig", "GemmaForCausalLM"), "gemma2": ("Gemma2Config", "Gemma2ForCausalLM"), "gemma3": ("Gemma3TextConfig", "Gemma3ForCausalLM")}
ALL_NORMS = ("input_layernorm", "post_attention_layernorm", "pre_feedforward_layernorm", "post_feedforward_layernorm")
FUSED = {"gemma": ("input_layernorm", "post_attention_layernorm"), "gemma2": ("input_layernorm", "pre_feedforward_layernorm"),
         "gemma3": ("input_layernorm", "pre_feedforward_layernorm")}
L = 3


def _model(family, swapped=True):
    cname, mname = FAMILIES[family]
    if not (hasattr(tr, cname) and hasattr(tr, mname)):
        pytest.skip(f"the installed transformers has no {mname}")
    torch.manual_seed(0)
    cfg = getattr(tr, cname)(vocab_size=128, hidden_size=64, intermediate_size=128, num_hidden_layers=L, num_attention_heads=4, num_key_value_heads=2, head_dim=16,
                             max_position_embeddings=64)
    model = getattr(tr, mname)(cfg).to(torch.bfloat16).eval()
    with torch.no_grad():
        for m in model.modules():          # transformers initialises the Gemma norm weights to 0
            if type(m).__name__.endswith("RMSNorm"):
                m.weight.copy_((0.3 * torch.randn(m.weight.shape)).to(m.weight.dtype))
    if swapped:
        from protoquant_amd.serialize import prepare_for_int8
        prepare_for_int8(model)
    return model


def _layers(model):
    return list(model.model.layers)


def _norm_objects(model):
    return [{n: getattr(layer, n) for n in ALL_NORMS if hasattr(layer, n)} for layer in _layers(model)]


@pytest.mark.parametrize("family", list(FAMILIES))
def test_what_the_table_of_the_issue_says(family):
    from protoquant_amd.gptlike import activation_kind
    from protoquant_amd.llama import _is_rmsnorm, residual_flow_is_llama
    layer = _layers(_model(family, swapped=False))[0]
    assert residual_flow_is_llama(layer) == (family == "gemma")
    assert not _is_rmsnorm(layer.input_layernorm)
    assert type(layer.mlp.act_fn).__name__ == "GELUTanh" and activation_kind(layer.mlp.act_fn) == "gelu_tanh"


@pytest.mark.parametrize("family", list(FAMILIES))
def test_norms_replaced_and_left_alone_by_identity(family):
    from protoquant_amd import FusedQLinear, GatedMLP, GemmaRMSNormQuant, fuse_gemma_layers
    from protoquant_amd.llama import _FusedSlice, residual_fused_layers
    model = _model(family)
    before = _norm_objects(model)
    final, qk = model.model.norm, [(getattr(l.self_attn, "q_norm", None), getattr(l.self_attn, "k_norm", None)) for l in _layers(model)]
    assert fuse_gemma_layers(model) == L
    for layer, old in zip(_layers(model), before):
        for n, m in old.items():
            now = getattr(layer, n)
            if n in FUSED[family]:
                assert isinstance(now, GemmaRMSNormQuant) and now is not m, (family, n)
                assert torch.equal(now.weight, m.weight) and now.eps == m.eps          # the STORED weight, not 1 + w
                assert not hasattr(now, "variance_epsilon")
            else:
                assert now is m, (family, n)                                             # a post-norm feeds the residual add: the model's module, object for object
        assert isinstance(layer.mlp, GatedMLP) and layer.mlp.act == "gelu_tanh" and isinstance(layer.mlp.gate_up, FusedQLinear)
        assert layer.mlp.gate_up.splits == [128, 128] and layer.mlp.down.in_features == 128
        assert all(isinstance(getattr(layer.self_attn, p), _FusedSlice) for p in ("q_proj", "k_proj", "v_proj"))
        assert layer.self_attn.qkv_fused.fused.splits == [64, 32, 32]
    assert model.model.norm is final                                                     # the final norm stays the model's
    assert qk == [(getattr(l.self_attn, "q_norm", None), getattr(l.self_attn, "k_norm", None)) for l in _layers(model)]
    assert residual_fused_layers(model) == 0                                             # opt-in
    assert fuse_gemma_layers(model) == 0                                                 # nothing left to change


@pytest.mark.parametrize("family", list(FAMILIES))
def test_fuse_residual_accepts_gemma_and_refuses_gemma2_and_gemma3(family):
    from protoquant_amd import fuse_gemma_layers
    from protoquant_amd.llama import ResidualFusedLayer, residual_fused_layers
    model = _model(family)
    classes = [type(l) for l in _layers(model)]
    assert fuse_gemma_layers(model, fuse_residual=True) == L
    if family == "gemma":
        assert residual_fused_layers(model) == L and all(isinstance(l, ResidualFusedLayer) and isinstance(l, c) for l, c in zip(_layers(model), classes))
        assert [l._rf_next[0] for l in _layers(model)] == _layers(model)[1:] + [None]
    else:
        assert residual_fused_layers(model) == 0 and [type(l) for l in _layers(model)] == classes and not hasattr(model.model, "_rf_layers")


def test_switches_select_the_fusions():
    from protoquant_amd import GatedMLP, GemmaRMSNormQuant, fuse_gemma_layers, qlinear
    model = _model("gemma")
    mlps = [l.mlp for l in _layers(model)]
    assert fuse_gemma_layers(model, fuse_mlp=False, fuse_qkv=False) == L
    for layer, mlp in zip(_layers(model), mlps):
        assert layer.mlp is mlp and isinstance(layer.self_attn.q_proj, qlinear) and isinstance(layer.input_layernorm, GemmaRMSNormQuant)
    model = _model("gemma2")
    before = _norm_objects(model)
    assert fuse_gemma_layers(model, fuse_norms=False) == L
    assert _norm_objects(model) == before and all(isinstance(l.mlp, GatedMLP) for l in _layers(model))
    # a model whose linears were not swapped: the norm's consumers are not int8, nothing is replaced
    model = _model("gemma", swapped=False)
    before, mlps = _norm_objects(model), [l.mlp for l in _layers(model)]
    assert fuse_gemma_layers(model, fuse_residual=True) == 0
    assert _norm_objects(model) == before and [l.mlp for l in _layers(model)] == mlps


def test_is_gemma_rmsnorm_is_probed_not_named():
    from transformers.models.gemma.modeling_gemma import GemmaRMSNorm
    from transformers.models.llama.modeling_llama import LlamaRMSNorm

    from protoquant_amd import GemmaRMSNormQuant, is_gemma_rmsnorm

    class OtherForward(GemmaRMSNorm):
        def forward(self, x):
            return super().forward(x) * 2.0

    class LlamaFormUnderGemmaNames(nn.Module):
        def __init__(self, dim, eps=1e-6):
            super().__init__()
            self.weight, self.eps = nn.Parameter(torch.ones(dim)), eps

        def forward(self, x):
            xf = x.float()
            return self.weight * (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + self.eps)).to(x.dtype)

    class SameFormulaOtherName(nn.Module):
        def __init__(self, dim, eps=1e-6):
            super().__init__()
            self.weight, self.eps = nn.Parameter(torch.zeros(dim)), eps

        def forward(self, x):
            y = x.float()
            y = y * torch.rsqrt(y.pow(2).mean(-1, keepdim=True) + self.eps)
            return (y * (1.0 + self.weight.float())).type_as(x)

    class WithBuffer(GemmaRMSNorm):
        def __init__(self, dim):
            super().__init__(dim)
            self.register_buffer("extra", torch.zeros(1))

    assert is_gemma_rmsnorm(GemmaRMSNorm(64)) and is_gemma_rmsnorm(GemmaRMSNorm(7, eps=1e-5).to(torch.bfloat16)) and is_gemma_rmsnorm(SameFormulaOtherName(64))
    for m in (LlamaRMSNorm(64), nn.LayerNorm(64), nn.LayerNorm(64, bias=False), OtherForward(64), LlamaFormUnderGemmaNames(64), WithBuffer(64), nn.Linear(4, 4),
              GemmaRMSNormQuant(torch.zeros(64), 1e-6), torch.zeros(64)):
        assert not is_gemma_rmsnorm(m), type(m).__name__
    # the probe reads the class's forward on a stand-in: the module's own weight is not touched
    n = GemmaRMSNorm(64)
    assert is_gemma_rmsnorm(n) and bool((n.weight == 0).all())


def test_a_llama_model_passed_to_fuse_gemma_layers_is_left_alone():
    from protoquant_amd import fuse_gemma_layers
    from protoquant_amd.serialize import prepare_for_int8
    cfg = tr.LlamaConfig(vocab_size=128, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2)
    model = tr.LlamaForCausalLM(cfg).to(torch.bfloat16).eval()
    prepare_for_int8(model)
    before = {n: m for n, m in model.named_modules()}
    assert fuse_gemma_layers(model, fuse_residual=True) == 0
    assert {n: m for n, m in model.named_modules()} == before and not hasattr(model.model, "_rf_layers")


@pytest.mark.parametrize("family", list(FAMILIES))
def test_a_gemma_model_passed_to_fuse_llama_layers_keeps_its_norms_and_its_mlp(family):
    from protoquant_amd import fuse_llama_layers
    from protoquant_amd.llama import residual_fused_layers
    model = _model(family)
    before, mlps = _norm_objects(model), [l.mlp for l in _layers(model)]
    assert fuse_llama_layers(model, fuse_residual=True) == L                  # q / k / v are fused, as at the parent commit
    assert _norm_objects(model) == before and [l.mlp for l in _layers(model)] == mlps and residual_fused_layers(model) == 0
    # and after fuse_gemma_layers, fuse_llama_layers does not take a GemmaRMSNormQuant for a Llama norm
    from protoquant_amd import GemmaRMSNormQuant, fuse_gemma_layers
    model = _model(family)
    fuse_gemma_layers(model)
    fused = _norm_objects(model)
    fuse_llama_layers(model)
    assert _norm_objects(model) == fused and all(isinstance(o[FUSED[family][0]], GemmaRMSNormQuant) for o in fused)


def test_fusable_norms_default_is_the_layernorm_probe():
    """the candidate predicate generalises the probe and changes nothing for a caller that passes none"""
    import inspect

    from protoquant_amd import gptlike
    sig = inspect.signature(gptlike.fusable_norms)
    assert list(sig.parameters) == ["block", "candidate"] and sig.parameters["candidate"].default is None
    model = _model("gemma")
    assert gptlike.fusable_norms(_layers(model)[0]) == []                     # no nn.LayerNorm child: nothing, as before
    assert gptlike.fusable_norms(_layers(model)[0], candidate=lambda m: False) == []


def test_fuse_residual_touches_the_layers_it_recognised_and_no_others():
    """a Llama model whose norms fuse_llama_layers made RMSNormQuant (its own fuse_residual not asked for) stays without residual fusion when it is handed to
    fuse_gemma_layers(fuse_residual=True): that switch is for the Gemma layers of this call"""
    from protoquant_amd import RMSNormQuant, fuse_gemma_layers, fuse_llama_layers
    from protoquant_amd.llama import residual_fused_layers
    from protoquant_amd.serialize import prepare_for_int8
    cfg = tr.LlamaConfig(vocab_size=128, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2)
    model = tr.LlamaForCausalLM(cfg).to(torch.bfloat16).eval()
    prepare_for_int8(model, fuse_gated_mlp=True)
    assert fuse_llama_layers(model) == 2 and all(isinstance(l.input_layernorm, RMSNormQuant) for l in model.model.layers)
    classes = [type(l) for l in model.model.layers]
    assert fuse_gemma_layers(model, fuse_residual=True) == 0
    assert residual_fused_layers(model) == 0 and [type(l) for l in model.model.layers] == classes and not hasattr(model.model, "_rf_layers")
    fuse_llama_layers(model, fuse_residual=True)          # (the Llama switch still does it)
    assert residual_fused_layers(model) == 2
