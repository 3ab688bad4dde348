"""CPU: what protoquant_amd/qk_norm.py recognises.  head_norm_kind on the stock norm classes of transformers and on look-alikes; fuse_qk_norms on tiny random-init Qwen3,
Qwen3-MoE and Gemma-3 (text) models — which modules it replaces, with the same weight objects and state-dict keys — and on the models it must leave alone object for
object (OLMo-2, Llama, Cohere with use_qk_norm); and the order requirement: called BEFORE fuse_gemma_layers it makes that entry refuse the norms (it fails safe)."""
import pytest
import torch
from torch import nn

tr = pytest.importorskip("transformers")

from tests import moe_models as M  # noqa: E402
from tests.test_gemma_recognition import _model as _gemma_model  # noqa: E402  (the tiny Gemma models of the Gemma recognition tests)

L = 3


def _tiny(cname, mname, **over):
    if not (hasattr(tr, cname) and hasattr(tr, mname)):
        pytest.skip(f"the installed transformers has no {mname}")
    kw = dict(vocab_size=128, hidden_size=64, intermediate_size=128, num_hidden_layers=L, num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=64)
    kw.update(over)
    torch.manual_seed(0)
    return getattr(tr, mname)(getattr(tr, cname)(**kw)).to(torch.bfloat16).eval()


def _qwen3(swapped=False):
    m = _tiny("Qwen3Config", "Qwen3ForCausalLM", head_dim=16)
    if swapped:
        from protoquant_amd.serialize import prepare_for_int8
        prepare_for_int8(m, fuse_gated_mlp=True)
    return m


def _attentions(model):
    return [m for m in model.modules() if hasattr(m, "q_norm") and hasattr(m, "k_norm")]


def _stock(path, cls):
    mod = pytest.importorskip(path)
    return getattr(mod, cls)


# ---------------------------------------------------------------------------------------------------------------- the probe
@pytest.mark.parametrize("path,cls,want", [
    ("transformers.models.qwen3.modeling_qwen3", "Qwen3RMSNorm", "llama"), ("transformers.models.llama.modeling_llama", "LlamaRMSNorm", "llama"),
    ("transformers.models.qwen3_moe.modeling_qwen3_moe", "Qwen3MoeRMSNorm", "llama"),
    ("transformers.models.gemma3.modeling_gemma3", "Gemma3RMSNorm", "gemma"), ("transformers.models.gemma.modeling_gemma", "GemmaRMSNorm", "gemma"),
    ("transformers.models.olmo2.modeling_olmo2", "Olmo2RMSNorm", None)])
@pytest.mark.parametrize("width", [16, 64, 128, 256])
def test_head_norm_kind_on_the_stock_classes(path, cls, want, width):
    from protoquant_amd import head_norm_kind
    for dt in (torch.bfloat16, torch.float32):          # the module's own dtype does not matter: the probe runs the class's forward in bf16 AND in f32
        m = _stock(path, cls)(width, eps=1e-6).to(dt)
        with torch.no_grad():
            m.weight.copy_(0.5 * torch.randn(width))
        assert head_norm_kind(m) == want, (cls, width, dt)


def test_head_norm_kind_refuses_everything_else():
    from protoquant_amd import HeadRMSNorm, OlmoRMSNorm, head_norm_kind
    Qwen3RMSNorm = _stock("transformers.models.qwen3.modeling_qwen3", "Qwen3RMSNorm")
    assert head_norm_kind(nn.LayerNorm(64)) is None and head_norm_kind(nn.LayerNorm(64, bias=False)) is None
    assert head_norm_kind(nn.Linear(8, 8)) is None and head_norm_kind(None) is None and head_norm_kind(torch.ones(4)) is None

    class Centred(Qwen3RMSNorm):          # a subclass with another forward
        def forward(self, x):
            return super().forward(x - x.mean(-1, keepdim=True))

    class Doubled(Qwen3RMSNorm):
        def forward(self, x):
            return 2 * super().forward(x)

    class Raises(Qwen3RMSNorm):
        def forward(self, x):
            raise RuntimeError("no")

    class WithBuffer(Qwen3RMSNorm):       # the stock forward, one buffer more
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.register_buffer("running", torch.zeros(1))

    class WithChild(Qwen3RMSNorm):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.drop = nn.Dropout(0.0)

    for cls in (Centred, Doubled, Raises, WithBuffer, WithChild):
        assert head_norm_kind(cls(64, eps=1e-6)) is None, cls.__name__

    class Same(Qwen3RMSNorm):             # a subclass that keeps the forward is still the Llama norm
        pass
    assert head_norm_kind(Same(64, eps=1e-6)) == "llama"
    two_d = Qwen3RMSNorm(64, eps=1e-6)
    two_d.weight = nn.Parameter(torch.ones(4, 16))          # Cohere's per-head weight
    assert head_norm_kind(two_d) is None
    no_eps = Qwen3RMSNorm(64, eps=1e-6)
    no_eps.variance_epsilon = None
    assert head_norm_kind(no_eps) is None
    w = nn.Parameter(torch.ones(64))
    assert head_norm_kind(HeadRMSNorm(w, 1e-6, "llama")) is None and head_norm_kind(OlmoRMSNorm(w, 1e-6)) is None


def test_head_rmsnorm_module_keeps_the_weight_object_and_the_name_of_eps():
    from protoquant_amd import HeadRMSNorm
    w = nn.Parameter(torch.ones(16, dtype=torch.bfloat16))
    a, b = HeadRMSNorm(w, 1e-5, "llama"), HeadRMSNorm(w, 1e-6, "gemma", eps_name="eps")
    assert a.weight is w and b.weight is w and a.variance_epsilon == 1e-5 and b.eps == 1e-6 and not hasattr(a, "eps") and not hasattr(b, "variance_epsilon")
    assert list(a.state_dict()) == ["weight"] and list(b.state_dict()) == ["weight"]
    assert "per head, one launch" in repr(a) and "gain 1 + w" in repr(b) and "gain 1 + w" not in repr(a)


# ---------------------------------------------------------------------------------------------------------------- the models it takes
def _taken(model, kind, eps_name, layers):
    from protoquant_amd import HeadRMSNorm, fuse_qk_norms
    attns = _attentions(model)
    assert len(attns) == layers
    before = [(a.q_norm, a.k_norm) for a in attns]
    keys, ptrs = list(model.state_dict()), {k: v.data_ptr() for k, v in model.state_dict().items()}
    others = {n: m for n, m in model.named_modules() if not n.endswith(("q_norm", "k_norm"))}
    assert fuse_qk_norms(model) == 2 * layers
    for a, (q0, k0) in zip(attns, before):
        for new, old in ((a.q_norm, q0), (a.k_norm, k0)):
            assert isinstance(new, HeadRMSNorm) and new.kind == kind and new.weight is old.weight and new.weight.shape == (a.head_dim,)
            assert getattr(new, eps_name) == getattr(old, eps_name) and new._eps_name == eps_name
    assert list(model.state_dict()) == keys and {k: v.data_ptr() for k, v in model.state_dict().items()} == ptrs
    assert {n: m for n, m in model.named_modules() if not n.endswith(("q_norm", "k_norm"))} == others          # every other module: the very same object
    assert fuse_qk_norms(model) == 0                                                                             # a second call finds nothing left


@pytest.mark.parametrize("swapped", [False, True], ids=["float", "int8"])
def test_qwen3_is_taken(swapped):
    _taken(_qwen3(swapped), "llama", "variance_epsilon", L)


def test_qwen3_moe_is_taken():
    if not hasattr(tr, "Qwen3MoeConfig"):
        pytest.skip("the installed transformers has no Qwen3-MoE")
    _taken(M.build("qwen3_moe").to(torch.bfloat16), "llama", "variance_epsilon", 2)


@pytest.mark.parametrize("swapped", [False, True], ids=["float", "int8"])
def test_gemma3_is_taken(swapped):
    _taken(_gemma_model("gemma3", swapped=swapped), "gemma", "eps", 3)


def test_after_the_other_entries_it_takes_the_same_norms():
    """the documented order: fuse_llama_layers / fuse_gemma_layers + fuse_gemma_postnorm_residual first, fuse_qk_norms LAST"""
    import protoquant_amd as pq
    m = _qwen3(swapped=True)
    assert pq.fuse_llama_layers(m, fuse_residual=True) == L
    _taken(m, "llama", "variance_epsilon", L)
    g = _gemma_model("gemma3")
    assert pq.fuse_gemma_layers(g) == 3 and pq.fuse_gemma_postnorm_residual(g) == 3
    _taken(g, "gemma", "eps", 3)


def test_a_hooked_k_norm_stays_while_its_q_norm_is_taken():
    from protoquant_amd import HeadRMSNorm, fuse_qk_norms
    m = _qwen3()
    attns = _attentions(m)
    hooked, pre_hooked = attns[0].k_norm, attns[1].q_norm
    h1 = hooked.register_forward_hook(lambda mod, a, o: None)
    h2 = pre_hooked.register_forward_pre_hook(lambda mod, a: None)
    assert fuse_qk_norms(m) == 2 * L - 2
    assert attns[0].k_norm is hooked and isinstance(attns[0].q_norm, HeadRMSNorm) and attns[1].q_norm is pre_hooked and isinstance(attns[1].k_norm, HeadRMSNorm)
    h1.remove(); h2.remove()
    assert fuse_qk_norms(m) == 2 and isinstance(attns[0].k_norm, HeadRMSNorm) and isinstance(attns[1].q_norm, HeadRMSNorm)


def test_a_wrong_width_or_a_missing_head_dim_is_left_alone():
    from protoquant_amd import fuse_qk_norms
    Qwen3RMSNorm = _stock("transformers.models.qwen3.modeling_qwen3", "Qwen3RMSNorm")
    m = _qwen3()
    attns = _attentions(m)
    attns[0].q_norm = wide = Qwen3RMSNorm(64, eps=1e-6)          # not head_dim wide (the whole of q: OLMo's shape)
    attns[1].head_dim = 16.0                                      # not an integer
    assert fuse_qk_norms(m) == 2 * L - 1 - 2 and attns[0].q_norm is wide and type(attns[1].q_norm) is Qwen3RMSNorm and type(attns[1].k_norm) is Qwen3RMSNorm


# ---------------------------------------------------------------------------------------------------------------- the models it leaves alone
@pytest.mark.parametrize("family", ["olmo2", "llama", "cohere", "gemma2"])
def test_other_models_are_left_alone_object_for_object(family):
    from protoquant_amd import fuse_qk_norms
    if family == "olmo2":
        m = _tiny("Olmo2Config", "Olmo2ForCausalLM")              # q_norm / k_norm are H * D wide: fuse_olmo_layers'
        assert m.model.layers[0].self_attn.q_norm.weight.shape == (64,)
    elif family == "llama":
        m = _tiny("LlamaConfig", "LlamaForCausalLM")              # no such children
    elif family == "cohere":
        m = _tiny("CohereConfig", "CohereForCausalLM", use_qk_norm=True)          # a mean-subtracting LayerNorm with a 2-D weight
        assert m.model.layers[0].self_attn.q_norm.weight.dim() == 2
    else:
        m = _gemma_model("gemma2", swapped=False)
    before = dict(m.named_modules())
    keys = list(m.state_dict())
    assert fuse_qk_norms(m) == 0
    after = dict(m.named_modules())
    assert list(after) == list(before) and all(after[n] is before[n] for n in before) and list(m.state_dict()) == keys


def test_olmo_norms_already_fused_are_left_alone():
    from protoquant_amd import OlmoRMSNorm, fuse_qk_norms
    m = _qwen3()
    a = _attentions(m)[0]
    a.q_norm = o = OlmoRMSNorm(a.q_norm.weight, 1e-6)            # head_dim wide, but already a library norm
    assert fuse_qk_norms(m) == 2 * L - 1 and a.q_norm is o


# ---------------------------------------------------------------------------------------------------------------- the order requirement
def test_called_first_it_makes_the_later_entries_refuse_and_the_model_stays_valid():
    """fuse_qk_norms is documented as the LAST call.  Called first, fuse_gemma_layers' CPU probe of how a norm's output is used runs the real attention forward, the
    HeadRMSNorm in it raises on the CPU tensor, and the entry refuses those norms: every module afterwards is either the object it was or a valid fused module —
    nothing is half converted — and the later fuse_gemma_postnorm_residual finds no layer it can take."""
    import protoquant_amd as pq
    from protoquant_amd.llama import _FusedSlice
    right = _gemma_model("gemma3")
    assert pq.fuse_gemma_layers(right) == 3 and pq.fuse_gemma_postnorm_residual(right) == 3 and pq.fuse_qk_norms(right) == 6
    m = _gemma_model("gemma3")
    before = dict(m.named_modules())
    assert pq.fuse_qk_norms(m) == 6
    heads = {n: mod for n, mod in m.named_modules() if isinstance(mod, pq.HeadRMSNorm)}
    pq.fuse_gemma_layers(m)                                       # must not raise
    assert pq.fuse_gemma_postnorm_residual(m) == 0
    valid = (pq.GemmaRMSNormQuant, pq.GatedMLP, pq.FusedQLinear, pq.qlinear, pq.HeadRMSNorm, _FusedSlice)
    for n, mod in m.named_modules():
        assert (n in before and mod is before[n]) or isinstance(mod, valid) or n.endswith(("qkv_fused", "qkv_fused.fused")), (n, type(mod).__name__)
    assert {n: mod for n, mod in m.named_modules() if isinstance(mod, pq.HeadRMSNorm)} == heads          # the q / k norms stay what fuse_qk_norms made them
    for layer in m.model.layers:                                  # the norms whose use could not be probed stay the model's eager modules
        assert type(layer.input_layernorm).__name__ == "Gemma3RMSNorm" and not isinstance(layer, pq.SandwichFusedLayer)
    assert sum(isinstance(l, pq.SandwichFusedLayer) for l in right.model.layers) == 3
