"""-m gpu: RotatedQLinear / rotate_linears (protoquant_amd/hadamard.py) — the module against the composition written out with the library's own pieces, its error on the
designed outlier input against qlinear's, the state-dict round trip, and rotate_linears -> swap_linears -> fuse_llama_layers on a tiny Llama."""
import pytest
import torch

from tests import llama_twin as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pq():
    import protoquant_amd
    assert torch.cuda.is_available()
    return protoquant_amd


def _outlier_input(M, K, dtype):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(M, K, generator=g)
    x[:, 5] *= 50
    x[:, K // 2 + 3] *= 25
    return x.to(dtype).cuda()


def _linear(K, N, dtype, bias):
    torch.manual_seed(K + N)
    return torch.nn.Linear(K, N, bias=bias, dtype=dtype).cuda()


@pytest.mark.parametrize("dtype,K,N,bias", [(torch.bfloat16, 256, 64, True), (torch.bfloat16, 256, 64, False), (torch.bfloat16, 320, 64, True), (torch.bfloat16, 320, 64, False),
                                            (torch.float16, 256, 64, True)])
def test_module_is_the_composition_and_beats_qlinear_on_outliers(pq, dtype, K, N, bias):
    lin = _linear(K, N, dtype, bias)
    x = _outlier_input(32, K, dtype)
    rot = pq.RotatedQLinear.from_linear(lin)
    block = rot.block
    assert block == min(4096, K & -K) and int(rot.rot_block) == block
    y = rot(x)
    wq = pq.quantize(pq.hadamard(lin.weight.detach().float(), block).to(dtype))
    xq = pq.hadamard_quantize(x, block)
    kp = -(-K // 128) * 128          # K = 320 runs the zero-padded GEMM: the same accumulators
    pad = lambda t: torch.nn.functional.pad(t, (0, kp - K))          # noqa: E731
    want = pq.qlinear_s8(pad(xq.int_data), xq.scale, pad(wq.int_data), wq.scale, lin.bias.detach() if bias else None, dtype)
    assert torch.equal(rot.wq, wq.int_data) and torch.equal(rot.ws, wq.scale) and torch.equal(y.view(torch.int16), want.view(torch.int16))
    exact = x.double() @ lin.weight.detach().double().t() + (lin.bias.detach().double() if bias else 0)
    err = lambda t: float((t.double() - exact).norm() / exact.norm())          # noqa: E731
    plain = err(pq.qlinear.from_linear(lin)(x))
    print(f"K={K} block={block} {dtype}: plain {plain:.4f} rotated {err(y):.4f}")
    assert err(y) < plain
    # state_dict -> a fresh module -> the same bits
    fresh = pq.RotatedQLinear(K, N, bias=bias, device="cuda", dtype=dtype, block=16)
    fresh.load_state_dict(rot.state_dict())
    assert fresh.block == block and torch.equal(fresh(x).view(torch.int16), y.view(torch.int16))
    with pytest.raises(TypeError, match="QTensor"):
        rot(pq.quantize(x))


def test_rotate_linears_then_swap_and_fuse_on_a_tiny_llama(pq):
    built = T.build("llama", torch.bfloat16, "aligned")
    model, layers = built.model, T.decoder_layers(built.model)
    downs = [l.mlp.down_proj for l in layers]
    others = [l.mlp.gate_proj for l in layers]
    assert pq.rotate_linears(model, lambda name, mod: name == "down_proj") == len(layers)
    assert all(isinstance(l.mlp.down_proj, pq.RotatedQLinear) and l.mlp.down_proj.block == 128 for l in layers)          # 640 = 5 x 128
    assert all(l.mlp.gate_proj is g for l, g in zip(layers, others)) and not any(l.mlp.down_proj is d for l, d in zip(layers, downs))
    rotated = [l.mlp.down_proj for l in layers]
    assert pq.rotate_linears(model, lambda name, mod: name == "down_proj") == 0          # a qlinear is never touched
    pq.swap_linears(model)
    assert pq.fuse_llama_layers(model) == len(layers)
    assert all(l.mlp.down_proj is r for l, r in zip(layers, rotated))
    assert all(type(l.mlp.gate_proj) is pq.qlinear and isinstance(l.post_attention_layernorm, pq.RMSNormQuant) for l in layers)
    ids = torch.arange(24, device="cuda").reshape(2, 12) % T.VOCAB
    with torch.no_grad():
        logits = model(ids).logits
    assert logits.shape == (2, 12, T.VOCAB) and bool(torch.isfinite(logits.float()).all())
