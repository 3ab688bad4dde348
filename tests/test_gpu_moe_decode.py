"""-m gpu: mixture-of-experts layers at DECODE sizes.  A forward with at most GroupedQLinear.stream_rows grouped rows takes the weight-streaming grouped kernel
(gemm_s8_grouped_stream.hip) for both GEMMs; it must equal, bit for bit, the same module on the 64-row tiles (stream_rows = 0) and the eager per-expert loop; and a
swapped decoder must decode the same logits either way."""
import copy

import pytest
import torch

from tests import moe_models as M
from tests.test_gpu_moe import _eager_loop, _expert_linears, _routing, _same

pytestmark = pytest.mark.gpu


def _set_stream_rows(module, rows):
    import protoquant_amd as pq
    n = 0
    for m in module.modules():
        if isinstance(m, pq.GroupedQLinear):
            m.stream_rows = rows
            n += 1
    assert n > 0
    return n


def _entries(monkeypatch):
    """which grouped entry point GroupedQLinear.forward calls: a list of (name, grouped rows)"""
    from protoquant_amd import moe
    seen = []
    for name in ("qlinear_s8_grouped", "qlinear_s8_grouped_stream"):
        real = getattr(moe, name)

        def spy(*a, _real=real, _name=name, **k):
            y = _real(*a, **k)
            seen.append((_name, y.shape[0]))
            return y
        monkeypatch.setattr(moe, name, spy)
    return seen


@pytest.mark.parametrize("E,k", ((8, 2), (128, 8)))
@pytest.mark.parametrize("T", (1, 2, 7, 32))
def test_decode_forward_equals_the_tile_path_and_the_eager_loop(monkeypatch, T, E, k):
    import protoquant_amd as pq
    H, I = 256, 384
    lins = _expert_linears(E, H, I, 3)
    mlps = [pq.GatedMLP.from_linears(*l) for l in lins]
    moe = pq.MoEGatedMLP.from_experts(mlps)
    x = (torch.randn(T, H, device="cuda", generator=torch.Generator(device="cuda").manual_seed(T)) * 1.5).to(torch.bfloat16)
    ids, w = _routing(T, E, k, "skewed" if T == 7 else "balanced", 5 * T + k)
    seen = _entries(monkeypatch)
    _set_stream_rows(moe, 64)
    fast = moe(x, ids, w)
    took = [n for n, _ in seen]
    assert took == (["qlinear_s8_grouped_stream"] * 2 if T * k <= 64 else ["qlinear_s8_grouped"] * 2), (T, k, seen)
    assert all(rows == T * k for _, rows in seen)
    del seen[:]
    _set_stream_rows(moe, 0)
    tiles = moe(x, ids, w)
    assert [n for n, _ in seen] == ["qlinear_s8_grouped"] * 2
    _same(fast, tiles, f"T {T} E {E} k {k}: stream_rows 64 against 0")
    _same(fast, _eager_loop(mlps, x, ids, w), f"T {T} E {E} k {k}: against the eager per-expert loop")


def test_the_threshold_is_honoured_at_the_edge(monkeypatch):
    """T x k = 65 grouped rows: the tile path; 64: the streaming path; a smaller per-instance threshold moves the edge"""
    import protoquant_amd as pq
    E, H, I = 16, 128, 128
    mlps = [pq.GatedMLP.from_linears(*l) for l in _expert_linears(E, H, I, 8)]
    moe = pq.MoEGatedMLP.from_experts(mlps)
    seen = _entries(monkeypatch)
    for T, k, rows, want in ((13, 5, 64, "qlinear_s8_grouped"), (64, 1, 64, "qlinear_s8_grouped_stream"), (8, 8, 64, "qlinear_s8_grouped_stream"),
                             (8, 2, 16, "qlinear_s8_grouped_stream"), (17, 1, 16, "qlinear_s8_grouped"), (1, 1, 0, "qlinear_s8_grouped")):
        _set_stream_rows(moe, rows)
        x = torch.randn(T, H, device="cuda").to(torch.bfloat16)
        ids, w = _routing(T, E, k, "balanced", T)
        del seen[:]
        got = moe(x, ids, w)
        assert [n for n, _ in seen] == [want] * 2, (T, k, rows, seen)
        _same(got, _eager_loop(mlps, x, ids, w), f"T {T} k {k} stream_rows {rows}")
    assert f"stream_rows={moe.down.stream_rows}" in repr(moe.down)


@pytest.mark.parametrize("family", ("mixtral", "qwen3_moe"))
def test_a_swapped_decoder_decodes_the_same_logits_on_both_paths(monkeypatch, family):
    """8 greedy tokens with the KV cache: every cached step sends 2 x k grouped rows through both GEMMs of every sparse layer"""
    import protoquant_amd as pq
    model = M.build(family, seed=0, H=256, I=128, E=8, k=2, layers=2)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for _, blk in M.sparse_blocks(model):
            blk.experts.gate_up_proj.normal_(0, 0.05, generator=g); blk.experts.down_proj.normal_(0, 0.05, generator=g)
            (blk.gate if hasattr(blk, "gate") else blk.router).weight.normal_(0, 0.3, generator=g)
    model = model.to(torch.bfloat16).cuda().eval()
    assert pq.swap_moe_experts(model) == 2
    ids = torch.randint(3, M.VOCAB, (2, 12), generator=torch.Generator().manual_seed(5)).cuda()
    seen = _entries(monkeypatch)
    outs = []
    for rows in (64, 0):
        _set_stream_rows(model, rows)
        del seen[:]
        with torch.no_grad():
            outs.append(model.generate(ids, max_new_tokens=8, min_new_tokens=8, do_sample=False, use_cache=True, output_logits=True, return_dict_in_generate=True,
                                       pad_token_id=0, eos_token_id=None))
        names = {n for n, r in seen if r == 4}                  # the cached steps: 2 sequences x top-2
        assert names == ({"qlinear_s8_grouped_stream"} if rows else {"qlinear_s8_grouped"}), (rows, seen)
        assert sum(1 for n, r in seen if r == 4) == 7 * 2 * 2  # 7 cached steps x 2 layers x 2 GEMMs
    assert torch.equal(outs[0].sequences, outs[1].sequences) and outs[0].sequences.shape == (2, 20)
    for step in range(8):
        assert torch.equal(outs[0].logits[step], outs[1].logits[step]), f"{family}: the logits of step {step} differ between stream_rows 64 and 0"
