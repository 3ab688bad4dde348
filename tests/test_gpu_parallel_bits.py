"""-m gpu: fuse_parallel_residual(model) — the three-way sum of a parallel-residual block (GPT-NeoX with use_parallel_residual, Phi) inside the LayerNorm +
quantisation kernel of the next block (K1pl), and the two norms of the first GPT-NeoX block in one launch (K1l2).  The sum is two binary32 adds with two storage
roundings in the block's own association either way (QSPEC A2) and the norms are K1l's, so the parallel-fused model is held bit for bit to the SAME model fused
without it and to the specification twin (built here as in tests/test_gpu_gptlike_residual.py): logits, every hidden state, greedy generation with the KV cache, in
bf16 and fp16, at a hidden size that is a multiple of 128 and one that is not.  Plus the launch counts per forward, the hand-over discipline (nothing pending after a
forward — one that raised included — a block called alone, a refused block in the middle of the stack) and the fallbacks to the original forward.  There is no
tolerance anywhere in this file."""
import copy

import numpy as np
import pytest
import torch
from torch import nn

from tests import act_spec as AS
from tests import gptlike_models as G
from tests import lnorm_spec as LS

pytestmark = pytest.mark.gpu

CODE = {torch.bfloat16: 0, torch.float16: 1}
FAMILIES = ["gpt_neox", "phi"]


@pytest.fixture(scope="module")
def pq():
    import protoquant_amd
    from protoquant_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available()
    return protoquant_amd


def _store(t):
    return t.detach().contiguous().cpu().view(torch.int16).numpy().view(np.uint16).copy()


def _load(a, like):
    return torch.from_numpy(a.view(np.int16)).view(like.dtype).reshape(like.shape).to(like.device)


class SpecLayerNorm(nn.Module):
    def __init__(self, ln):
        super().__init__()
        self.weight, self.bias, self.eps = ln.weight, ln.bias, ln.eps

    def forward(self, x):
        h, _, _ = LS.layernorm(_store(x.reshape(-1, x.shape[-1])), _store(self.weight), None if self.bias is None else _store(self.bias), self.eps, CODE[x.dtype])
        return _load(h, x)


class SpecAct(nn.Module):
    def __init__(self, kind):
        super().__init__()
        self.kind = kind

    def forward(self, x):
        return _load(AS.act(_store(x.reshape(-1, x.shape[-1])), CODE[x.dtype], self.kind), x)


def _blocks(model):
    from protoquant_amd.gptlike import ParallelFusedBlock
    return [b for b in model.modules() if isinstance(b, ParallelFusedBlock)]


def _pending(model):
    return [i for i, b in enumerate(_blocks(model)) if b._rf_inbox.pending]


def _stack(model):
    """the ModuleList of decoder blocks (the only ModuleList of these models)"""
    stacks = [m for m in model.modules() if isinstance(m, nn.ModuleList)]
    assert len(stacks) == 1
    return stacks[0]


_CACHE = {}


def _models(pq, family, dtype=torch.bfloat16, hidden=128, layers=3, twin=False, **kw):
    """(the unquantised model, fused without the parallel fusion, fused with it[, the specification twin]): the same weights.  Built once per configuration and
    shared by the tests, which leave them as they found them."""
    key = (family, dtype, hidden, layers, twin, tuple(sorted(kw.items())))
    if key in _CACHE:
        return _CACHE[key]
    base = G.build(family, hidden=hidden, layers=layers, **kw).to(dtype).cuda()
    with torch.no_grad():
        for m in base.modules():
            if isinstance(m, nn.LayerNorm):
                m.weight.copy_((1 + 0.2 * torch.randn(m.weight.shape)).to(dtype))
                m.bias.copy_((0.2 * torch.randn(m.bias.shape)).to(dtype))
    swapped = pq.swap_linears(copy.deepcopy(base))
    plain, fused = copy.deepcopy(swapped), copy.deepcopy(swapped)
    assert pq.fuse_layernorm_layers(plain) == pq.fuse_layernorm_layers(fused) == layers
    assert pq.fuse_parallel_residual(fused) == layers and pq.parallel_fused_blocks(fused) == layers and pq.parallel_fused_blocks(plain) == 0
    assert list(plain.state_dict()) == list(fused.state_dict())
    out = (base, plain, fused)
    if twin:
        tw = copy.deepcopy(swapped)
        fm, tm = dict(plain.named_modules()), dict(tw.named_modules())
        for name, m in fm.items():
            if isinstance(m, (pq.LayerNormQuant, pq.ActQuant)):
                parent, attr = name.rsplit(".", 1)
                setattr(tm[parent], attr, SpecLayerNorm(m) if isinstance(m, pq.LayerNormQuant) else SpecAct(m.kind))
        out += (tw,)
    _CACHE[key] = out
    return out


def _same_outputs(a, b, ids, nhidden):
    with torch.no_grad():
        oa = a(input_ids=ids, output_hidden_states=True, use_cache=False)
        ob = b(input_ids=ids, output_hidden_states=True, use_cache=False)
    assert torch.equal(oa.logits, ob.logits), f"logits differ in {int((oa.logits != ob.logits).sum())} places"
    assert len(oa.hidden_states) == len(ob.hidden_states) == nhidden
    for i, (x, y) in enumerate(zip(oa.hidden_states, ob.hidden_states)):
        assert torch.equal(x, y), f"hidden state {i} differs"
    return oa.logits


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("hidden", [128, 96])
def test_parallel_fused_models_equal_the_fused_model_and_the_spec_twin(pq, family, dtype, hidden):
    base, plain, fused, twin = _models(pq, family, dtype, hidden, twin=True)
    g = torch.Generator().manual_seed(hidden)
    ids = torch.randint(3, 128, (2, 11), generator=g).cuda()
    lf = _same_outputs(fused, plain, ids, 4)
    _same_outputs(fused, twin, ids, 4)
    assert _pending(fused) == []
    with torch.no_grad():                       # decode shapes: one token per step against the KV cache
        gf = fused.generate(ids[:1, :5], max_new_tokens=6, do_sample=False, use_cache=True, pad_token_id=0)
        gp = plain.generate(ids[:1, :5], max_new_tokens=6, do_sample=False, use_cache=True, pad_token_id=0)
        gt = twin.generate(ids[:1, :5], max_new_tokens=6, do_sample=False, use_cache=True, pad_token_id=0)
        lb = base(input_ids=ids, use_cache=False).logits
        lp = plain(input_ids=ids, use_cache=False).logits
    assert gf.shape == (1, 11) and torch.equal(gf, gp) and torch.equal(gf, gt)
    assert _pending(fused) == []
    # the cosine of all logits to the unquantised model is what it was: printed for the record (README), a criterion only through equality with the un-switched model
    cos = lambda a, b: float(torch.nn.functional.cosine_similarity(a.double().flatten(), b.double().flatten(), dim=0))          # noqa: E731
    print(f"cosine to the unquantised model, {family} {dtype} hidden {hidden}: fused {cos(lf, lb):.6f}, without the parallel fusion {cos(lp, lb):.6f}")
    assert cos(lf, lb) == cos(lp, lb)


NAMES = ("pq_qlinear_dyn", "pq_qlinear_s8", "pq_layernorm_quant_rowwise", "pq_add_layernorm_quant_rowwise", "pq_parallel_layernorm_quant_rowwise", "pq_act_quant_rowwise",
         "pq_quant_rowwise", "pq_gemm_s8s8s32")


def _count(pq, model, ids):
    """one forward: calls of the library's entry points (the new one split into K1pl — a is given — and K1l2), and calls of the LayerNormQuant modules"""
    from protoquant_amd import _lib
    L = _lib.lib()
    calls = dict.fromkeys(NAMES + ("K1pl", "K1l2"), 0)
    norms = [0]
    orig = {n: getattr(L, n) for n in NAMES}

    def wrap(n):
        def f(*a):
            calls[n] += 1
            if n == "pq_parallel_layernorm_quant_rowwise":
                calls["K1pl" if a[0] else "K1l2"] += 1
            return orig[n](*a)
        return f

    def hook(mod, args, out):
        norms[0] += 1
    hs = [m.register_forward_hook(hook) for m in model.modules() if isinstance(m, pq.LayerNormQuant)]
    try:
        for n in NAMES:
            setattr(L, n, wrap(n))
        with torch.no_grad():
            logits = model(input_ids=ids, use_cache=False).logits
    finally:
        for n in NAMES:
            setattr(L, n, orig[n])
        for h in hs:
            h.remove()
    return calls, norms[0], logits


@pytest.mark.parametrize("family", FAMILIES)
def test_launch_counts_per_forward(pq, family):
    """GPT-NeoX: L - 1 K1pl, one K1l2 and no K1l; Phi: L - 1 K1pl and one K1l.  The GEMM and activation calls are those of the model fused without it."""
    layers = 4
    _, plain, fused = _models(pq, family, layers=layers)
    ids = torch.randint(3, 128, (1, 9)).cuda()
    per_block = 2 if family == "gpt_neox" else 1
    cp, np_, lp = _count(pq, plain, ids)
    cf, nf, lf = _count(pq, fused, ids)
    assert torch.equal(lp, lf)
    assert np_ == per_block * layers and cp["pq_layernorm_quant_rowwise"] == per_block * layers and cp["pq_parallel_layernorm_quant_rowwise"] == 0
    assert nf == 0                                            # the norm modules are read for their parameters and no longer called
    assert cf["K1pl"] == layers - 1 and cf["K1l2"] == (1 if family == "gpt_neox" else 0) and cf["pq_layernorm_quant_rowwise"] == (0 if family == "gpt_neox" else 1), cf
    assert cf["pq_add_layernorm_quant_rowwise"] == 0
    for n in ("pq_qlinear_dyn", "pq_qlinear_s8", "pq_act_quant_rowwise", "pq_quant_rowwise", "pq_gemm_s8s8s32"):
        assert cf[n] == cp[n], (n, cp, cf)
    assert cf["pq_act_quant_rowwise"] == layers
    # the model's input tensor is never written: the embedding output feeds block 0 and stays what it was
    emb = fused.get_input_embeddings()(ids)
    keep = emb.clone()
    with torch.no_grad():
        fused(inputs_embeds=emb, use_cache=False)
    assert torch.equal(emb, keep) and _pending(fused) == []


def _block_kwargs(model, family, x):
    """what the model hands its blocks besides the hidden states, for a block called alone"""
    pos = torch.arange(x.shape[1], device="cuda")[None]
    inner = model.gpt_neox if family == "gpt_neox" else model.model
    return {"position_embeddings": inner.rotary_emb(x, position_ids=pos)}


@pytest.mark.parametrize("family", FAMILIES)
def test_a_block_called_alone_gives_the_unfused_blocks_bits(pq, family):
    _, plain, fused = _models(pq, family)
    sp, sf = _stack(plain), _stack(fused)
    x = torch.randn(2, 8, 128, device="cuda").to(torch.bfloat16)
    keep = x.clone()
    kw = _block_kwargs(plain, family, x)
    with torch.no_grad():
        for i in (0, 1, 2):                                   # a link of the chain, and its end (two torch adds)
            assert torch.equal(sp[i](x, **kw), sf[i](x, **kw)), i
        assert _pending(fused) == []                          # each hand-over was parked for a tensor its successor was not called with: not served, and gone
        y = sf[0](x, **kw)
        assert _pending(fused) == [1]
        assert torch.equal(sf[1](x, **kw), sp[1](x, **kw))    # a hand-over parked for ANOTHER tensor is not served
        y = sf[0](x, **kw)
        y.mul_(1.25)                                          # ... nor for the same tensor changed in place since
        assert torch.equal(sf[1](y, **kw), sp[1](y, **kw))
        y = sf[0](x, **kw)
        assert torch.equal(sf[1](y, **kw), sp[1](sp[0](x, **kw), **kw))          # served: the same bits
        sf[2]._rf_inbox.clear()
    assert torch.equal(x, keep) and _pending(fused) == []     # the tensor a block is called with is never written


def test_nothing_is_pending_after_a_forward_that_raised_or_in_a_deep_copy(pq):
    _, plain, fused = _models(pq, "gpt_neox")
    ids = torch.randint(3, 128, (1, 12)).cuda()

    class Boom(RuntimeError):
        pass

    def boom(mod, args, kwargs):
        raise Boom()
    st = _stack(fused)
    for target in (st[2].mlp, st[1].attention):
        h = target.register_forward_pre_hook(boom, with_kwargs=True)
        with torch.no_grad(), pytest.raises(Boom):
            fused(input_ids=ids, use_cache=False)
        h.remove()
        assert _pending(fused) == []
    x = torch.randn(1, 8, 128, device="cuda").to(torch.bfloat16)
    with torch.no_grad():
        st[0](x, **_block_kwargs(fused, "gpt_neox", x))
    assert _pending(fused) == [1]
    c = copy.deepcopy(fused)
    sc = _stack(c)
    assert _pending(c) == [] and _pending(fused) == [1]
    assert sc[0]._rf_next[0] is sc[1] and sc[0] is not st[0] and c.gpt_neox._rf_layers[0] is sc[0]
    with torch.no_grad():
        want = plain(input_ids=ids, use_cache=False).logits
        assert torch.equal(fused(input_ids=ids, use_cache=False).logits, want) and torch.equal(c(input_ids=ids, use_cache=False).logits, want)
    assert _pending(fused) == [] and _pending(c) == []


@pytest.mark.parametrize("family", FAMILIES)
def test_a_hooked_block_in_the_middle_breaks_the_chain_and_the_model_still_matches(pq, family):
    """a norm of block 1 of 4 carries a forward hook: the block keeps the norm / activation fusions and is not parallel-fused (its hook keeps firing), and its
    predecessor ends with the two torch adds"""
    from protoquant_amd.gptlike import ParallelFusedBlock
    base = pq.swap_linears(G.build(family, hidden=128, layers=4).to(torch.bfloat16).cuda())
    plain, fused = base, copy.deepcopy(base)
    assert pq.fuse_layernorm_layers(plain) == 4 and pq.fuse_layernorm_layers(fused) == 4
    fired = [0]
    _stack(fused)[1].input_layernorm.register_forward_hook(lambda mod, args, out: fired.__setitem__(0, fired[0] + 1))
    assert pq.fuse_parallel_residual(fused) == 3 and pq.parallel_fused_blocks(fused) == 3
    st = _stack(fused)
    assert [isinstance(b, ParallelFusedBlock) for b in st] == [True, False, True, True]
    assert type(st[1]) is type(_stack(plain)[1]) and isinstance(st[1].input_layernorm, pq.LayerNormQuant)
    assert st[0]._rf_next[0] is None and st[2]._rf_next[0] is st[3] and st[3]._rf_next[0] is None
    ids = torch.randint(3, 128, (2, 17)).cuda()
    _same_outputs(fused, plain, ids, 5)
    assert _pending(fused) == [] and fired[0] == 1
    # a second call finds nothing left to change (no block is converted or hooked twice)
    owner = fused.gpt_neox if family == "gpt_neox" else fused.model
    assert pq.fuse_layernorm_layers(fused) == 0 and pq.fuse_parallel_residual(fused) == 0 and pq.parallel_fused_blocks(fused) == 3 and len(owner._rf_layers) == 3


def test_fallbacks_behave_exactly_like_the_unfused_model(pq):
    # a positional argument too many: the TypeError of the original forward
    _, plain, fused = _models(pq, "phi")
    x = torch.randn(1, 6, 128, device="cuda").to(torch.bfloat16)
    for m in (plain, fused):
        with pytest.raises(TypeError):
            _stack(m)[0](x, None, None, None, False, None, "one too many")
    # training mode with a non-zero dropout on the stream: the original forward, the same random stream
    for family, kw, names in (("gpt_neox", dict(hidden_dropout=0.25), {"post_attention_dropout", "post_mlp_dropout"}), ("phi", dict(resid_pdrop=0.25), {"resid_dropout"})):
        _, plain, fused = _models(pq, family, layers=2, **kw)
        assert len(_blocks(fused)) == 2 and set(_blocks(fused)[0]._pfb_plan.stateless) == names
        ids = torch.randint(3, 128, (2, 9)).cuda()
        outs = []
        for m in (plain, fused):
            m.train()
            torch.manual_seed(11)
            with torch.no_grad():
                outs.append(m(input_ids=ids, use_cache=False).logits)
            m.eval()
        assert torch.equal(outs[0], outs[1]) and _pending(fused) == []
        with torch.no_grad():
            le = fused(input_ids=ids, use_cache=False).logits
            assert torch.equal(le, plain(input_ids=ids, use_cache=False).logits) and not torch.equal(le, outs[1])          # (the dropout did drop)


def test_a_withheld_argument_runs_the_original_forward(pq):
    """a block class whose forward has a parameter the attention never sees: a call that sets it takes the original forward (and its branch), any other call the fused one"""
    from protoquant_amd.gptlike import ParallelFusedBlock
    base = pq.swap_linears(G.build("gpt_neox", hidden=128, layers=2).to(torch.bfloat16).cuda())
    cls = type(base.gpt_neox.layers[0])

    class WithSwitch(cls):
        def forward(self, hidden_states, attention_mask=None, position_ids=None, use_cache=False, layer_past=None, position_embeddings=None, double=None, **kwargs):
            out = cls.forward(self, hidden_states, attention_mask=attention_mask, position_ids=position_ids, use_cache=use_cache, layer_past=layer_past,
                              position_embeddings=position_embeddings, **kwargs)
            return out if double is None else out * 2.0
    for b in base.gpt_neox.layers:
        b.__class__ = WithSwitch
    plain, fused = base, copy.deepcopy(base)
    assert pq.fuse_layernorm_layers(plain) == 2 and pq.fuse_layernorm_layers(fused) == 2 and pq.fuse_parallel_residual(fused) == 2
    b0 = _stack(fused)[0]
    assert isinstance(b0, ParallelFusedBlock) and isinstance(b0, WithSwitch) and b0._pfb_plan.withheld == ("double",)
    x = torch.randn(1, 6, 128, device="cuda").to(torch.bfloat16)
    kw = _block_kwargs(plain, "gpt_neox", x)
    with torch.no_grad():
        assert torch.equal(b0(x, double=True, **kw), _stack(plain)[0](x, double=True, **kw)) and _pending(fused) == []          # the original forward: nothing handed over
        assert torch.equal(b0(x, **kw), _stack(plain)[0](x, **kw)) and _pending(fused) == [1]
        ids = torch.randint(3, 128, (1, 7)).cuda()
        assert torch.equal(plain(input_ids=ids, use_cache=False).logits, fused(input_ids=ids, use_cache=False).logits) and _pending(fused) == []
