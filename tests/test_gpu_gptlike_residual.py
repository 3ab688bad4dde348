"""-m gpu: fuse_layernorm_residual(model) — the two residual adds of a sequential pre-norm block inside the LayerNorm + quantisation kernels that follow them
(K1al).  The add is one binary32 add and one storage rounding either way (QSPEC A1), so the residual-fused model is held bit for bit to the SAME model fused without
it, and to the specification twin of tests/test_gpu_gptlike_bits.py (built here): logits, every hidden state, greedy generation with the KV cache, in bf16 and fp16,
at a hidden size that is a multiple of 128 and one that is not.  Plus the hand-over discipline (2L - 1 fused add-norms and one plain norm per forward, the same GEMM
and activation calls, nothing pending after a forward — one that raised included — or in a deep copy, a block called alone, a refused block in the middle of the stack),
the fallbacks to the original forward, and the refused families.  There is no tolerance anywhere in this file."""
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
    from protoquant_amd.gptlike import ResidualFusedBlock
    return [b for b in model.modules() if isinstance(b, ResidualFusedBlock)]


def _pending(model):
    return [i for i, b in enumerate(_blocks(model)) if b._rf_inbox.pending]


def _stack(model):
    """the ModuleList of decoder blocks (the only ModuleList of these models)"""
    stacks = [m for m in model.modules() if isinstance(m, nn.ModuleList)]
    assert len(stacks) == 1
    return stacks[0]


def _fuse(pq, model, with_llama, residual):
    if with_llama == "first":
        pq.fuse_llama_layers(model, fuse_residual=residual)
    n = pq.fuse_layernorm_layers(model)
    if residual:
        pq.fuse_layernorm_residual(model)
    if with_llama == "after":
        pq.fuse_llama_layers(model, fuse_residual=residual)
    return n


def _models(pq, family, dtype=torch.bfloat16, hidden=128, with_llama=None, layers=2, twin=False, **kw):
    """(the unquantised model, fused without the residual fusion, fused with it[, the specification twin]): the same weights"""
    base = G.build(family, hidden=hidden, layers=layers, **kw).to(dtype).cuda()
    with torch.no_grad():
        for m in base.modules():
            if isinstance(m, nn.LayerNorm):
                m.weight.copy_((1 + 0.2 * torch.randn(m.weight.shape)).to(dtype))
                m.bias.copy_((0.2 * torch.randn(m.bias.shape)).to(dtype))
    swapped = pq.swap_linears(copy.deepcopy(base))
    plain, fused = copy.deepcopy(swapped), copy.deepcopy(swapped)
    assert _fuse(pq, plain, with_llama, False) == _fuse(pq, fused, with_llama, True) == layers
    assert list(plain.state_dict()) == list(fused.state_dict())
    if not twin:
        return base, plain, fused
    tw = copy.deepcopy(swapped)
    fm, tm = dict(plain.named_modules()), dict(tw.named_modules())
    for name, m in fm.items():
        if isinstance(m, (pq.LayerNormQuant, pq.ActQuant)):
            parent, attr = name.rsplit(".", 1)
            setattr(tm[parent], attr, SpecLayerNorm(m) if isinstance(m, pq.LayerNormQuant) else SpecAct(m.kind))
    return base, plain, fused, tw


def _same_outputs(a, b, ids, nhidden):
    with torch.no_grad():
        oa = a(input_ids=ids, output_hidden_states=True, use_cache=False)
        ob = b(input_ids=ids, output_hidden_states=True, use_cache=False)
    assert torch.equal(oa.logits, ob.logits), f"logits differ in {int((oa.logits != ob.logits).sum())} places"
    assert len(oa.hidden_states) == len(ob.hidden_states) == nhidden
    for i, (x, y) in enumerate(zip(oa.hidden_states, ob.hidden_states)):
        assert torch.equal(x, y), f"hidden state {i} differs"


CASES = [("gpt2", None), ("starcoder2", None), ("starcoder2", "first"), ("starcoder2", "after"), ("gpt_neox_seq", None)]


@pytest.mark.parametrize("family,with_llama", CASES, ids=[f"{a}-{b}" for a, b in CASES])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("hidden", [128, 96])
def test_residual_fused_models_equal_the_fused_model_and_the_spec_twin(pq, family, with_llama, dtype, hidden):
    from protoquant_amd.gptlike import residual_fused_blocks
    from protoquant_amd.llama import residual_fused_layers
    _, plain, fused, twin = _models(pq, family, dtype, hidden, with_llama, layers=3, twin=True)
    assert residual_fused_blocks(plain) == 0 and residual_fused_blocks(fused) == 3 and residual_fused_layers(fused) == 3
    g = torch.Generator().manual_seed(hidden)
    ids = torch.randint(3, 128, (2, 11), generator=g).cuda()
    _same_outputs(fused, plain, ids, 4)
    _same_outputs(fused, twin, ids, 4)
    assert _pending(fused) == []
    with torch.no_grad():                       # decode shapes: one token per step against the KV cache
        gf = fused.generate(ids[:1, :5], max_new_tokens=6, do_sample=False, use_cache=True, pad_token_id=0)
        gp = plain.generate(ids[:1, :5], max_new_tokens=6, do_sample=False, use_cache=True, pad_token_id=0)
        gt = twin.generate(ids[:1, :5], max_new_tokens=6, do_sample=False, use_cache=True, pad_token_id=0)
    assert gf.shape == (1, 11) and torch.equal(gf, gp) and torch.equal(gf, gt)
    assert _pending(fused) == []


NAMES = ("pq_qlinear_dyn", "pq_qlinear_s8", "pq_layernorm_quant_rowwise", "pq_add_layernorm_quant_rowwise", "pq_act_quant_rowwise", "pq_quant_rowwise", "pq_gemm_s8s8s32")


def _count(pq, model, ids):
    """one forward: calls of the library's entry points, and calls of the LayerNormQuant modules with / without a residual"""
    from protoquant_amd import _lib
    L = _lib.lib()
    calls = dict.fromkeys(NAMES, 0)
    norms = {"fused": 0, "plain": 0}
    orig = {n: getattr(L, n) for n in NAMES}

    def wrap(n):
        def f(*a):
            calls[n] += 1
            return orig[n](*a)
        return f

    def hook(mod, args, kwargs, out):
        norms["fused" if (kwargs.get("residual") is not None or len(args) > 1) else "plain"] += 1
    hs = [m.register_forward_hook(hook, with_kwargs=True) for m in model.modules() if isinstance(m, pq.LayerNormQuant)]
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
    return calls, norms, logits


@pytest.mark.parametrize("family,with_llama", CASES, ids=[f"{a}-{b}" for a, b in CASES])
def test_the_fused_add_norm_runs_2l_minus_1_times_and_the_plain_norm_once(pq, family, with_llama):
    layers = 4
    _, plain, fused = _models(pq, family, with_llama=with_llama, layers=layers)
    ids = torch.randint(3, 128, (1, 9)).cuda()
    cp, np_, lp = _count(pq, plain, ids)
    cf, nf, lf = _count(pq, fused, ids)
    assert torch.equal(lp, lf)
    assert np_ == {"fused": 0, "plain": 2 * layers} and cp["pq_add_layernorm_quant_rowwise"] == 0 and cp["pq_layernorm_quant_rowwise"] == 2 * layers
    assert nf == {"fused": 2 * layers - 1, "plain": 1}, nf          # without a residual: the first block's first norm, and nothing else
    assert cf["pq_add_layernorm_quant_rowwise"] == 2 * layers - 1 and cf["pq_layernorm_quant_rowwise"] == 1, cf
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
    if family == "gpt2":
        return {}
    pos = torch.arange(x.shape[1], device="cuda")[None]
    inner = model.model if family == "starcoder2" else model.gpt_neox
    return {"position_embeddings": inner.rotary_emb(x, position_ids=pos)}


@pytest.mark.parametrize("family", ["gpt2", "starcoder2", "gpt_neox_seq"])
def test_a_block_called_alone_gives_the_unfused_blocks_bits(pq, family):
    _, plain, fused = _models(pq, family, layers=3)
    sp, sf = _stack(plain), _stack(fused)
    x = torch.randn(2, 8, 128, device="cuda").to(torch.bfloat16)
    keep = x.clone()
    kw = _block_kwargs(plain, family, x)
    with torch.no_grad():
        for i in (0, 1, 2):                                   # a link of the chain, and its end (a torch add)
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
    assert torch.equal(x, keep)                               # the tensor a block is called with is never written


def test_nothing_is_pending_after_a_forward_that_raised_or_in_a_deep_copy(pq):
    _, plain, fused = _models(pq, "gpt2", layers=3)
    ids = torch.randint(3, 128, (1, 12)).cuda()

    class Boom(RuntimeError):
        pass

    def boom(mod, args, kwargs):
        raise Boom()
    st = _stack(fused)
    for target in (st[2].mlp, st[1].attn):
        h = target.register_forward_pre_hook(boom, with_kwargs=True)
        with torch.no_grad(), pytest.raises(Boom):
            fused(input_ids=ids, use_cache=False)
        h.remove()
        assert _pending(fused) == []
    x = torch.randn(1, 8, 128, device="cuda").to(torch.bfloat16)
    with torch.no_grad():
        st[0](x)
    assert _pending(fused) == [1]
    c = copy.deepcopy(fused)
    sc = _stack(c)
    assert _pending(c) == [] and _pending(fused) == [1]
    assert sc[0]._rf_next[0] is sc[1] and sc[0] is not st[0] and c.transformer._rf_layers[0] is sc[0]
    with torch.no_grad():
        want = plain(input_ids=ids, use_cache=False).logits
        assert torch.equal(fused(input_ids=ids, use_cache=False).logits, want) and torch.equal(c(input_ids=ids, use_cache=False).logits, want)
    assert _pending(fused) == [] and _pending(c) == []


def test_a_refused_block_in_the_middle_breaks_the_chain_and_the_model_still_matches(pq):
    """block 1 of 4 gets a forward with a scaled residual: it keeps the norm / activation fusions, is not residual-fused, and its predecessor ends with a torch add"""
    from protoquant_amd.gptlike import ResidualFusedBlock, residual_fused_blocks
    base = G.build("gpt2", hidden=128, layers=4).to(torch.bfloat16).cuda()
    cls = type(base.transformer.h[1])

    class Scaled(cls):
        def forward(self, hidden_states, past_key_values=None, attention_mask=None, encoder_hidden_states=None, encoder_attention_mask=None, use_cache=False, **kwargs):
            a, _ = self.attn(self.ln_1(hidden_states), past_key_values=past_key_values, attention_mask=attention_mask, use_cache=use_cache, **kwargs)
            hidden_states = hidden_states + a * 0.5
            return hidden_states + self.mlp(self.ln_2(hidden_states)) * 0.5
    base.transformer.h[1].__class__ = Scaled
    pq.swap_linears(base)
    plain, fused = base, copy.deepcopy(base)
    assert pq.fuse_layernorm_layers(plain) == 4
    assert pq.fuse_layernorm_layers(fused) == 4 and pq.fuse_layernorm_residual(fused) == 3 and residual_fused_blocks(fused) == 3
    st = fused.transformer.h
    assert [isinstance(b, ResidualFusedBlock) for b in st] == [True, False, True, True]
    assert type(st[1]) is Scaled and isinstance(st[1].ln_1, pq.LayerNormQuant)
    assert st[0]._rf_next[0] is None and st[2]._rf_next[0] is st[3] and st[3]._rf_next[0] is None
    ids = torch.randint(3, 128, (2, 17)).cuda()
    _same_outputs(fused, plain, ids, 5)
    assert _pending(fused) == []
    # a second call finds nothing left to change (no block is converted or hooked twice)
    assert pq.fuse_layernorm_layers(fused) == 0 and pq.fuse_layernorm_residual(fused) == 0 and residual_fused_blocks(fused) == 3 and len(fused.transformer._rf_layers) == 3
    assert len(fused.transformer._forward_hooks) == len(plain.transformer._forward_hooks) + 1


def test_fallbacks_behave_exactly_like_the_unfused_model(pq):
    # GPT-2 called with encoder_hidden_states: the argument the probe withheld — the original forward runs, and raises what it raises (no cross-attention here)
    _, plain, fused = _models(pq, "gpt2", layers=2)
    x = torch.randn(1, 6, 128, device="cuda").to(torch.bfloat16)
    enc = torch.randn(1, 3, 128, device="cuda").to(torch.bfloat16)
    errs = []
    for m in (plain, fused):
        with torch.no_grad(), pytest.raises(Exception) as ei:
            m.transformer.h[0](x, encoder_hidden_states=enc)
        errs.append(type(ei.value))
    assert errs[0] is errs[1] is ValueError
    for m in (plain, fused):
        with pytest.raises(TypeError):
            m.transformer.h[0](x, None, None, None, None, False, "one too many")
    # a GPT-2 WITH cross-attention: the same output
    _, plain, fused = _models(pq, "gpt2", layers=2, add_cross_attention=True)
    assert len(_blocks(fused)) == 2
    with torch.no_grad():
        want = plain.transformer.h[0](x, encoder_hidden_states=enc)
        got = fused.transformer.h[0](x, encoder_hidden_states=enc)
        assert torch.equal(want, got) and _pending(fused) == []
        ids = torch.randint(3, 128, (1, 7)).cuda()
        assert torch.equal(plain(input_ids=ids, encoder_hidden_states=enc, use_cache=False).logits, fused(input_ids=ids, encoder_hidden_states=enc, use_cache=False).logits)
    # training mode with a non-zero dropout on the stream (GPT-NeoX's two dropout children): the original forward, the same random stream
    _, plain, fused = _models(pq, "gpt_neox_seq", layers=2, hidden_dropout=0.25)
    assert len(_blocks(fused)) == 2 and set(_blocks(fused)[0]._rfb_plan.stateless) == {"post_attention_dropout", "post_mlp_dropout"}
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


@pytest.mark.parametrize("family", ["gpt_neox", "opt"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_refused_families_equal_their_unfused_selves(pq, family, dtype):
    from protoquant_amd.gptlike import residual_fused_blocks
    _, plain, fused = _models(pq, family, dtype, layers=2)
    assert residual_fused_blocks(fused) == 0 and G.module_types(plain) == G.module_types(fused)
    assert not any(hasattr(m, "_rf_layers") for m in fused.modules())
    ids = torch.randint(3, 128, (2, 11)).cuda()
    _same_outputs(fused, plain, ids, 3)
    with torch.no_grad():
        assert torch.equal(fused.generate(ids[:1, :5], max_new_tokens=4, do_sample=False, use_cache=True, pad_token_id=0),
                           plain.generate(ids[:1, :5], max_new_tokens=4, do_sample=False, use_cache=True, pad_token_id=0))
