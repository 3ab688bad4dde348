"""Tiny mixture-of-experts decoders for the tests of swap_moe_experts on real model code: one config builder per transformers family (random seeded initialisation,
nothing is downloaded), the table of what the library does with each, and the 4.x ModuleList layout as look-alike classes that can stand in a real decoder layer."""
import torch
from torch import nn

VOCAB = 128

# family -> (what swap_moe_experts does, why).  "experts": the fused-parameter `experts` module of every sparse layer is replaced by MoEGatedMLP and nothing else of
# the block is touched; "refused": swap_moe_experts returns 0 and every module object stays the very same object.
TABLE = {
    "mixtral": ("experts", "MixtralExperts [E, 2I, H] / [E, H, I], silu; router (softmax, top-k, renormalise, f32 scores) stays the model's"),
    "qwen3_moe": ("experts", "Qwen3MoeExperts, as Mixtral's; norm_topk_prob is the router's business"),
    "olmoe": ("experts", "OlmoeExperts, as Mixtral's"),
    "qwen2_moe": ("experts", "Qwen2MoeExperts; shared_expert and shared_expert_gate stay the model's modules and still run"),
    "deepseek_v3": ("experts", "DeepseekV3Experts only: the sigmoid / grouped top-k router, routed_scaling_factor and shared_experts stay the model's code"),
    "phimoe": ("experts", "PhimoeExperts is Mixtral's arithmetic; the sparsemixer router (an nn.Linear subclass) stays the model's and is NOT a linear layer to swap_linears"),
    "granitemoe": ("experts", "GraniteMoeExperts is Mixtral's arithmetic; the top-k-then-softmax router stays the model's"),
    "deepseek_v4": ("refused", "DeepseekV4Experts has Mixtral's shapes, silu, flags and signature, and clamps gate and up to +-swiglu_limit in an _apply_gate of its own"),
    "gpt_oss": ("refused", "gate_up_proj is [E, H, 2I] with interleaved gate / up columns, biases, a clamped alpha-sigmoid gate instead of an act_fn"),
}
SWAPPED = tuple(f for f, (what, _) in TABLE.items() if what == "experts")
REFUSED = tuple(f for f, (what, _) in TABLE.items() if what == "refused")


def config(family: str, H=64, I=128, E=4, k=2, layers=2, act="silu", **over):
    """The smallest config of a family: `layers` decoder layers, hidden H, expert intermediate I, E experts, top-k k.  experts_implementation = "eager": the float
    model runs its own loop over the experts, the arithmetic the library restates."""
    import transformers as tr
    base = dict(vocab_size=VOCAB, hidden_size=H, num_hidden_layers=layers, num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=256,
                hidden_act=act, experts_implementation="eager", pad_token_id=0, bos_token_id=1, eos_token_id=2)
    per = {
        "mixtral": (tr.MixtralConfig, dict(intermediate_size=I, num_local_experts=E, num_experts_per_tok=k)),
        "qwen3_moe": (tr.Qwen3MoeConfig, dict(intermediate_size=2 * I, moe_intermediate_size=I, num_experts=E, num_experts_per_tok=k, head_dim=H // 4, mlp_only_layers=[],
                                             decoder_sparse_step=1, norm_topk_prob=True)),
        "olmoe": (tr.OlmoeConfig, dict(intermediate_size=I, num_experts=E, num_experts_per_tok=k)),
        "qwen2_moe": (tr.Qwen2MoeConfig, dict(intermediate_size=2 * I, moe_intermediate_size=I, shared_expert_intermediate_size=I, num_experts=E, num_experts_per_tok=k,
                                             mlp_only_layers=[], decoder_sparse_step=1)),
        "deepseek_v3": (tr.DeepseekV3Config, dict(intermediate_size=2 * I, moe_intermediate_size=I, n_routed_experts=E, num_experts_per_tok=k, n_group=2 if E % 2 == 0 else 1,
                                                 topk_group=1 if k <= E // 2 else (2 if E % 2 == 0 else 1), first_k_dense_replace=1, n_shared_experts=1, num_key_value_heads=4, q_lora_rank=32,
                                                 kv_lora_rank=16, qk_rope_head_dim=8, qk_nope_head_dim=8, v_head_dim=H // 4)),
        "deepseek_v4": (tr.DeepseekV4Config, dict(moe_intermediate_size=I, n_routed_experts=E, num_experts_per_tok=k)),
        "gpt_oss": (tr.GptOssConfig, dict(intermediate_size=I, num_local_experts=E, num_experts_per_tok=k, head_dim=H // 4)),
        "phimoe": (tr.PhimoeConfig, dict(intermediate_size=I, num_local_experts=E, num_experts_per_tok=k)),
        "granitemoe": (tr.GraniteMoeConfig, dict(intermediate_size=I, num_local_experts=E, num_experts_per_tok=k)),
        "llama": (tr.LlamaConfig, dict(intermediate_size=I)),
    }
    cls, kw = per[family]
    kw = dict(base, **kw)
    kw.update(over)
    return cls(**kw)


def build(family: str, seed=0, **kw):
    """A seeded float32 CPU model of the family (AutoModelForCausalLM.from_config), in eval mode"""
    import transformers as tr
    torch.manual_seed(seed)
    return tr.AutoModelForCausalLM.from_config(config(family, **kw)).eval()


def sparse_blocks(model):
    """(qualified name, block) of every module that holds a fused-parameter `experts` child: the sparse MoE blocks of a transformers 5 decoder"""
    return [(n, m) for n, m in model.named_modules() if isinstance(getattr(m, "experts", None), nn.Module) and "gate_up_proj" in dict(m.experts.named_parameters(recurse=False))]


# ------------------------------------------------------------------------------------------------ the 4.x layout: one module per expert, a Linear router
class ListExpert(nn.Module):
    def __init__(self, H, I, names=("gate_proj", "up_proj", "down_proj")):
        super().__init__()
        self.names = names
        for n, (i, o) in zip(names, ((H, I), (H, I), (I, H))):
            setattr(self, n, nn.Linear(i, o, bias=False))
        self.act_fn = nn.SiLU()

    def forward(self, x):
        g, u, d = (getattr(self, n) for n in self.names)
        return d(self.act_fn(g(x)) * u(x))


class ListMoeBlock(nn.Module):
    """Mixtral's block as transformers 4.x wrote it — a ModuleList of experts and a Linear router, softmax / top-k / renormalise in the block — returning a TENSOR, so
    that it can stand where a transformers 5 decoder layer expects its block (the name does not end in SparseMoeBlock, and return_router_logits says so)."""
    return_router_logits = False

    def __init__(self, E, H, I, top_k, names=("gate_proj", "up_proj", "down_proj"), norm_topk_prob=True):
        super().__init__()
        self.top_k, self.norm_topk_prob = top_k, norm_topk_prob
        self.gate = nn.Linear(H, E, bias=False)
        self.experts = nn.ModuleList([ListExpert(H, I, names) for _ in range(E)])

    def forward(self, hidden_states):
        x = hidden_states.reshape(-1, hidden_states.shape[-1])
        w = torch.softmax(self.gate(x), dim=1, dtype=torch.float)
        w, sel = torch.topk(w, self.top_k, dim=-1)
        w = (w / w.sum(dim=-1, keepdim=True) if self.norm_topk_prob else w).to(x.dtype)
        final = torch.zeros_like(x)
        for e, expert in enumerate(self.experts):
            tok, slot = torch.where(sel == e)
            if tok.numel():
                final.index_add_(0, tok, (expert(x[tok]) * w[tok, slot, None]).to(x.dtype))
        return final.reshape(hidden_states.shape)

    @classmethod
    def from_stacked(cls, gate_weight, gate_up_proj, down_proj, top_k, norm_topk_prob=True):
        """the same experts as a fused-parameter module holds them: expert e's gate = gate_up_proj[e, :I], up = gate_up_proj[e, I:], down = down_proj[e]"""
        E, H, I = gate_up_proj.shape[0], gate_up_proj.shape[2], down_proj.shape[2]
        blk = cls(E, H, I, top_k, norm_topk_prob=norm_topk_prob).to(device=gate_up_proj.device, dtype=gate_up_proj.dtype)
        with torch.no_grad():
            blk.gate.weight.copy_(gate_weight)
            for e, ex in enumerate(blk.experts):
                ex.gate_proj.weight.copy_(gate_up_proj[e, :I])
                ex.up_proj.weight.copy_(gate_up_proj[e, I:])
                ex.down_proj.weight.copy_(down_proj[e])
        return blk
