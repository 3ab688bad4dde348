"""protoquant_amd — MI355X-native dynamic-int8 linear path behind the protoquant Python surface
(QTensor, quantize(), dequantize(), qlinear).  Hot path = hand-written HIP (gfx950) in
libpq_hip.so reached through the C-ABI in include/pq_hip.h; there is no CPU/eager fallback."""
from .qtensor import QTensor, quantize, dequantize, silu_mul_quantize, rmsnorm_quantize, silu_mul_rowamax, silu_mul_quantize_with_amax, rowamax, quantize_with_amax, glu_quantize, add_rmsnorm_quantize, layernorm_quantize, act_quantize, add_layernorm_quantize, add2_layernorm_quantize, layernorm_quantize2, gemma_rmsnorm_quantize, add_gemma_rmsnorm_quantize, gelu_mul_quantize, gemma_postnorm_add_rmsnorm_quantize, gemma_postnorm_add, olmo_postnorm_add_quantize, olmo_postnorm_add, olmo_rmsnorm, scaled_add_rmsnorm_quantize, scaled_add, head_rmsnorm
from .qlinear import qlinear, qlinear_s8, qlinear_s8_t, qlinear_s8_kslabs, qlinear_dyn, int_mm, clear_workspaces, swap_linears, FusedQLinear, GatedMLP, qlinear_s8_grouped, int_mm_grouped, qlinear_s8_grouped_stream, int_mm_grouped_stream
from .moe import GroupedQLinear, MoEGatedMLP, MoEBlock, swap_moe_experts, moe_route, moe_combine, moe_topk, clamped_experts_parts, ClampedExperts
from .moe_router import RouterParts, fuse_moe_routers, router_parts
from .gptlike import LayerNormQuant, ActQuant, fuse_layernorm_layers, fuse_layernorm_residual, residual_fused_blocks, fuse_parallel_residual, parallel_fused_blocks, parallel_flow_plan, ParallelFusedBlock
from .llama import RMSNormQuant, fuse_llama_layers
from .gemma import GemmaRMSNormQuant, GemmaSandwichNormQuant, SandwichFusedLayer, fuse_gemma_layers, fuse_gemma_postnorm_residual, is_gemma_rmsnorm, residual_flow_is_sandwich
from .olmo import OlmoRMSNorm, PostNormFusedLayer, fuse_olmo_layers, is_olmo_rmsnorm, residual_flow_is_postnorm
from .qk_norm import HeadRMSNorm, fuse_qk_norms, head_norm_kind
from .granite import ScaledResidualFusedLayer, fuse_granite_residual, residual_flow_is_scaled
from .sharded import (ColumnShardedGatedMLP, ColumnShardedQLinear, RcclColumnGather, RcclRowReduceScatter, RowShardedQLinear, ShardedGatedMLP,
                      gather_columns, gather_columns_overlapped, gather_rows_t, reduce_rows, shard_bounds)

__all__ = ["QTensor", "quantize", "dequantize", "qlinear", "qlinear_s8", "qlinear_dyn", "int_mm", "swap_linears", "FusedQLinear", "GatedMLP", "silu_mul_quantize", "rmsnorm_quantize",
           "ColumnShardedQLinear", "RcclColumnGather", "gather_columns", "shard_bounds", "RowShardedQLinear", "ShardedGatedMLP",
           "RcclRowReduceScatter", "reduce_rows", "gather_columns_overlapped", "gather_rows_t", "qlinear_s8_t", "clear_workspaces",
           "ColumnShardedGatedMLP", "qlinear_s8_kslabs", "silu_mul_rowamax", "silu_mul_quantize_with_amax", "rowamax", "quantize_with_amax",
           "qlinear_s8_grouped", "int_mm_grouped", "qlinear_s8_grouped_stream", "int_mm_grouped_stream", "GroupedQLinear", "MoEGatedMLP", "MoEBlock", "swap_moe_experts", "moe_route", "moe_combine", "glu_quantize", "clamped_experts_parts", "ClampedExperts", "add_rmsnorm_quantize",
           "layernorm_quantize", "act_quantize", "LayerNormQuant", "ActQuant", "fuse_layernorm_layers", "add_layernorm_quantize", "residual_fused_blocks", "fuse_layernorm_residual",
           "gemma_rmsnorm_quantize", "add_gemma_rmsnorm_quantize", "gelu_mul_quantize", "GemmaRMSNormQuant", "fuse_gemma_layers", "is_gemma_rmsnorm",
           "gemma_postnorm_add_rmsnorm_quantize", "gemma_postnorm_add", "SandwichFusedLayer", "GemmaSandwichNormQuant", "fuse_gemma_postnorm_residual", "residual_flow_is_sandwich",
           "add2_layernorm_quantize", "layernorm_quantize2", "fuse_parallel_residual", "parallel_fused_blocks", "parallel_flow_plan", "ParallelFusedBlock",
           "olmo_postnorm_add_quantize", "olmo_postnorm_add", "olmo_rmsnorm", "OlmoRMSNorm", "PostNormFusedLayer", "fuse_olmo_layers", "is_olmo_rmsnorm", "residual_flow_is_postnorm",
           "scaled_add_rmsnorm_quantize", "scaled_add", "ScaledResidualFusedLayer", "fuse_granite_residual", "residual_flow_is_scaled",
           "head_rmsnorm", "HeadRMSNorm", "fuse_qk_norms", "head_norm_kind",
           "moe_topk", "fuse_moe_routers", "router_parts", "RouterParts"]
