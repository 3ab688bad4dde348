"""ctypes binding of libpq_hip.so (include/pq_hip.h).  There is NO fallback: if the HIP library is
missing or fails to load, every entry point raises — the product never routes through oracle/ or a
CPU/eager path."""
from __future__ import annotations

import ctypes
import os

import torch  # noqa: F401  (must be imported first: libpq_hip.so shares torch's libamdhip64.so.7)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpq_hip.so")
ABI_VERSION = 1

PQ_BF16, PQ_FP16, PQ_F32 = 0, 1, 2
GLU_KINDS = {"clamped_silu": 0, "alpha_sigmoid": 1}        # PQ_GLU_* of include/pq_hip.h
ACT_KINDS = {"relu": 0, "gelu_tanh": 1, "gelu_erf": 2}     # PQ_ACT_* of include/pq_hip.h
GAIN_KINDS = {"llama": 0, "gemma": 1}                      # PQ_GAIN_* of include/pq_hip.h
ROUTER_KINDS = {"softmax_topk": 0, "topk_softmax": 1}      # PQ_ROUTER_* of include/pq_hip.h
_DT = {torch.bfloat16: PQ_BF16, torch.float16: PQ_FP16, torch.float32: PQ_F32}

_lib = None
i32, i64, vp, sz, f32, cstr = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_float, ctypes.c_char_p

# symbol -> (restype, argtypes), the prototypes of include/pq_hip.h (tests/test_abi.py compares the two, parameter by parameter); None: no parameters.  Entries that
# share a prototype share its list.
_QUANT = [vp, i32, i64, i64, i64, vp, i64, vp, vp]
_QLINEAR = [vp, i64, vp, vp, i64, vp, vp, vp, i64, i32, i64, i64, i64, vp, sz, vp]
_WORKSPACE = [i64, i64, i64]
_GROUPED = [vp, i64, vp, i64, vp, vp, i64, i64, vp, vp, vp, i32, i64, i64, i64, vp, i64, i32, vp]
_GROUPED_GEMM = [vp, i64, vp, i64, vp, i64, i64, vp, i32, i64, i64, i64, vp, i64, vp]
_GROUPED_NAME = [i32, i64, i64, i64]
_RMSNORM = [vp, i64, vp, f32, i32, i64, i64, vp, i64, vp, vp, i64, vp]
_ADD_RMSNORM = [vp, i64, vp, i64, vp, i64, vp, f32, i32, i64, i64, vp, i64, vp, vp, i64, vp]
_SELFTEST = [i32, vp, vp]
SIGNATURES = {
    "pq_version": (i32, None),
    "pq_last_error": (cstr, None),
    "pq_quant_rowwise": (i32, _QUANT),
    "pq_quant_colwise": (i32, _QUANT),
    "pq_dequant": (i32, [vp, i64, vp, i32, i64, i64, vp, i64, i32, vp]),
    "pq_gemm_s8s8s32": (i32, [vp, i64, vp, i64, vp, i64, i64, i64, i64, vp]),
    "pq_qlinear_s8": (i32, _QLINEAR),
    "pq_qlinear_workspace_bytes": (sz, _WORKSPACE),
    "pq_gemm_variant_name": (cstr, [i64, i64, i64, i64, i64]),
    "pq_selftest_fast_quotient": (i32, [vp, vp, i64, vp, vp]),
    "pq_selftest_half_encode": (i32, _SELFTEST),
    "pq_selftest_silu_short": (i32, _SELFTEST),
    "pq_qlinear_dyn": (i32, [vp, i32, i64, vp, i64, vp, vp, vp, i64, i64, i64, i64, vp, sz, vp]),
    "pq_qlinear_dyn_workspace_bytes": (sz, _WORKSPACE),
    "pq_silu_mul_quant_rowwise": (i32, [vp, i64, vp, i64, i32, i64, i64, vp, i64, vp, vp, i64, vp]),
    "pq_rmsnorm_quant_rowwise": (i32, _RMSNORM),
    "pq_set_option": (i32, [cstr, cstr]),
    "pq_qlinear_s8_t": (i32, _QLINEAR),
    "pq_qlinear_t_workspace_bytes": (sz, _WORKSPACE),
    "pq_silu_mul_rowamax": (i32, [vp, i64, vp, i64, i32, i64, i64, vp, vp]),
    "pq_silu_mul_quant_rowwise_amax": (i32, [vp, i64, vp, i64, i32, i64, i64, vp, vp, i64, vp, vp]),
    "pq_qlinear_s8_kslabs": (i32, [vp, i64, i64, i64, vp, vp, i64, vp, vp, vp, i64, i32, i64, i64, i64, vp, sz, vp]),
    "pq_qlinear_kslabs_workspace_bytes": (sz, [i64, i64, i64, i64]),
    "pq_qlinear_kslabs_workspace_bytes_for": (sz, [vp, i64, i64, i64, vp, i64, i64, i64, i64]),
    "pq_kslabs_way_name": (cstr, [vp, i64, i64, i64, vp, i64, i64, i64, i64, sz]),
    "pq_quant_rowamax": (i32, [vp, i32, i64, i64, i64, vp, vp]),
    "pq_quant_rowwise_amax": (i32, [vp, i32, i64, i64, i64, vp, vp, i64, vp, vp]),
    "pq_qlinear_s8_grouped": (i32, _GROUPED),
    "pq_gemm_s8s8s32_grouped": (i32, _GROUPED_GEMM),
    "pq_grouped_variant_name": (cstr, _GROUPED_NAME),
    "pq_qlinear_s8_grouped_stream": (i32, _GROUPED),
    "pq_gemm_s8s8s32_grouped_stream": (i32, _GROUPED_GEMM),
    "pq_grouped_stream_plan_name": (cstr, _GROUPED_NAME),
    "pq_moe_route": (i32, [vp, i32, i64, i64, i32, i32, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
    "pq_moe_route_workspace_bytes": (sz, [i64, i32, i32]),
    "pq_moe_combine": (i32, [vp, i64, i32, i64, vp, vp, vp, i64, i64, i32, i64, vp, i64, vp]),
    "pq_glu_quant_rowwise": (i32, [vp, i64, vp, i64, i32, i64, i64, i32, f32, f32, vp, i64, vp, vp, i64, vp]),
    "pq_selftest_glu_short": (i32, [i32, i32, f32, f32, vp, vp]),
    "pq_add_rmsnorm_quant_rowwise": (i32, _ADD_RMSNORM),
    "pq_layernorm_quant_rowwise": (i32, [vp, i64, vp, vp, f32, i32, i64, i64, vp, i64, vp, vp, i64, vp]),
    "pq_act_quant_rowwise": (i32, [vp, i64, i32, i64, i64, i32, vp, i64, vp, vp, i64, vp]),
    "pq_add_layernorm_quant_rowwise": (i32, [vp, i64, vp, i64, vp, i64, vp, vp, f32, i32, i64, i64, vp, i64, vp, vp, i64, vp]),
    "pq_parallel_layernorm_quant_rowwise": (i32, [vp, i64, vp, i64, vp, i64, vp, i64, vp, vp, f32, vp, vp, f32, i32, i64, i64,
                                                  vp, i64, vp, vp, i64, vp, i64, vp, vp, i64, vp]),
    "pq_gemma_rmsnorm_quant_rowwise": (i32, _RMSNORM),
    "pq_add_gemma_rmsnorm_quant_rowwise": (i32, _ADD_RMSNORM),
    "pq_gelu_mul_quant_rowwise": (i32, [vp, i64, vp, i64, i32, i64, i64, i32, vp, i64, vp, vp, i64, vp]),
    "pq_gemma_postnorm_add_rmsnorm_quant_rowwise": (i32, [vp, i64, vp, f32, vp, i64, vp, i64, vp, f32, i32, i64, i64, vp, i64, vp, vp, i64, vp]),
    "pq_olmo_postnorm_add_quant_rowwise": (i32, [vp, i64, vp, f32, vp, i64, vp, i64, i32, i64, i64, vp, i64, vp, vp]),
    "pq_scaled_add_rmsnorm_quant_rows": (i32, [vp, i64, vp, i64, f32, vp, i64, vp, f32, i32, i64, i64, vp, i64, vp, vp, i64, vp]),
    "pq_head_rmsnorm": (i32, [vp, i64, i64, vp, f32, i32, i32, i64, i64, i64, vp, i64, i64, vp]),
    "pq_moe_topk": (i32, [vp, i32, i64, i64, i32, i32, i32, i32, vp, i32, i64, vp, i32, i64, vp]),
}
EXPORTS = tuple(SIGNATURES)


class PQError(RuntimeError):
    pass


def lib() -> ctypes.CDLL:
    """Load libpq_hip.so once; raise loudly when it is absent (build it with __graft_entry__.build()
    or `make -C protoquant_amd/csrc`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PQError(f"{LIB_PATH} not found: build it with `make -C protoquant_amd/csrc` "
                      "(protoquant_amd has no CPU/eager fallback)")
    L = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype = restype
        if argtypes is not None:
            fn.argtypes = argtypes
    if L.pq_version() != ABI_VERSION:
        raise PQError(f"libpq_hip.so ABI {L.pq_version()} != expected {ABI_VERSION}")
    _lib = L
    return L


def check(status: int, what: str):
    if status != 0:
        raise PQError(f"{what} failed (status {status}): {lib().pq_last_error().decode()}")


def set_option(name: str, value) -> None:
    """Change a behaviour switch of the loaded library (pq_set_option): PQ_FORCE_VARIANT, PQ_NO_TAILSPLIT, PQ_NO_SPLITK,
    PQ_SKINNY_RB.  value None / "" restores the default.  The environment variables are read once at the first call."""
    v = "" if value is None else str(value)
    check(lib().pq_set_option(name.encode(), v.encode()), f"pq_set_option({name})")


def dtype_code(dt: torch.dtype) -> int:
    try:
        return _DT[dt]
    except KeyError:
        raise TypeError(f"protoquant_amd supports bf16/fp16/fp32 tensors, got {dt}") from None


def require_gpu(t: torch.Tensor, name: str):
    if t.device.type != "cuda":
        raise PQError(f"{name} is on {t.device}: protoquant_amd runs on MI355X (HIP) only and has no "
                      "CPU fallback — move the tensor to the GPU")


def stream_ptr(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def row_major_2d(t: torch.Tensor) -> torch.Tensor:
    """A 2-D view whose last dim is contiguous (stride(1) == 1); copies only if it must."""
    if t.dim() != 2:
        raise ValueError("expected a 2-D tensor")
    if t.shape[1] > 0 and t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t


def ld(t: torch.Tensor) -> int:
    return t.stride(0) if t.shape[0] > 1 else max(t.shape[1], 1)
