"""-m gpu: ONE TABLE, one row per value of a behaviour switch that selects device code or launch geometry ("time only, never bits": pq_common.h, pq_hip.h).

Each row names the switch, its value, the operation, the CONDITION under which the launcher really takes the other path (quoted from the launcher), shapes that meet
it, and the fragment of the kernel name the row expects to launch.  A shape that does not meet the condition tests nothing, so every runner asserts the condition on its
shapes before it launches.  Every result is compared bit for bit with the oracle and with the bits of the default setting in the same process.

That the rows REACH their kernels is not something bits can show: the three files test_gpu_k_rotation.py, test_gpu_switch_paths.py and test_gpu_grouped_edges.py were run
once under a kernel trace on an MI355X, the list of kernel names and call counts is profiles/r21_switch_paths_kernels.txt, and tests/test_switch_coverage.py (CPU)
holds every fragment below against that list.

PQ_SP128_LC=2 (12 waves) exists only in ablation builds (PQ_ABLATION_BUILD, gemm_s8_fast.hip): the shipped library treats it as 1, so it has no row."""
import collections

import numpy as np
import pytest
import torch

from oracle import c_oracle as C
from oracle import qspec_numpy as Q
from tests.gpu_util import TD, bits, same, same_f, to_gpu

pytestmark = pytest.mark.gpu

Row = collections.namedtuple("Row", "switch value op condition shapes kernels")

# GEMM rows: the shape list of test_qlinear_vs_oracle (tests/test_gpu_parity.py) + one ragged shape of tests/test_gpu_k_rotation.py (rotation on, short last chunk)
GEMM_SHAPES = [(300, 520, 640), (256, 512, 1024), (77, 130, 384), (512, 1024, 512), (300, 1000, 8320)]
K1_ROWS = (1, 7, 8, 9, 1001)            # around the pairing of two rows per wave (8 rows per workgroup, 4 without)
K2_SHAPES = [(1, 8, 0), (1000, 520, 0), (4097, 1032, 1), (33, 50257, 0), (1000, 520, 2), (33, 50257, 2)]          # (rows, cols, dtype): 50257 columns = the scalar form
SKINNY_N = (37, 1000, 5120, 28672)

TABLE = [
    # ---- K1 (quant_kernels.hip, launch_rowwise_vec)
    Row("PQ_K1_RPW", "2", "k1", "TPR == kWave [nvec <= 64 * 8] && o.k1_rpw == 2 && vpt <= 8",
        [(r, c, d) for r in K1_ROWS for (c, d) in ((512, 0), (1040, 1), (4096, 0), (264, 2), (2048, 2))],
        ["quant_rowwise_vec<0, 1, 64, 2, false>", "quant_rowwise_vec<1, 4, 64, 2, false>", "quant_rowwise_vec<0, 8, 64, 2, false>", "quant_rowwise_vec<2, 2, 64, 2, false>",
         "quant_rowwise_vec<2, 8, 64, 2, false>"]),
    Row("PQ_K1_ST16", "1", "k1", "TPR == kWave && kBytes == 2 && k1_st16 && (nvec & 1) == 0 && (ldq & 15) == 0 && q 16-byte aligned && vpt >= 2 && vpt <= 8",
        [(r, c, d) for r in (1, 9, 1001) for (c, d) in ((1024, 0), (1040, 1), (3088, 0), (4096, 1))],
        ["quant_rowwise_vec<0, 2, 64, 1, true>", "quant_rowwise_vec<1, 4, 64, 1, true>", "quant_rowwise_vec<0, 8, 64, 1, true>", "quant_rowwise_vec<1, 8, 64, 1, true>"]),
    Row("PQ_K1_ST16", "1", "k1_fallback", "(ldq & 15) != 0, or q not 16-byte aligned, or an odd vector count: the 8-byte-store kernel runs and still matches",
        [(37, 1040, 0), (37, 3088, 1), (37, 1032, 0)], ["quant_rowwise_vec<0, 4, 64, 1, false>"]),
    Row("PQ_K1_LDS", "16384", "k1", "every launch of launch_rowwise_vec passes k1_lds as its dynamic LDS size: 64 threads per row (nvec <= 512) and 256",
        [(300, 4096, 0), (300, 2048, 2), (300, 8192, 0), (64, 11008, 1), (40, 40960, 0), (12, 32768, 2)],
        ["quant_rowwise_vec<0, 8, 64, 1, false>", "quant_rowwise_vec<0, 4, 256, 1, false>", "quant_rowwise_vec<2, 32, 256, 1, false>"]),
    Row("PQ_K1_LDS", "65536", "k1", "as above; 64 KiB per workgroup = at most two resident workgroups per CU",
        [(300, 4096, 0), (300, 2048, 2), (300, 8192, 0), (64, 11008, 1), (40, 40960, 0), (12, 32768, 2)], ["quant_rowwise_vec<1, 8, 256, 1, false>"]),
    # ---- K2 (quant_kernels.hip, quant_colwise_dispatch)
    *[Row(sw, v, "k2", "rpb = plan(k2_blocks > 0 ? k2_blocks : default, strips, batch): rows per workgroup of the amax / the encode pass, vectorised and scalar form",
          K2_SHAPES, ["col_amax<0, true>", "col_amax<0, false>", "col_encode<1, true>", "col_encode<2, false>"])
      for sw in ("PQ_K2_BLOCKS_A", "PQ_K2_BLOCKS_E") for v in ("1", "7", "100000")],
    # ---- K1s (producer_kernels.hip, silu_mul_quant_dispatch / silu_mul_split_dispatch; the ladder is rowmap_dispatch's, rowmap_kernels.h)
    Row("PQ_SILU_TPR", "256", "silu", "nvec > 1024 && nvec <= 1536 && opt().silu_tpr != 256 -> 512 threads x 3 vectors; with the switch: 256 threads x 8",
        [(33, 8200, 0), (130, 11008, 0), (9, 12288, 1), (33, 4100, 2), (17, 6144, 2)],
        ["rowmap_quant_rows<pq::SiluMulOp, 0, 8, 256, false, 0>", "rowmap_quant_rows<pq::SiluMulOp, 0, 8, 256, true, 0>", "rowmap_quant_rows<pq::SiluMulOp, 1, 8, 256, false, 1>",
         "rowmap_quant_rows<pq::SiluMulOp, 2, 8, 256, false, 2>", "rowmap_quant_rows<pq::SiluMulOp, 0, 3, 512, false, 0>"]),
    # ---- K1g (glu_kernels.hip, glu_quant_dispatch): the same ladder (rowmap_dispatch), both kinds
    Row("PQ_SILU_TPR", "256", "glu", "nvec > 1024 && nvec <= 1536 && opt().silu_tpr != 256 -> 512 threads x 3 vectors; with the switch: 256 threads x 8",
        [(33, 8200, 0), (9, 12288, 1), (17, 6144, 2)],
        ["rowmap_quant_rows<pq::GluOp<0>, 0, 8, 256, false, 0>", "rowmap_quant_rows<pq::GluOp<1>, 0, 8, 256, true, 0>", "rowmap_quant_rows<pq::GluOp<0>, 1, 8, 256, true, 0>",
         "rowmap_quant_rows<pq::GluOp<1>, 2, 8, 256, false, 0>", "rowmap_quant_rows<pq::GluOp<0>, 0, 3, 512, false, 0>"]),
    # ---- the weight-streaming kernel (gemm_s8_skinny.hip, skinny_plan / launch_gemm_skinny)
    *[Row("PQ_SKINNY_RB", v, "skinny", "if (const int f = opt().skinny_rb; f && mt <= 2) rb = f   [mt = ceil(M / 16)]",
          [(M, N, 1024) for M in (1, 16, 17, 32) for N in SKINNY_N], [f"gemm_s8_skinny<0, 1, {v}, true>", f"gemm_s8_skinny<3, 2, {v}, true>", f"gemm_s8_skinny<2, 1, {v}, false>"])
      for v in ("1", "2")],
    *[Row("PQ_SKINNY_KS", v, "skinny", "ks = 1; while (ks < f && ks < 16 && steps / (ks * 2) >= 1) ks <<= 1   [steps = K / 64: K = 128 clamps at 2]",
          [(M, N, K) for (M, N) in ((1, 1000), (9, 37), (32, 5120), (50, 1000)) for K in (128, 640, 8192)], ["gemm_s8_skinny<0, 1, 1, true>", "gemm_s8_skinny<1, 4, 1, true>"])
      for v in ("1", "2", "4", "8", "16")],
    Row("PQ_SKINNY_STAGE", "0", "skinny", "const bool stage = opt().skinny_stage && M > 1: all four token-tile counts of the unstaged kernel, rb = 1 and 2",
        [(M, N, K) for M in (2, 17, 33, 64) for (N, K) in ((37, 256), (1000, 2048), (5120, 1024))],
        ["gemm_s8_skinny<0, 1, 1, false>", "gemm_s8_skinny<0, 2, 1, false>", "gemm_s8_skinny<0, 3, 1, false>", "gemm_s8_skinny<0, 4, 1, false>", "gemm_s8_skinny<0, 2, 2, false>"]),
    # ---- the 128-row loader / consumer tiles (gemm_s8_fast.hip)
    Row("PQ_RING_LC", "0", "gemm:ring128", "if (opt().ring_lc || xs.tiles > 0) <LC form> else gemm_s8_ring128<OUT, false> on 256 threads (never with a stacked operand)",
        GEMM_SHAPES, ["gemm_s8_ring128<0, false, 0>", "gemm_s8_ring128<1, false, 0>", "gemm_s8_ring128<2, false, 0>", "gemm_s8_ring128<3, false, 0>"]),
    Row("PQ_SP128_LC", "0", "gemm:sp128_16", "if (opt().sp128_lc) <4 consumers + 4 loaders> else gemm_s8_sp256<OUT, 0, 128, 256> (8 symmetric waves)",
        GEMM_SHAPES, ["gemm_s8_sp256<0, 0, 128, 256, false, false, 0, 4, 0, false>", "gemm_s8_sp256<3, 0, 128, 256, false, false, 0, 4, 0, false>"]),
    # ---- planner only
    Row("PQ_NO_RING160", "1", "plan", "!options().no_ring160 && ... && t160 <= cus && t160 * 10 >= cus * 9: 4096 x 1280 x 8192 is the 128 x 160 tile's class",
        [(4096, 1280, 8192)], ["gemm_s8_ringt<0, 128, 160, 4, 1>", "gemm_s8_sp256<0, 0, 128, 256, true, false, 0, 4, 0, false>"]),
]
# kernels of the other two traced files that the recorded list must hold as well (tests/test_switch_coverage.py)
ALSO_TRACED = ["gemm_s8_ring128<0, true, 0>", "gemm_s8_ringt<0, 64, 128, 3, 2>", "gemm_s8_ringt<3, 64, 64, 4, 2>", "gemm_s8_grouped<0, 64, 128, 3, 2, true>",
               "gemm_s8_grouped<3, 64, 64, 4, 2, false>"]


@pytest.fixture(scope="module")
def pq():
    import protoquant_amd
    from protoquant_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available()
    return protoquant_amd


def _epv(code):
    return 4 if code == 2 else 8


def _x(rows, cols, code, seed):
    rng = np.random.default_rng(seed)
    xf = (rng.standard_normal((rows, cols)) * rng.uniform(0.05, 20)).astype(np.float32)
    if rows > 2:
        xf[1] = 0                                   # a zero row (scale 1) beside its pair
        xf[2, cols // 3] = np.nan
    if rows > 8:
        xf[8, 0] = np.inf
    return Q.from_f32(xf, code)


# ---------------------------------------------------------------- runners: one per operation
def _run_k1(pq, pq_opt, row):
    for rows, cols, code in row.shapes:
        nvec = cols // _epv(code)
        assert cols % _epv(code) == 0 and nvec <= 256 * 32
        if row.switch == "PQ_K1_RPW":
            assert nvec <= 512
        if row.switch == "PQ_K1_ST16":
            assert code != 2 and 65 <= nvec <= 512 and nvec % 2 == 0 and cols % 16 == 0
        x = _x(rows, cols, code, rows * 7919 + cols + code)
        xg = to_gpu(x, code)
        wq, ws = C.quant_rowwise(x, code)
        d = pq.quantize(xg, axis=-1)
        same(d.int_data, wq, f"default codes {rows}x{cols}/{code}"); same(d.scale, ws, "default scale")
        pq_opt(row.switch, row.value)
        q = pq.quantize(xg, axis=-1)
        pq_opt(row.switch, "")
        same(q.int_data, wq, f"{row.switch}={row.value} codes {rows}x{cols}/{code}"); same(q.scale, ws, f"{row.switch}={row.value} scale {rows}x{cols}/{code}")
        assert torch.equal(q.int_data, d.int_data) and torch.equal(q.scale.view(torch.int32), d.scale.view(torch.int32))


def _run_k1_fallback(pq, pq_opt, row):
    """through the C-ABI: a code buffer whose leading dimension is not a multiple of 16, one that starts 8 bytes into a 16-byte line, and an odd vector count"""
    from protoquant_amd import _lib
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    for rows, cols, code in row.shapes:
        x = _x(rows, cols, code, rows + cols + code)
        xg = to_gpu(x, code)
        wq, ws = C.quant_rowwise(x, code)
        for pad, off in ((8, 0), (16, 8), (0, 0)):
            if (pad, off) == (0, 0) and (cols // 8) % 2 == 0:
                continue                        # (the aligned, even case is the row above)
            ldq = cols + pad
            assert ldq % 16 != 0 or off % 16 != 0 or (cols // 8) % 2 == 1
            outs = []
            for value in ("", row.value):
                pq_opt(row.switch, value)
                qb = torch.full((rows, ldq), 77, dtype=torch.int8, device="cuda")
                sc = torch.empty(rows, dtype=torch.float32, device="cuda")
                _lib.check(L.pq_quant_rowwise(xg.data_ptr(), code, rows, cols, cols, qb.data_ptr() + off, ldq, sc.data_ptr(), st), "k1")
                got = qb.flatten()[off:off + (rows - 1) * ldq + cols].cpu().numpy()
                win = np.lib.stride_tricks.as_strided(got, (rows, cols), (ldq, 1))
                assert np.array_equal(win, wq), f"{row.switch}={value!r} {rows}x{cols} pad {pad} off {off}"
                same(sc, ws, "scale")
                outs.append(qb)
            pq_opt(row.switch, "")
            assert torch.equal(outs[0], outs[1]), "bytes outside the window included: the two settings wrote the same buffer"
            whole = outs[1].flatten().cpu().numpy()
            mask = np.ones(whole.shape, bool)
            for r in range(rows):
                mask[off + r * ldq: off + r * ldq + cols] = False
            assert np.all(whole[mask] == 77), "wrote outside its window"


def _run_k2(pq, pq_opt, row):
    for rows, cols, code in row.shapes:
        x = _x(rows, cols, code, rows * 31 + cols + code)
        xg = to_gpu(x, code)
        cq, cs = C.quant_colwise(x, code)
        d = pq.quantize(xg, axis=0)
        same(d.int_data, cq, "default col codes"); same(d.scale, cs, "default col scale")
        pq_opt(row.switch, row.value)
        q = pq.quantize(xg, axis=0)
        pq_opt(row.switch, "")
        same(q.int_data, cq, f"{row.switch}={row.value} col codes {rows}x{cols}/{code}"); same(q.scale, cs, f"{row.switch}={row.value} col scale {rows}x{cols}/{code}")


def _run_silu(pq, pq_opt, row):
    for rows, cols, code in row.shapes:
        nvec = cols // _epv(code)
        assert cols % _epv(code) == 0 and 1024 < nvec <= 1536
        rng = np.random.default_rng(rows * 131 + cols + code)
        g = Q.from_f32((rng.standard_normal((rows, cols)) * 2.5).astype(np.float32), code)
        u = Q.from_f32(rng.standard_normal((rows, cols)).astype(np.float32), code)
        gt, ut = to_gpu(g, code), to_gpu(u, code)
        want_q, want_s, want_h = C.silu_mul_quant_rowwise(g, u, code)
        want_amax = Q.row_amax_bits(Q.silu_mul(g, u, code), code)
        res = []
        for value in ("", row.value):
            pq_opt(row.switch, value)
            qt, h = pq.silu_mul_quantize(gt, ut, return_h=True)
            q2 = pq.silu_mul_quantize(gt, ut)
            am = pq.silu_mul_rowamax(gt, ut)
            q3 = pq.silu_mul_quantize_with_amax(gt, ut, am)
            what = f"{row.switch}={value!r} {rows}x{cols}/{code}"
            same(qt.int_data, want_q, what + " q"); same(qt.scale, want_s, what + " scale"); same(h, want_h, what + " h")
            same(q2.int_data, want_q, what + " q (no h)"); same(q2.scale, want_s, what + " scale (no h)")
            assert np.array_equal(am.cpu().numpy().view(np.uint32), want_amax), what + " row amax"
            same(q3.int_data, want_q, what + " q (amax form)"); same(q3.scale, want_s, what + " scale (amax form)")
            res.append((qt.int_data, h))
        pq_opt(row.switch, "")
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1].view(torch.uint8), res[1][1].view(torch.uint8))


def _run_glu(pq, pq_opt, row):
    from tests import glu_spec as G
    for rows, cols, code in row.shapes:
        nvec = cols // _epv(code)
        assert cols % _epv(code) == 0 and 1024 < nvec <= 1536
        rng = np.random.default_rng(rows * 137 + cols + code)
        g = (rng.standard_normal((rows, cols)) * 4).astype(np.float32)
        u = (rng.standard_normal((rows, cols)) * 4).astype(np.float32)
        if code != 2:
            g, u = Q.from_f32(g, code), Q.from_f32(u, code)
        gt, ut = to_gpu(g, code), to_gpu(u, code)
        for kname, kind, alpha in (("clamped_silu", G.CLAMPED_SILU, None), ("alpha_sigmoid", G.ALPHA_SIGMOID, 1.702)):
            want_q, want_s, want_h = G.glu_quantize(g, u, code, kind, 7.0, alpha or 0.0)
            res = []
            for value in ("", row.value):
                pq_opt(row.switch, value)
                qt, h = pq.glu_quantize(gt, ut, kname, 7.0, alpha, return_h=True)
                q2 = pq.glu_quantize(gt, ut, kname, 7.0, alpha)
                what = f"{row.switch}={value!r} {kname} {rows}x{cols}/{code}"
                same(qt.int_data, want_q, what + " q"); same(qt.scale, want_s, what + " scale"); same_f(h, want_h, code, what + " h")
                same(q2.int_data, want_q, what + " q (no h)"); same(q2.scale, want_s, what + " scale (no h)")
                res.append((qt.int_data, h))
            pq_opt(row.switch, "")
            assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1].view(torch.uint8), res[1][1].view(torch.uint8))


def _gemm_operands(M, N, K, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(-128, 128, (M, K), dtype=np.int8); b = rng.integers(-128, 128, (N, K), dtype=np.int8)
    xs = (rng.random(M, dtype=np.float32) * 0.1 + 1e-3).astype(np.float32); ws = (rng.random(N, dtype=np.float32) * 0.01 + 1e-4).astype(np.float32)
    bias = {c: Q.from_f32(rng.standard_normal(N).astype(np.float32), c) for c in (0, 1, 2)}
    return a, b, xs, ws, bias, Q.gemm_s8s8s32(a, b)


def _gemm_all_kinds(pq, pq_opt, row, shapes, name):
    """all four output kinds, bias on and off, under "" and under the row's value: == the oracle, and the two settings == each other"""
    from protoquant_amd import _lib
    for (M, N, K) in shapes:
        assert _lib.lib().pq_gemm_variant_name(M, N, K, K, K) == name, (M, N, K)
        a, b, xs, ws, bias, acc = _gemm_operands(M, N, K, M * 1000003 + N * 1009 + K)
        ag, bg, xg, wg = (torch.from_numpy(t).cuda() for t in (a, b, xs, ws))
        outs = []
        for value in ("", row.value):
            pq_opt(row.switch, value)
            what = f"{row.switch}={value!r} {M}x{N}x{K}"
            got = [pq.int_mm(ag, bg)]
            same(got[0], acc, what + " int32")
            for code in (0, 1, 2):
                for bv in (None, bias[code]):
                    y = pq.qlinear_s8(ag, xg, bg, wg, to_gpu(bv, code) if bv is not None else None, TD[code])
                    same(y, Q.epilogue(acc, xs, ws, bv, code), what + f" code {code} bias {bv is not None}")
                    got.append(y)
            outs.append(got)
        pq_opt(row.switch, "")
        for y0, y1 in zip(*outs):
            assert torch.equal(y0.view(torch.uint8), y1.view(torch.uint8))


def _run_skinny(pq, pq_opt, row):
    pq_opt("PQ_FORCE_VARIANT", "skinny")
    for (M, N, K) in row.shapes:
        assert M <= 64 and K % 128 == 0
        if row.switch == "PQ_SKINNY_RB":
            assert (M + 15) // 16 <= 2
        if row.switch == "PQ_SKINNY_STAGE":
            assert M > 1
    _gemm_all_kinds(pq, pq_opt, row, row.shapes, b"skinny_16x16x64")


def _run_gemm(pq, pq_opt, row):
    variant = row.op.split(":")[1]
    pq_opt("PQ_FORCE_VARIANT", variant)
    _gemm_all_kinds(pq, pq_opt, row, row.shapes, {"ring128": b"ring128_16x16x64", "sp128_16": b"sp128x256_16x16x64"}[variant])


def _run_plan(pq, pq_opt, row):
    """the name changes, the bits do not"""
    from protoquant_amd import _lib
    L = _lib.lib()
    (M, N, K), = row.shapes
    a, b, xs, ws, bias, acc = _gemm_operands(M, N, K, 160)
    ag, bg, xg, wg, bb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), torch.from_numpy(xs).cuda(), torch.from_numpy(ws).cuda(), to_gpu(bias[0], 0)
    assert L.pq_gemm_variant_name(M, N, K, K, K) == b"ring128x160_16x16x64"
    y0 = pq.qlinear_s8(ag, xg, bg, wg, bb, torch.bfloat16)
    pq_opt(row.switch, row.value)
    assert L.pq_gemm_variant_name(M, N, K, K, K) == b"sp128x256_16x16x64"
    y1 = pq.qlinear_s8(ag, xg, bg, wg, bb, torch.bfloat16)
    assert torch.equal(y0.view(torch.int16), y1.view(torch.int16))
    rows = sorted({0, 1, 127, 128, 2047, 2048, M - 129, M - 1})           # sampled rows against the oracle (tests/test_gpu_model_shapes.py does the same)
    assert np.array_equal(bits(y1[torch.tensor(rows, device="cuda")]), Q.epilogue(acc[rows], xs[rows], ws, bias[0], 0))


RUNNERS = {"k1": _run_k1, "k1_fallback": _run_k1_fallback, "k2": _run_k2, "silu": _run_silu, "glu": _run_glu, "skinny": _run_skinny, "gemm:ring128": _run_gemm, "gemm:sp128_16": _run_gemm,
           "plan": _run_plan}


@pytest.mark.parametrize("row", TABLE, ids=[f"{r.switch}={r.value}-{r.op}" for r in TABLE])
def test_switch_row(pq, pq_opt, row):
    RUNNERS[row.op](pq, pq_opt, row)


def test_table_names_every_switch_of_this_file_once_per_value():
    ids = [(r.switch, r.value, r.op) for r in TABLE]
    assert len(set(ids)) == len(ids)
    assert {r.switch for r in TABLE} == {"PQ_K1_RPW", "PQ_K1_ST16", "PQ_K1_LDS", "PQ_K2_BLOCKS_A", "PQ_K2_BLOCKS_E", "PQ_SILU_TPR", "PQ_SKINNY_RB", "PQ_SKINNY_KS",
                                         "PQ_SKINNY_STAGE", "PQ_RING_LC", "PQ_SP128_LC", "PQ_NO_RING160"}
