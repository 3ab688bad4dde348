"""Dev tool (GPU box): K1n (pq_rmsnorm_quant_rowwise) and K1a (pq_add_rmsnorm_quant_rowwise) of several library builds in ONE process, bf16: 4096 x 4096, 32 x 4096 and
4096 x 2600 (325 vectors: 256 threads x 2 with 187 dead slots).  Every build's call is captured into a hipGraph that walks a rotation of inputs larger than the Infinity
Cache (the large shapes), the graphs are replayed in turn, round by round; medians [min .. max] per call.  Outputs of all builds must be identical.  Changes no device setting.
usage: python tools/k1n_dead_slots_ab.py name=path/to/libpq_hip.so name2=path2 ... [> profiles/...txt]"""
import ctypes
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.addlnorm_bench import fmt, graph_of, time_graphs  # noqa: E402
from tools.gemma_bench import rotation  # noqa: E402

i32, i64, vp, f32 = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_float
SHAPES = ((4096, 4096), (32, 4096), (4096, 2600))
EPS = 1e-5


def load(path):
    L = ctypes.CDLL(os.path.abspath(path))
    L.pq_rmsnorm_quant_rowwise.restype = i32
    L.pq_rmsnorm_quant_rowwise.argtypes = [vp, i64, vp, f32, i32, i64, i64, vp, i64, vp, vp, i64, vp]
    L.pq_add_rmsnorm_quant_rowwise.restype = i32
    L.pq_add_rmsnorm_quant_rowwise.argtypes = [vp, i64, vp, i64, vp, i64, vp, f32, i32, i64, i64, vp, i64, vp, vp, i64, vp]
    return L


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    libs = [(s.split("=")[0], load(s.split("=")[1])) for s in sys.argv[1:] if "=" in s]
    assert len(libs) >= 2, __doc__
    rounds = 6 if "--quick" in sys.argv else 20
    dev = torch.device("cuda:0")
    st = lambda: torch.cuda.current_stream().cuda_stream              # noqa: E731
    print("# tools/k1n_dead_slots_ab.py  (one MI355X, one process, bf16): " + ", ".join(n for n, _ in libs))
    print(f"# {torch.cuda.get_device_name(0)}; {time.strftime('%Y-%m-%d')}; medians [min .. max] per call of hipGraph replays, the builds of a shape replayed in turn")
    for rows, cols in SHAPES:
        nbuf = rotation(rows, cols, 2)
        g = torch.Generator(device=dev).manual_seed(rows + cols)
        xs = [torch.randn(rows, cols, generator=g, device=dev).to(torch.bfloat16) for _ in range(nbuf)]
        rs = [(torch.randn(rows, cols, generator=g, device=dev) * 3).to(torch.bfloat16) for _ in range(nbuf)]
        w = (1 + 0.1 * torch.randn(cols, generator=g, device=dev)).to(torch.bfloat16)
        outs = []
        for kern in ("K1n", "K1a"):
            cands = []
            for name, L in libs:
                q = torch.empty((rows, cols), dtype=torch.int8, device=dev)
                sc = torch.empty(rows, dtype=torch.float32, device=dev)
                s = torch.empty((rows, cols), dtype=torch.bfloat16, device=dev)
                if kern == "K1n":
                    fn = lambda i, L=L, q=q, sc=sc: L.pq_rmsnorm_quant_rowwise(xs[i % nbuf].data_ptr(), cols, w.data_ptr(), EPS, 0, rows, cols, q.data_ptr(), cols,      # noqa: E731
                                                                               sc.data_ptr(), None, 0, st())
                else:
                    fn = lambda i, L=L, q=q, sc=sc, s=s: L.pq_add_rmsnorm_quant_rowwise(xs[i % nbuf].data_ptr(), cols, rs[i % nbuf].data_ptr(), cols, s.data_ptr(), cols,   # noqa: E731
                                                                                        w.data_ptr(), EPS, 0, rows, cols, q.data_ptr(), cols, sc.data_ptr(), None, 0, st())
                assert fn(0) == 0, (name, kern)
                torch.cuda.synchronize()
                outs.append((kern, q.clone(), sc.clone()))
                cands.append((name, fn))
            same = all(torch.equal(o[1], outs[-len(libs)][1]) and torch.equal(o[2].view(torch.int32), outs[-len(libs)][2].view(torch.int32)) for o in outs[-len(libs):])
            reps = 2 * nbuf if rows >= 1024 else 64
            graphs = [graph_of(fn, reps) for _, fn in cands]
            times = time_graphs([gr for gr, _ in graphs], reps, rounds)
            del graphs
            n = rows * cols
            fed = "HBM-fed" if nbuf * n * 4 > 512e6 else "cache-resident: launch-bound"
            print(f"{kern} {rows} x {cols}  (rotation of {nbuf} x 2 x {n * 2 / 2**20:.2f} MiB inputs: {fed}; identical outputs: {same})")
            lo, hi = max(min(t) for t in times), min(max(t) for t in times)
            for (name, _), t in zip(cands, times):
                print(f"  {name:12s} {fmt(t)}")
            print(f"  ranges overlap: {lo <= hi}   median / median of the first = " + ", ".join(f"x {np.median(t) / np.median(times[0]):.3f}" for t in times[1:]))
        del xs, rs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
