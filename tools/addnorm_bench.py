"""Dev tool (GPU box): K1a (add_rmsnorm_quantize: residual add + RMSNorm + per-token int8 quantisation in one kernel) against the pair it replaces (torch add, then
rmsnorm_quantize = K1n) at 4096 x 4096, 4096 x 8192, 32 x 4096 and 1 x 8192 bf16.  Each shape is first compared bit for bit (codes, scales, the stored sum); then both
candidates are captured into hipGraphs and replayed in turn, round by round, in ONE process.  Every launch of a graph walks a rotation of input buffers larger than the
256-MiB Infinity Cache, so the large shapes are fed from HBM (the two small ones measure launches, not bytes).  Bytes per element: 2 + 2 read, 2 + 1 written = 7 for
the fused kernel; the pair moves 2 + 2 + 2 (the add) + 2 + 1 (K1n) = 9.
usage: python tools/addnorm_bench.py [--quick] [> profiles/r13_addnorm_bench.txt]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((4096, 4096), (4096, 8192), (32, 4096), (1, 8192))
EPS = 1e-5


def graph_of(fn, reps):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn(0)                                               # warm-up outside capture (code objects)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        keep = [fn(i) for i in range(reps)]
    return gr, keep


def time_graphs(graphs, reps, rounds):
    """per graph, microseconds per launch of every round; the graphs are replayed in turn"""
    out = [[] for _ in graphs]
    for gr in graphs:
        gr.replay()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for i, gr in enumerate(graphs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            gr.replay()
            b.record()
            b.synchronize()
            out[i].append(a.elapsed_time(b) * 1e3 / reps)
    return out


def fmt(v):
    return f"{np.median(v):8.2f} us [{min(v):.2f} .. {max(v):.2f}]"


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    import protoquant_amd as pq
    quick = "--quick" in sys.argv
    dev = torch.device("cuda:0")
    print("# tools/addnorm_bench.py  (one MI355X, one process)")
    print(f"# {torch.cuda.get_device_name(0)}; {time.strftime('%Y-%m-%d')}; medians [min .. max] per call of hipGraph replays, the two candidates replayed in turn; bf16")
    print("# fused = add_rmsnorm_quantize (K1a, 1 launch, 7 B/elem); pair = torch add + rmsnorm_quantize (K1n) (2 launches, 9 B/elem)")
    for rows, cols in SHAPES:
        nbuf = max(3, int(np.ceil(600e6 / (rows * cols * 2 * 2))))
        nbuf = min(nbuf, 64)                               # (the small shapes: a rotation of 64 pairs, cache-resident whatever one does)
        g = torch.Generator(device=dev).manual_seed(rows + cols)
        xs = [torch.randn(rows, cols, generator=g, device=dev).to(torch.bfloat16) for _ in range(nbuf)]
        rs = [(torch.randn(rows, cols, generator=g, device=dev) * 3).to(torch.bfloat16) for _ in range(nbuf)]
        w = (1 + 0.1 * torch.randn(cols, generator=g, device=dev)).to(torch.bfloat16)
        # bit for bit first
        qa, sa = pq.add_rmsnorm_quantize(xs[0], rs[0], w, EPS)
        sb = rs[0] + xs[0]
        qb = pq.rmsnorm_quantize(sb, w, EPS)
        torch.cuda.synchronize()
        same = torch.equal(sa, sb) and torch.equal(qa.int_data, qb.int_data) and torch.equal(qa.scale, qb.scale)
        assert same, f"{rows} x {cols}: the fused kernel and the pair differ"

        def fused(i):
            return pq.add_rmsnorm_quantize(xs[i % nbuf], rs[i % nbuf], w, EPS)

        def pair(i):
            s = rs[i % nbuf] + xs[i % nbuf]
            return pq.rmsnorm_quantize(s, w, EPS), s
        reps = 2 * nbuf if rows >= 1024 else 64
        graphs = [graph_of(fn, reps) for fn in (fused, pair)]
        tf, tp = time_graphs([g_ for g_, _ in graphs], reps, 6 if quick else 30)
        n = rows * cols
        fed = "HBM-fed" if nbuf * n * 4 > 512e6 else "cache-resident: launch-bound"
        print(f"{rows} x {cols} bf16  (rotation of {nbuf} x 2 x {n * 2 / 2**20:.2f} MiB inputs: {fed}; bit-identical: {same})")
        print(f"  fused (K1a)          {fmt(tf)}   {(7 * n + 4 * rows) / np.median(tf) / 1e6:5.2f} TB/s of its 7 B/elem")
        print(f"  pair  (add + K1n)    {fmt(tp)}   {(9 * n + 4 * rows) / np.median(tp) / 1e6:5.2f} TB/s of its 9 B/elem   pair / fused = x {np.median(tp) / np.median(tf):.2f}")
        del graphs, xs, rs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
