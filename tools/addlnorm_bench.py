"""Dev tool (GPU box): K1al (add_layernorm_quantize: residual add + LayerNorm + per-token int8 quantisation in one kernel) against the pair it replaces (torch add,
then layernorm_quantize = K1l) at 4096 x 768, 4096 x 4096, 4096 x 6144, 32 x 4096 and 1 x 6144 bf16 (4096 x 4096 in fp16 too), with a bias.  Each shape is first
compared bit for bit (codes, scales, the stored sum); then both candidates are captured into hipGraphs and replayed in turn, round by round, in ONE process.  Every
launch of a graph walks a rotation of input buffers larger than the 256-MiB Infinity Cache, so the large shapes are fed from HBM (the two small ones measure launches,
not bytes).  Bytes per element: 2 + 2 read, 2 + 1 written = 7 for the fused kernel; the pair moves 2 + 2 + 2 (the add) + 2 + 1 (K1l) = 9.  Changes no device setting.
usage: python tools/addlnorm_bench.py [--quick] [> profiles/r16_addlnorm_bench.txt]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((4096, 768, torch.bfloat16), (4096, 4096, torch.bfloat16), (4096, 4096, torch.float16), (4096, 6144, torch.bfloat16), (32, 4096, torch.bfloat16),
          (1, 6144, torch.bfloat16))
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
    print("# tools/addlnorm_bench.py  (one MI355X, one process)")
    print(f"# {torch.cuda.get_device_name(0)}; {time.strftime('%Y-%m-%d')}; medians [min .. max] per call of hipGraph replays, the two candidates replayed in turn")
    print("# fused = add_layernorm_quantize (K1al, 1 launch, 7 B/elem); pair = torch add + layernorm_quantize (K1l) (2 launches, 9 B/elem); weight and bias")
    for rows, cols, dt in SHAPES:
        nbuf = max(3, int(np.ceil(600e6 / (rows * cols * 2 * 2))))
        nbuf = min(nbuf, 64)                               # (the small shapes: a rotation of 64 pairs, cache-resident whatever one does)
        g = torch.Generator(device=dev).manual_seed(rows + cols)
        xs = [torch.randn(rows, cols, generator=g, device=dev).to(dt) for _ in range(nbuf)]
        rs = [(torch.randn(rows, cols, generator=g, device=dev) * 3).to(dt) for _ in range(nbuf)]
        w = (1 + 0.1 * torch.randn(cols, generator=g, device=dev)).to(dt)
        b = (0.1 * torch.randn(cols, generator=g, device=dev)).to(dt)
        name = str(dt).replace("torch.", "").replace("bfloat16", "bf16").replace("float16", "fp16")
        # bit for bit first
        qa, sa = pq.add_layernorm_quantize(xs[0], rs[0], w, b, EPS)
        sb = rs[0] + xs[0]
        qb = pq.layernorm_quantize(sb, w, b, EPS)
        torch.cuda.synchronize()
        same = torch.equal(sa, sb) and torch.equal(qa.int_data, qb.int_data) and torch.equal(qa.scale, qb.scale)
        assert same, f"{rows} x {cols}: the fused kernel and the pair differ"

        def fused(i):
            return pq.add_layernorm_quantize(xs[i % nbuf], rs[i % nbuf], w, b, EPS)

        def pair(i):
            s = rs[i % nbuf] + xs[i % nbuf]
            return pq.layernorm_quantize(s, w, b, EPS), s
        reps = 2 * nbuf if rows >= 1024 else 64
        graphs = [graph_of(fn, reps) for fn in (fused, pair)]
        tf, tp = time_graphs([g_ for g_, _ in graphs], reps, 6 if quick else 30)
        n = rows * cols
        fed = "HBM-fed" if nbuf * n * 4 > 512e6 else "cache-resident: launch-bound"
        print(f"{rows} x {cols} {name}  (rotation of {nbuf} x 2 x {n * 2 / 2**20:.2f} MiB inputs: {fed}; bit-identical: {same})")
        print(f"  fused (K1al)         {fmt(tf)}   {(7 * n + 4 * rows) / np.median(tf) / 1e6:5.2f} TB/s of its 7 B/elem")
        print(f"  pair  (add + K1l)    {fmt(tp)}   {(9 * n + 4 * rows) / np.median(tp) / 1e6:5.2f} TB/s of its 9 B/elem   pair / fused = x {np.median(tp) / np.median(tf):.2f}")
        del graphs, xs, rs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
