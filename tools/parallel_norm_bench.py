"""Dev tool (GPU box): the parallel-residual kernels against the launches they replace, at bf16 and 4096 / 32 / 1 rows x 2048 / 2560 / 4096 / 6144 columns, with biases:
  K1pl, two norms  (add2_layernorm_quantize with weight2: 1 launch, 10 B/elem)   against   two torch adds + layernorm_quantize (K1l) twice   (4 launches, 18 B/elem)
  K1pl, one norm   (add2_layernorm_quantize: 1 launch, 9 B/elem)                 against   two torch adds + K1l                            (3 launches, 15 B/elem)
  K1l2             (layernorm_quantize2: 1 launch, 4 B/elem)                     against   K1l twice                                       (2 launches, 6 B/elem)
Each shape is first compared bit for bit (codes, scales, the stored sum); then all six candidates are captured into hipGraphs and replayed in turn, round by round,
in ONE process.  Every launch of a graph walks a rotation of input buffers larger than the 256-MiB Infinity Cache, so the 4096-row shapes are fed from HBM (the small
ones measure launches, not bytes).  The baselines are kernels this tool's subject does not touch.  Changes no device setting.
usage: python tools/parallel_norm_bench.py [--quick] [> profiles/r20_parallel_norm_bench.txt]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.addlnorm_bench import fmt, graph_of, time_graphs          # noqa: E402

ROWS, COLS = (4096, 32, 1), (2048, 2560, 4096, 6144)
EPS1, EPS2 = 1e-5, 1e-6


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    import protoquant_amd as pq
    quick = "--quick" in sys.argv
    dev, dt = torch.device("cuda:0"), torch.bfloat16
    print("# tools/parallel_norm_bench.py  (one MI355X, one process)")
    print(f"# {torch.cuda.get_device_name(0)}; {time.strftime('%Y-%m-%d')}; bf16; medians [min .. max] per call of hipGraph replays, the six candidates of a shape replayed in turn")
    print("# K1pl x2 = add2_layernorm_quantize with two norms (1 launch, 10 B/elem) vs two torch adds + K1l twice (4 launches, 18 B/elem)")
    print("# K1pl x1 = add2_layernorm_quantize with one norm  (1 launch,  9 B/elem) vs two torch adds + K1l       (3 launches, 15 B/elem)")
    print("# K1l2    = layernorm_quantize2                    (1 launch,  4 B/elem) vs K1l twice                  (2 launches,  6 B/elem)")
    for rows in ROWS:
        for cols in COLS:
            n = rows * cols
            nbuf = min(max(3, int(np.ceil(600e6 / (n * 2 * 3)))), 64)          # (the small shapes: a rotation of 64 triples, cache-resident whatever one does)
            g = torch.Generator(device=dev).manual_seed(rows + cols)
            rnd = lambda scale: [(torch.randn(rows, cols, generator=g, device=dev) * scale).to(dt) for _ in range(nbuf)]          # noqa: E731
            xs, at, ml = rnd(1.0), rnd(3.0), rnd(0.5)
            w1, w2 = ((1 + 0.1 * torch.randn(cols, generator=g, device=dev)).to(dt) for _ in range(2))
            b1, b2 = ((0.1 * torch.randn(cols, generator=g, device=dev)).to(dt) for _ in range(2))

            def k1pl2(i):
                return pq.add2_layernorm_quantize(ml[i % nbuf], at[i % nbuf], xs[i % nbuf], w1, b1, EPS1, w2, b2, EPS2)

            def adds_k1l_twice(i):
                s = (ml[i % nbuf] + at[i % nbuf]) + xs[i % nbuf]
                return pq.layernorm_quantize(s, w1, b1, EPS1), pq.layernorm_quantize(s, w2, b2, EPS2), s

            def k1pl1(i):
                return pq.add2_layernorm_quantize(ml[i % nbuf], at[i % nbuf], xs[i % nbuf], w1, b1, EPS1)

            def adds_k1l(i):
                s = (ml[i % nbuf] + at[i % nbuf]) + xs[i % nbuf]
                return pq.layernorm_quantize(s, w1, b1, EPS1), s

            def k1l2(i):
                return pq.layernorm_quantize2(xs[i % nbuf], w1, b1, w2, b2, EPS1, EPS2)

            def k1l_twice(i):
                return pq.layernorm_quantize(xs[i % nbuf], w1, b1, EPS1), pq.layernorm_quantize(xs[i % nbuf], w2, b2, EPS2)

            # bit for bit first
            same = True
            for fused, base in ((k1pl2, adds_k1l_twice), (k1pl1, adds_k1l), (k1l2, k1l_twice)):
                for got, want in zip(fused(0), base(0)):
                    same = same and (torch.equal(got, want) if isinstance(got, torch.Tensor) else torch.equal(got.int_data, want.int_data) and torch.equal(got.scale, want.scale))
            torch.cuda.synchronize()
            assert same, f"{rows} x {cols}: a fused kernel and the launches it replaces differ"
            reps = 2 * nbuf if rows >= 1024 else 64
            cands = (k1pl2, adds_k1l_twice, k1pl1, adds_k1l, k1l2, k1l_twice)
            graphs = [graph_of(fn, reps) for fn in cands]
            t = time_graphs([g_ for g_, _ in graphs], reps, 6 if quick else 30)
            fed = "HBM-fed" if nbuf * n * 6 > 512e6 else "cache-resident: launch-bound"
            print(f"{rows} x {cols} bf16  (rotation of {nbuf} x 3 x {n * 2 / 2**20:.2f} MiB inputs: {fed}; bit-identical: {same})")
            rowsfmt = (("K1pl, two norms       ", "2 adds + K1l twice    ", 10, 18, 8), ("K1pl, one norm        ", "2 adds + K1l          ", 9, 15, 4),
                       ("K1l2                  ", "K1l twice             ", 4, 6, 8))
            for k, (nf, nb, bf, bb, brow) in enumerate(rowsfmt):
                tf, tb = t[2 * k], t[2 * k + 1]
                print(f"  {nf} {fmt(tf)}   {(bf * n + brow * rows) / np.median(tf) / 1e6:5.2f} TB/s of its {bf} B/elem")
                print(f"  {nb} {fmt(tb)}   {(bb * n + brow * rows) / np.median(tb) / 1e6:5.2f} TB/s of its {bb} B/elem   baseline / fused = x {np.median(tb) / np.median(tf):.2f}")
            del graphs, xs, at, ml
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
