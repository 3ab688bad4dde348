"""Dev tool (GPU box): the three Gemma kernels against what they stand next to and what they replace, bf16.
  K1ng  (gemma_rmsnorm_quantize)      vs K1n (rmsnorm_quantize) at the same shape — both move 3 B/elem — and vs transformers' eager GemmaRMSNorm chain + K1 (quantize)
  K1ang (add_gemma_rmsnorm_quantize)  vs the torch add + the eager chain + K1
  K1gg  (gelu_mul_quantize)           vs K1s (silu_mul_quantize) at the same shape — both move 5 B/elem — and vs F.gelu(g, approximate="tanh") * u + K1 (13 B/elem)
at hidden 2048 / 2304 / 3072 / 3584 / 4608, intermediate 16384 / 9216 / 24576 / 14336 and 4096, 32 and 1 rows.  Every candidate of a shape is captured into a hipGraph and
the graphs are replayed in turn, round by round, in ONE process.  Every launch of a graph walks a rotation of input buffers larger than the 256-MiB Infinity Cache, so
the large shapes are fed from HBM (the small ones measure launches, not bytes).  K1ng is to be judged against K1n IN THE SAME RUN (within its [min .. max] spread), K1gg
against the torch chain.  Changes no device setting.
usage: python tools/gemma_bench.py [--quick] [> profiles/r18_gemma_bench.txt]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.addlnorm_bench import fmt, graph_of, time_graphs  # noqa: E402

HIDDEN = (2048, 2304, 3072, 3584, 4608)
INTERMEDIATE = (16384, 9216, 24576, 14336)
ROWS = (4096, 32, 1)
EPS = 1e-6
DT = torch.bfloat16


def gemma_eager(x, w):
    """transformers' GemmaRMSNorm.forward, op for op"""
    xf = x.float()
    out = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + EPS)
    return (out * (1.0 + w.float())).type_as(x)


def rotation(rows, cols, tensors_per_set):
    nbuf = max(3, int(np.ceil(600e6 / (rows * cols * 2 * tensors_per_set))))
    return min(nbuf, 64)          # (the small shapes: a rotation of 64 sets, cache-resident whatever one does)


def run(cands, reps, rounds):
    graphs = [graph_of(fn, reps) for _, fn in cands]
    times = time_graphs([g for g, _ in graphs], reps, rounds)
    del graphs
    return times


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    import protoquant_amd as pq
    rounds = 6 if "--quick" in sys.argv else 20
    dev = torch.device("cuda:0")
    print("# tools/gemma_bench.py  (one MI355X, one process, bf16)")
    print(f"# {torch.cuda.get_device_name(0)}; {time.strftime('%Y-%m-%d')}; medians [min .. max] per call of hipGraph replays, the candidates of a shape replayed in turn")
    print("# norms: K1ng / K1n 1 launch, 3 B/elem; eager = GemmaRMSNorm's torch chain + K1; K1ang 1 launch, 7 B/elem; add + eager = torch add + that chain + K1")
    for cols in HIDDEN:
        for rows in ROWS:
            nbuf = rotation(rows, cols, 2)
            g = torch.Generator(device=dev).manual_seed(rows + cols)
            xs = [torch.randn(rows, cols, generator=g, device=dev).to(DT) for _ in range(nbuf)]
            rs = [(torch.randn(rows, cols, generator=g, device=dev) * 3).to(DT) for _ in range(nbuf)]
            w = (0.3 * torch.randn(cols, generator=g, device=dev)).to(DT)
            qa, sa = pq.add_gemma_rmsnorm_quantize(xs[0], rs[0], w, EPS)
            qb = pq.gemma_rmsnorm_quantize(rs[0] + xs[0], w, EPS)
            torch.cuda.synchronize()
            assert torch.equal(sa, rs[0] + xs[0]) and torch.equal(qa.int_data, qb.int_data) and torch.equal(qa.scale, qb.scale), f"{rows} x {cols}: K1ang and the pair differ"
            cands = [("K1ng", lambda i: pq.gemma_rmsnorm_quantize(xs[i % nbuf], w, EPS)),
                     ("K1n", lambda i: pq.rmsnorm_quantize(xs[i % nbuf], w, EPS)),
                     ("eager chain + K1", lambda i: pq.quantize(gemma_eager(xs[i % nbuf], w))),
                     ("K1ang", lambda i: pq.add_gemma_rmsnorm_quantize(xs[i % nbuf], rs[i % nbuf], w, EPS)),
                     ("add + eager chain + K1", lambda i: pq.quantize(gemma_eager(rs[i % nbuf] + xs[i % nbuf], w)))]
            reps = 2 * nbuf if rows >= 1024 else 64
            t = dict(zip((n for n, _ in cands), run(cands, reps, rounds)))
            n = rows * cols
            fed = "HBM-fed" if nbuf * n * 4 > 512e6 else "cache-resident: launch-bound"
            med = {k: float(np.median(v)) for k, v in t.items()}
            print(f"norm {rows} x {cols}  (rotation of {nbuf} x 2 x {n * 2 / 2**20:.2f} MiB inputs: {fed})")
            print(f"  K1ng                    {fmt(t['K1ng'])}   {(3 * n + 4 * rows) / med['K1ng'] / 1e6:5.2f} TB/s of its 3 B/elem   K1ng / K1n = x {med['K1ng'] / med['K1n']:.3f}")
            print(f"  K1n                     {fmt(t['K1n'])}   {(3 * n + 4 * rows) / med['K1n'] / 1e6:5.2f} TB/s of its 3 B/elem")
            print(f"  eager chain + K1        {fmt(t['eager chain + K1'])}   eager / K1ng = x {med['eager chain + K1'] / med['K1ng']:.2f}")
            print(f"  K1ang                   {fmt(t['K1ang'])}   {(7 * n + 4 * rows) / med['K1ang'] / 1e6:5.2f} TB/s of its 7 B/elem")
            print(f"  add + eager chain + K1  {fmt(t['add + eager chain + K1'])}   add + eager / K1ang = x {med['add + eager chain + K1'] / med['K1ang']:.2f}")
            del xs, rs, cands
            torch.cuda.empty_cache()
    print("# GeGLU: K1gg / K1s 1 launch, 5 B/elem; chain = F.gelu(g, approximate='tanh') * u + K1: 3 launches, 13 B/elem")
    for cols in INTERMEDIATE:
        for rows in ROWS:
            nbuf = rotation(rows, cols, 2)
            g = torch.Generator(device=dev).manual_seed(rows + cols)
            gs = [(torch.randn(rows, cols, generator=g, device=dev) * 2).to(DT) for _ in range(nbuf)]
            us = [torch.randn(rows, cols, generator=g, device=dev).to(DT) for _ in range(nbuf)]
            cands = [("K1gg", lambda i: pq.gelu_mul_quantize(gs[i % nbuf], us[i % nbuf])),
                     ("K1s", lambda i: pq.silu_mul_quantize(gs[i % nbuf], us[i % nbuf])),
                     ("gelu * u + K1", lambda i: pq.quantize(torch.nn.functional.gelu(gs[i % nbuf], approximate="tanh") * us[i % nbuf]))]
            reps = 2 * nbuf if rows >= 1024 else 64
            t = dict(zip((n for n, _ in cands), run(cands, reps, rounds)))
            n = rows * cols
            fed = "HBM-fed" if nbuf * n * 4 > 512e6 else "cache-resident: launch-bound"
            med = {k: float(np.median(v)) for k, v in t.items()}
            print(f"geglu {rows} x {cols}  (rotation of {nbuf} x 2 x {n * 2 / 2**20:.2f} MiB inputs: {fed})")
            print(f"  K1gg             {fmt(t['K1gg'])}   {(5 * n + 4 * rows) / med['K1gg'] / 1e6:5.2f} TB/s of its 5 B/elem   K1gg / K1s = x {med['K1gg'] / med['K1s']:.3f}")
            print(f"  K1s              {fmt(t['K1s'])}   {(5 * n + 4 * rows) / med['K1s'] / 1e6:5.2f} TB/s of its 5 B/elem")
            print(f"  gelu * u + K1    {fmt(t['gelu * u + K1'])}   {(13 * n + 4 * rows) / med['gelu * u + K1'] / 1e6:5.2f} TB/s of its 13 B/elem   chain / K1gg = x {med['gelu * u + K1'] / med['K1gg']:.2f}")
            del gs, us, cands
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
