"""Dev tool (GPU box): the sandwich kernels K1pang (gemma_postnorm_add_rmsnorm_quantize) and K1pa (gemma_postnorm_add) against what they replace and what they stand
next to, bf16, at hidden 2304 / 3584 / 4608 (Gemma-2 2B / 9B / 27B) and 4096, 32 and 1 rows.  Per shape, K1pang against
  (a) what runs without the switch: transformers' eager GemmaRMSNorm chain on the sublayer output + a torch add + K1ng;
  (b) the library composition of its docstring: K1ng with return_h + a torch add + K1ng;
  (c) K1ang (add_gemma_rmsnorm_quantize) at the same shape: the same 7 B/elem — the floor to compare against;
and K1pa against the eager chain + the torch add.
Every candidate of a shape is captured into a hipGraph and the graphs are replayed in turn, round by round, in ONE process.  Every launch of a graph walks a rotation
of input buffers larger than the 256-MiB Infinity Cache, so the large shapes are fed from HBM (the small ones measure launches, not bytes).  Changes no device setting.
usage: python tools/gemma_postnorm_bench.py [--quick] [> profiles/r19_gemma_postnorm_bench.txt]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.addlnorm_bench import fmt  # noqa: E402
from tools.gemma_bench import gemma_eager, rotation, run  # noqa: E402

HIDDEN = (2304, 3584, 4608)
ROWS = (4096, 32, 1)
EPS = 1e-6
DT = torch.bfloat16


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    import protoquant_amd as pq
    rounds = 6 if "--quick" in sys.argv else 20
    dev = torch.device("cuda:0")
    print("# tools/gemma_postnorm_bench.py  (one MI355X, one process, bf16)")
    print(f"# {torch.cuda.get_device_name(0)}; {time.strftime('%Y-%m-%d')}; medians [min .. max] per call of hipGraph replays, the candidates of a shape replayed in turn")
    print("# K1pang 1 launch, 7 B/elem; (a) eager post-norm chain + torch add + K1ng; (b) K1ng with h + torch add + K1ng: 3 launches, 5 + 6 + 3 = 14 B/elem; (c) K1ang 1 launch, 7 B/elem")
    print("# K1pa 1 launch, 6 B/elem; eager + add = the eager post-norm chain + torch add")
    for cols in HIDDEN:
        for rows in ROWS:
            nbuf = rotation(rows, cols, 2)
            g = torch.Generator(device=dev).manual_seed(rows + cols)
            xs = [torch.randn(rows, cols, generator=g, device=dev).to(DT) for _ in range(nbuf)]
            rs = [(torch.randn(rows, cols, generator=g, device=dev) * 3).to(DT) for _ in range(nbuf)]
            pw = (0.3 * torch.randn(cols, generator=g, device=dev)).to(DT)
            w = (0.3 * torch.randn(cols, generator=g, device=dev)).to(DT)

            def composition(i):
                p = pq.gemma_rmsnorm_quantize(xs[i % nbuf], pw, EPS, return_h=True)[1]
                return pq.gemma_rmsnorm_quantize(rs[i % nbuf] + p, w, EPS)
            qa, sa = pq.gemma_postnorm_add_rmsnorm_quantize(xs[0], pw, rs[0], w, EPS, EPS)
            qb = composition(0)
            sb = pq.gemma_postnorm_add(xs[0], pw, rs[0], EPS)
            torch.cuda.synchronize()
            assert torch.equal(sa, sb) and torch.equal(qa.int_data, qb.int_data) and torch.equal(qa.scale, qb.scale), f"{rows} x {cols}: K1pang and the composition differ"
            cands = [("K1pang", lambda i: pq.gemma_postnorm_add_rmsnorm_quantize(xs[i % nbuf], pw, rs[i % nbuf], w, EPS, EPS)),
                     ("(a) eager + add + K1ng", lambda i: pq.gemma_rmsnorm_quantize(rs[i % nbuf] + gemma_eager(xs[i % nbuf], pw), w, EPS)),
                     ("(b) K1ng + add + K1ng", composition),
                     ("(c) K1ang", lambda i: pq.add_gemma_rmsnorm_quantize(xs[i % nbuf], rs[i % nbuf], w, EPS)),
                     ("K1pa", lambda i: pq.gemma_postnorm_add(xs[i % nbuf], pw, rs[i % nbuf], EPS)),
                     ("eager + add", lambda i: rs[i % nbuf] + gemma_eager(xs[i % nbuf], pw))]
            reps = 2 * nbuf if rows >= 1024 else 64
            t = dict(zip((n for n, _ in cands), run(cands, reps, rounds)))
            n = rows * cols
            fed = "HBM-fed" if nbuf * n * 4 > 512e6 else "cache-resident: launch-bound"
            med = {k: float(np.median(v)) for k, v in t.items()}
            print(f"sandwich {rows} x {cols}  (rotation of {nbuf} x 2 x {n * 2 / 2**20:.2f} MiB inputs: {fed})")
            print(f"  K1pang                  {fmt(t['K1pang'])}   {(7 * n + 4 * rows) / med['K1pang'] / 1e6:5.2f} TB/s of its 7 B/elem   K1pang / K1ang = x {med['K1pang'] / med['(c) K1ang']:.3f}")
            print(f"  (a) eager + add + K1ng  {fmt(t['(a) eager + add + K1ng'])}   (a) / K1pang = x {med['(a) eager + add + K1ng'] / med['K1pang']:.2f}")
            print(f"  (b) K1ng + add + K1ng   {fmt(t['(b) K1ng + add + K1ng'])}   (b) / K1pang = x {med['(b) K1ng + add + K1ng'] / med['K1pang']:.2f}")
            print(f"  (c) K1ang               {fmt(t['(c) K1ang'])}   {(7 * n + 4 * rows) / med['(c) K1ang'] / 1e6:5.2f} TB/s of its 7 B/elem")
            print(f"  K1pa                    {fmt(t['K1pa'])}   {6 * n / med['K1pa'] / 1e6:5.2f} TB/s of its 6 B/elem")
            print(f"  eager + add             {fmt(t['eager + add'])}   eager + add / K1pa = x {med['eager + add'] / med['K1pa']:.2f}")
            del xs, rs, cands
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
