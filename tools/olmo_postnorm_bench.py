"""Dev tool (GPU box): the post-norm kernels K1oq (olmo_postnorm_add_quantize), K1oa (olmo_postnorm_add) and K1on (olmo_rmsnorm) against what they replace and what
they stand next to, bf16, at hidden 4096 and 5120 (OLMo-2 7B / 13B) and 4096, 32 and 1 rows.  Per shape, K1oq against
  (a) what runs without the switch: transformers' eager Olmo2RMSNorm chain on the sublayer output + a torch add + K1;
  (b) the library composition of its docstring: K1on + a torch add + K1;
  (c) K1pang (gemma_postnorm_add_rmsnorm_quantize) at the same shape: the same 7 B/elem and strictly more work (a second row reduction, a second weight row);
K1oa against the eager chain + the torch add, and K1on against the eager chain.
Every candidate of a shape is captured into a hipGraph and the graphs are replayed in turn, round by round, in ONE process.  Every launch of a graph walks a rotation
of input buffers larger than the 256-MiB Infinity Cache, so the large shapes are fed from HBM (the small ones measure launches, not bytes).  Changes no device setting.
usage: python tools/olmo_postnorm_bench.py [--quick] [> profiles/r21_olmo_postnorm_bench.txt]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.addlnorm_bench import fmt  # noqa: E402
from tools.gemma_bench import rotation, run  # noqa: E402

HIDDEN = (4096, 5120)
ROWS = (4096, 32, 1)
EPS = 1e-6
DT = torch.bfloat16


def olmo_eager(x, w):
    """transformers' Olmo2RMSNorm.forward, op for op"""
    h = x.to(torch.float32)
    variance = h.pow(2).mean(-1, keepdim=True)
    h = h * torch.rsqrt(variance + EPS)
    return (w * h).to(x.dtype)


def overlap(a, b):
    """do the [min .. max] ranges of two lists of timings overlap?"""
    return "overlap" if min(a) <= max(b) and min(b) <= max(a) else "disjoint"


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    import protoquant_amd as pq
    rounds = 6 if "--quick" in sys.argv else 20
    dev = torch.device("cuda:0")
    print("# tools/olmo_postnorm_bench.py  (one MI355X, one process, bf16)")
    print(f"# {torch.cuda.get_device_name(0)}; {time.strftime('%Y-%m-%d')}; medians [min .. max] per call of hipGraph replays, the candidates of a shape replayed in turn")
    print("# K1oq 1 launch, 7 B/elem; (a) eager norm chain + torch add + K1; (b) K1on + torch add + K1: 3 launches, 4 + 6 + 3 = 13 B/elem; (c) K1pang 1 launch, 7 B/elem")
    print("# K1oa 1 launch, 6 B/elem against the eager chain + torch add; K1on 1 launch, 4 B/elem against the eager chain")
    slower = []
    for cols in HIDDEN:
        for rows in ROWS:
            nbuf = rotation(rows, cols, 2)
            g = torch.Generator(device=dev).manual_seed(rows + cols)
            xs = [torch.randn(rows, cols, generator=g, device=dev).to(DT) for _ in range(nbuf)]
            rs = [(torch.randn(rows, cols, generator=g, device=dev) * 3).to(DT) for _ in range(nbuf)]
            pw = (1.0 + 0.3 * torch.randn(cols, generator=g, device=dev)).to(DT)
            w = (0.3 * torch.randn(cols, generator=g, device=dev)).to(DT)

            def composition(i):
                return pq.quantize(rs[i % nbuf] + pq.olmo_rmsnorm(xs[i % nbuf], pw, EPS))
            qa, sa = pq.olmo_postnorm_add_quantize(xs[0], pw, rs[0], EPS)
            qb = composition(0)
            sb = pq.olmo_postnorm_add(xs[0], pw, rs[0], EPS)
            torch.cuda.synchronize()
            assert torch.equal(sa, sb) and torch.equal(qa.int_data, qb.int_data) and torch.equal(qa.scale, qb.scale), f"{rows} x {cols}: K1oq and the composition differ"
            cands = [("K1oq", lambda i: pq.olmo_postnorm_add_quantize(xs[i % nbuf], pw, rs[i % nbuf], EPS)),
                     ("(a)", lambda i: pq.quantize(rs[i % nbuf] + olmo_eager(xs[i % nbuf], pw))),
                     ("(b)", composition),
                     ("(c)", lambda i: pq.gemma_postnorm_add_rmsnorm_quantize(xs[i % nbuf], pw, rs[i % nbuf], w, EPS, EPS)),
                     ("K1oa", lambda i: pq.olmo_postnorm_add(xs[i % nbuf], pw, rs[i % nbuf], EPS)),
                     ("eager + add", lambda i: rs[i % nbuf] + olmo_eager(xs[i % nbuf], pw)),
                     ("K1on", lambda i: pq.olmo_rmsnorm(xs[i % nbuf], pw, EPS)),
                     ("eager", lambda i: olmo_eager(xs[i % nbuf], pw))]
            reps = 2 * nbuf if rows >= 1024 else 64
            t = dict(zip((n for n, _ in cands), run(cands, reps, rounds)))
            n = rows * cols
            fed = "HBM-fed" if nbuf * n * 4 > 512e6 else "cache-resident: launch-bound"
            med = {k: float(np.median(v)) for k, v in t.items()}
            print(f"post-norm {rows} x {cols}  (rotation of {nbuf} x 2 x {n * 2 / 2**20:.2f} MiB inputs: {fed})")
            print(f"  K1oq                   {fmt(t['K1oq'])}   {(7 * n + 4 * rows) / med['K1oq'] / 1e6:5.2f} TB/s of its 7 B/elem   K1oq / K1pang = x {med['K1oq'] / med['(c)']:.3f} "
                  f"(ranges {overlap(t['K1oq'], t['(c)'])})")
            print(f"  (a) eager + add + K1   {fmt(t['(a)'])}   (a) / K1oq = x {med['(a)'] / med['K1oq']:.2f}")
            print(f"  (b) K1on + add + K1    {fmt(t['(b)'])}   (b) / K1oq = x {med['(b)'] / med['K1oq']:.2f}")
            print(f"  (c) K1pang             {fmt(t['(c)'])}   {(7 * n + 4 * rows) / med['(c)'] / 1e6:5.2f} TB/s of its 7 B/elem")
            print(f"  K1oa                   {fmt(t['K1oa'])}   {6 * n / med['K1oa'] / 1e6:5.2f} TB/s of its 6 B/elem")
            print(f"  eager + add            {fmt(t['eager + add'])}   eager + add / K1oa = x {med['eager + add'] / med['K1oa']:.2f}")
            print(f"  K1on                   {fmt(t['K1on'])}   {4 * n / med['K1on'] / 1e6:5.2f} TB/s of its 4 B/elem")
            print(f"  eager                  {fmt(t['eager'])}   eager / K1on = x {med['eager'] / med['K1on']:.2f}")
            for fused, unfused in (("K1oq", "(a)"), ("K1oq", "(b)"), ("K1oa", "eager + add"), ("K1on", "eager")):
                if med[fused] > med[unfused]:
                    slower.append(f"{rows} x {cols}: {fused} {med[fused]:.2f} us > {unfused} {med[unfused]:.2f} us")
            del xs, rs, cands
            torch.cuda.empty_cache()
    print("# shapes at which a fused form is slower than what it replaces: " + ("; ".join(slower) if slower else "none"))


if __name__ == "__main__":
    main()
