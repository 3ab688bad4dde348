"""Dev tool (GPU box): the scaled-residual kernels K1ma (scaled_add_rmsnorm_quantize) and K1mo (scaled_add) against what they replace and what they stand next to, bf16,
at hidden 2048 (Granite-3 2B) and 4096 (8B), 4096, 32 and 1 rows.  Per shape, K1ma against
  (a) what a Granite layer runs without the switch: torch multiply + torch add + K1n (3 launches, 4 + 6 + 3 = 13 B/elem);
  (b) torch multiply + K1a (2 launches, 4 + 7 = 11 B/elem);
  K1a (add_rmsnorm_quantize) at the same shape: the same 7 B/elem without the multiply and its rounding — the floor to compare against;
and K1mo (6 B/elem) against the torch multiply + torch add it replaces at the end of a chain.
Every candidate of a shape is captured into a hipGraph and the graphs are replayed in turn, round by round, in ONE process.  Every launch of a graph walks a rotation
of input buffers larger than the 256-MiB Infinity Cache, so the large shapes are fed from HBM (the small ones measure launches, not bytes).  Changes no device setting.
usage: python tools/scaled_addnorm_bench.py [--quick] [> profiles/r23_granite_residual_bench.txt]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.addlnorm_bench import fmt  # noqa: E402
from tools.gemma_bench import rotation, run  # noqa: E402

HIDDEN = (2048, 4096)
ROWS = (4096, 32, 1)
EPS = 1e-6
M = 0.22
DT = torch.bfloat16


def verdict(t, a, b):
    """a against b: the ratio of the medians, and whether the [min .. max] ranges overlap (then the two count as equal)"""
    ratio = float(np.median(t[a])) / float(np.median(t[b]))
    overlap = min(t[a]) <= max(t[b]) and min(t[b]) <= max(t[a])
    return f"x {ratio:.3f}" + (" (ranges overlap)" if overlap else " (ranges disjoint)")


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    import protoquant_amd as pq
    rounds = 6 if "--quick" in sys.argv else 20
    dev = torch.device("cuda:0")
    print("# tools/scaled_addnorm_bench.py  (one MI355X, one process, bf16, residual_multiplier 0.22)")
    print(f"# {torch.cuda.get_device_name(0)}; {time.strftime('%Y-%m-%d')}; medians [min .. max] per call of hipGraph replays, the candidates of a shape replayed in turn")
    print("# K1ma 1 launch, 7 B/elem; (a) torch mul + torch add + K1n: 3 launches, 13 B/elem; (b) torch mul + K1a: 2 launches, 11 B/elem; K1a 1 launch, 7 B/elem")
    print("# K1mo 1 launch, 6 B/elem; mul + add = torch mul + torch add: 2 launches, 10 B/elem")
    for cols in HIDDEN:
        for rows in ROWS:
            nbuf = rotation(rows, cols, 2)
            g = torch.Generator(device=dev).manual_seed(rows + cols)
            xs = [(torch.randn(rows, cols, generator=g, device=dev) * 4).to(DT) for _ in range(nbuf)]
            rs = [torch.randn(rows, cols, generator=g, device=dev).to(DT) for _ in range(nbuf)]
            w = (1 + 0.1 * torch.randn(cols, generator=g, device=dev)).to(DT)
            # bit for bit first
            qa, sa = pq.scaled_add_rmsnorm_quantize(xs[0], rs[0], M, w, EPS)
            sb = rs[0] + xs[0] * M
            qb = pq.rmsnorm_quantize(sb, w, EPS)
            torch.cuda.synchronize()
            assert torch.equal(sa, sb) and torch.equal(qa.int_data, qb.int_data) and torch.equal(qa.scale, qb.scale), f"{rows} x {cols}: K1ma and the eager chain differ"
            assert torch.equal(pq.scaled_add(xs[0], rs[0], M), sb), f"{rows} x {cols}: K1mo and the eager chain differ"
            cands = [("K1ma", lambda i: pq.scaled_add_rmsnorm_quantize(xs[i % nbuf], rs[i % nbuf], M, w, EPS)),
                     ("(a) mul + add + K1n", lambda i: pq.rmsnorm_quantize(rs[i % nbuf] + xs[i % nbuf] * M, w, EPS)),
                     ("(b) mul + K1a", lambda i: pq.add_rmsnorm_quantize(xs[i % nbuf] * M, rs[i % nbuf], w, EPS)),
                     ("K1a", lambda i: pq.add_rmsnorm_quantize(xs[i % nbuf], rs[i % nbuf], w, EPS)),
                     ("K1mo", lambda i: pq.scaled_add(xs[i % nbuf], rs[i % nbuf], M)),
                     ("mul + add", lambda i: rs[i % nbuf] + xs[i % nbuf] * M)]
            reps = 2 * nbuf if rows >= 1024 else 64
            t = dict(zip((n for n, _ in cands), run(cands, reps, rounds)))
            n = rows * cols
            fed = "HBM-fed" if nbuf * n * 4 > 512e6 else "cache-resident: launch-bound"
            med = {k: float(np.median(v)) for k, v in t.items()}
            print(f"scaled add {rows} x {cols}  (rotation of {nbuf} x 2 x {n * 2 / 2**20:.2f} MiB inputs: {fed})")
            print(f"  K1ma                 {fmt(t['K1ma'])}   {(7 * n + 4 * rows) / med['K1ma'] / 1e6:5.2f} TB/s of its 7 B/elem   K1ma / K1a = {verdict(t, 'K1ma', 'K1a')}")
            print(f"  (a) mul + add + K1n  {fmt(t['(a) mul + add + K1n'])}   (a) / K1ma = {verdict(t, '(a) mul + add + K1n', 'K1ma')}")
            print(f"  (b) mul + K1a        {fmt(t['(b) mul + K1a'])}   (b) / K1ma = {verdict(t, '(b) mul + K1a', 'K1ma')}")
            print(f"  K1a                  {fmt(t['K1a'])}   {(7 * n + 4 * rows) / med['K1a'] / 1e6:5.2f} TB/s of its 7 B/elem")
            print(f"  K1mo                 {fmt(t['K1mo'])}   {6 * n / med['K1mo'] / 1e6:5.2f} TB/s of its 6 B/elem")
            print(f"  mul + add            {fmt(t['mul + add'])}   mul + add / K1mo = {verdict(t, 'mul + add', 'K1mo')}")
            del xs, rs, cands
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
