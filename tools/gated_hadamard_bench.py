"""Dev tool (GPU box): K1gh (gated_hadamard_quantize) — silu * mul, the block Hadamard rotation and the per-token int8 quantisation in one launch — against what a rotated
down_proj ran before it and against its floor, bf16, at 4096, 32 and 1 rows of (cols, block) = (11008, 256), (14336, 2048), (8192, 4096).  g and u are the halves of one
[rows, 2 cols] buffer (a fused gate+up output).  Per shape:
  (a)  F.silu(g) * u in torch, then K1h: 3 launches, about 13 B/elem — the path of a rotated down_proj before K1gh;
  (b)  the library composition: K1s with return_h, then K1h: 2 launches, 11 B/elem;
  (c)  gated_hadamard_quantize (K1gh): 1 launch, 5 B/elem;
  (d)  K1s alone (silu_mul_quantize): the floor, it moves the same 5 B/elem without the rotation.
Every candidate of a shape is captured into a hipGraph and the graphs are replayed in turn, round by round, in ONE process; every launch of a graph walks a rotation of
inputs larger than the 256-MiB Infinity Cache, so the large shapes are fed from HBM (the small ones measure launches, not bytes).  Changes no device setting.
usage: python tools/gated_hadamard_bench.py [--quick] [--out profiles/r28_gated_hadamard_bench.txt]"""
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.addlnorm_bench import fmt  # noqa: E402
from tools.gemma_bench import rotation, run  # noqa: E402

SHAPES = ((11008, 256), (14336, 2048), (8192, 4096))
ROWS = (4096, 32, 1)
DT = torch.bfloat16


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    import protoquant_amd as pq
    rounds = 6 if "--quick" in sys.argv else 20
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "r28_gated_hadamard_bench.txt")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("# tools/gated_hadamard_bench.py  (one MI355X, one process, bf16; g and u: the halves of one [rows, 2 cols] buffer)")
    say(f"# {torch.cuda.get_device_name(0)}; {time.strftime('%Y-%m-%d')}; medians [min .. max] per call of hipGraph replays, the candidates of a shape replayed in turn")
    say("# (a) F.silu(g) * u in torch, then K1h: 3 launches, ~13 B/elem; (b) K1s with return_h, then K1h: 2 launches, 11 B/elem; (c) gated_hadamard_quantize (K1gh): 1 launch,")
    say("# 5 B/elem; (d) K1s alone: the floor, 5 B/elem")
    slower, overlap = [], []
    for cols, block in SHAPES:
        for rows in ROWS:
            nbuf = rotation(rows, cols, 2)
            gen = torch.Generator(device=dev).manual_seed(rows + cols)
            gus = [(torch.randn(rows, 2 * cols, generator=gen, device=dev) * 2).to(DT) for _ in range(nbuf)]
            gs, us = [t[:, :cols] for t in gus], [t[:, cols:] for t in gus]
            qc, hc = pq.gated_hadamard_quantize(gs[0], us[0], "silu", block, return_h=True)
            qb, hb = pq.hadamard_quantize(pq.silu_mul_quantize(gs[0], us[0], return_h=True)[1], block, return_h=True)
            torch.cuda.synchronize()
            assert torch.equal(qc.int_data, qb.int_data) and torch.equal(qc.scale, qb.scale) and torch.equal(hc.view(torch.int16), hb.view(torch.int16)), "K1gh differs from K1s + K1h"
            cands = [("(a)", lambda i: pq.hadamard_quantize(F.silu(gs[i % nbuf]) * us[i % nbuf], block)),
                     ("(b)", lambda i: pq.hadamard_quantize(pq.silu_mul_quantize(gs[i % nbuf], us[i % nbuf], return_h=True)[1], block)),
                     ("(c)", lambda i: pq.gated_hadamard_quantize(gs[i % nbuf], us[i % nbuf], "silu", block)),
                     ("(d)", lambda i: pq.silu_mul_quantize(gs[i % nbuf], us[i % nbuf]))]
            reps = 2 * nbuf if rows >= 1024 else 64
            t = dict(zip((n for n, _ in cands), run(cands, reps, rounds)))
            med = {k: float(np.median(v)) for k, v in t.items()}
            n = rows * cols
            fed = "HBM-fed" if nbuf * n * 4 > 512e6 else "cache-resident: launch-bound"
            say(f"{rows} x {cols}, block {block}  ({n * 4 / 2**20:.2f} MiB of g and u, rotation of {nbuf}: {fed})")
            say(f"  (a) torch silu * u + K1h   {fmt(t['(a)'])}   (a) / (c) = x {med['(a)'] / med['(c)']:.2f}")
            say(f"  (b) K1s (h) + K1h          {fmt(t['(b)'])}   (b) / (c) = x {med['(b)'] / med['(c)']:.2f}")
            say(f"  (c) K1gh                   {fmt(t['(c)'])}   {5 * n / med['(c)'] / 1e6:5.2f} TB/s of its 5 B/elem")
            say(f"  (d) K1s alone              {fmt(t['(d)'])}   (c) / (d) = x {med['(c)'] / med['(d)']:.2f} (the price of the rotation)")
            for other in ("(a)", "(b)"):
                if med["(c)"] > med[other]:
                    slower.append(f"{rows} x {cols} block {block}: (c) {med['(c)']:.2f} us > {other} {med[other]:.2f} us")
            if rows == 4096 and not max(t["(c)"]) < min(t["(a)"]):
                overlap.append(f"{rows} x {cols} block {block}")
            del cands, gus, gs, us
            torch.cuda.empty_cache()
    say("# shapes at which (c) is slower than (a) or (b): " + ("; ".join(slower) if slower else "none"))
    say("# 4096-row shapes at which the ranges of (c) and (a) are not disjoint with (c) below: " + ("; ".join(overlap) if overlap else "none"))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
