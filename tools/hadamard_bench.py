"""Dev tool (GPU box): K1h (hadamard_quantize), the block Hadamard rotation fused with the per-token int8 quantisation, against its floor and against what it replaces,
bf16, at 4096, 32 and 1 rows of (cols, block) = (4096, 4096), (11008, 256), (14336, 2048), (8192, 4096).  Per shape:
  (a)  K1 alone (quantize) on the same rows: the floor, it moves the same 3 B/elem;
  (b)  the torch composition (x.view(-1, nb, B) @ H).view_as(x) — a bf16 GEMM against the normalised Hadamard matrix — followed by K1: 2 launches, 7 B/elem;
  (c)  hadamard_quantize: 1 launch, 3 B/elem.
Every candidate of a shape is captured into a hipGraph and the graphs are replayed in turn, round by round, in ONE process; every launch of a graph walks a rotation of
inputs larger than the 256-MiB Infinity Cache, so the large shapes are fed from HBM (the small ones measure launches, not bytes).  Changes no device setting.
usage: python tools/hadamard_bench.py [--quick] [--out profiles/r27_hadamard_bench.txt]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.addlnorm_bench import fmt  # noqa: E402
from tools.gemma_bench import rotation, run  # noqa: E402

SHAPES = ((4096, 4096), (11008, 256), (14336, 2048), (8192, 4096))
ROWS = (4096, 32, 1)
DT = torch.bfloat16


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    import protoquant_amd as pq
    rounds = 6 if "--quick" in sys.argv else 20
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "r27_hadamard_bench.txt")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("# tools/hadamard_bench.py  (one MI355X, one process, bf16)")
    say(f"# {torch.cuda.get_device_name(0)}; {time.strftime('%Y-%m-%d')}; medians [min .. max] per call of hipGraph replays, the candidates of a shape replayed in turn")
    say("# (a) K1 alone, 3 B/elem: the floor; (b) x.view(-1, nb, B) @ H, then K1: 2 launches, 7 B/elem; (c) hadamard_quantize (K1h): 1 launch, 3 B/elem")
    slower = []
    for cols, block in SHAPES:
        h = torch.ones(1, 1, device=dev)
        while h.shape[0] < block:
            h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
        hm = (h / block ** 0.5).to(DT)
        for rows in ROWS:
            nbuf = rotation(rows, cols, 1)
            g = torch.Generator(device=dev).manual_seed(rows + cols)
            xs = [torch.randn(rows, cols, generator=g, device=dev).to(DT) for _ in range(nbuf)]
            cands = [("(a)", lambda i: pq.quantize(xs[i % nbuf])), ("(b)", lambda i: pq.quantize((xs[i % nbuf].view(rows, -1, block) @ hm).view(rows, cols))),
                     ("(c)", lambda i: pq.hadamard_quantize(xs[i % nbuf], block))]
            reps = 2 * nbuf if rows >= 1024 else 64
            t = dict(zip((n for n, _ in cands), run(cands, reps, rounds)))
            med = {k: float(np.median(v)) for k, v in t.items()}
            n = rows * cols
            fed = "HBM-fed" if nbuf * n * 2 > 512e6 else "cache-resident: launch-bound"
            say(f"{rows} x {cols}, block {block}  ({n * 2 / 2**20:.2f} MiB, rotation of {nbuf}: {fed})")
            say(f"  (a) K1 alone           {fmt(t['(a)'])}   {3 * n / med['(a)'] / 1e6:5.2f} TB/s of its 3 B/elem")
            say(f"  (b) torch @ H + K1     {fmt(t['(b)'])}   (b) / (c) = x {med['(b)'] / med['(c)']:.2f}")
            say(f"  (c) hadamard_quantize  {fmt(t['(c)'])}   {3 * n / med['(c)'] / 1e6:5.2f} TB/s of its 3 B/elem; (c) / (a) = x {med['(c)'] / med['(a)']:.2f} (the price of the rotation)")
            if med["(c)"] > med["(b)"]:
                slower.append(f"{rows} x {cols} block {block}: (c) {med['(c)']:.2f} us > (b) {med['(b)']:.2f} us")
            del cands, xs
            torch.cuda.empty_cache()
    say("# shapes at which (c) is slower than (b): " + ("; ".join(slower) if slower else "none"))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
