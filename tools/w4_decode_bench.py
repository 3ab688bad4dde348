"""Dev tool (GPU box): the decode GEMM on int4 weights (pq_qlinear_w4, gemm_w4_stream.hip) against the int8 path it halves the bytes of, bf16 out, at M in {1, 16, 64} x
(N, K) in {4096^2, 14336 x 4096, 4096 x 14336, 28672 x 4096}.  Per shape:
  (a)  qlinear_s8 on the int8 weight: the yardstick (the weight-streaming int8 kernel), N K weight bytes;
  (b)  qlinear_w4: one launch on the packed weight, N K (1/2 + 1/128) = 0.508 N K weight bytes — the byte ratio is the floor of (b) / (a);
  (c)  qlinear_w4(stream_rows=0): w4_expand into the workspace, then (a)'s GEMM on it: 2 launches, what `stream_rows = 0` costs at decode.
Every candidate of a shape is captured into a hipGraph and the graphs are replayed in turn, round by round, in ONE process.  "rotated": every launch of a graph takes the
next of a rotation of distinct weight buffers whose PACKED bytes exceed 600 MB, so every candidate is fed from HBM (a 4096^2 int4 matrix is 8 MiB and would sit in the
last-level cache).  "resident": one weight buffer, the method of tools/skinny_bench.py and profiles/r29_stream_body_ab.txt — its column (a) is comparable with that file.
Changes no device setting.   usage: python tools/w4_decode_bench.py [--quick] [--out profiles/r30_w4_decode_bench.txt]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.addlnorm_bench import fmt, graph_of, time_graphs  # noqa: E402

SHAPES = ((4096, 4096), (14336, 4096), (4096, 14336), (28672, 4096))
ROWS = (1, 16, 64)


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    import protoquant_amd as pq
    rounds = 5 if "--quick" in sys.argv else 15
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "r30_w4_decode_bench.txt")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("# tools/w4_decode_bench.py  (one MI355X, one process, bf16 out)")
    say(f"# {torch.cuda.get_device_name(0)}; {time.strftime('%Y-%m-%d')}; medians [min .. max] per call of hipGraph replays, the candidates of a shape replayed in turn")
    say("# (a) qlinear_s8, int8 weight: the yardstick; (b) qlinear_w4, packed weight, 1 launch; (c) w4_expand + qlinear_s8 (stream_rows = 0), 2 launches")
    not_faster = []
    for N, K in SHAPES:
        nbuf = max(3, int(np.ceil(600e6 / (N * K / 2))))
        g = torch.Generator(device=dev).manual_seed(N + K)
        wqs = [torch.randint(-127, 128, (N, K), dtype=torch.int8, device=dev, generator=g) for _ in range(nbuf)]
        packed = [pq.w4_pack(w) for w in wqs]
        ws = torch.rand(N, device=dev, generator=g) * 1e-3 + 1e-5
        for M in ROWS:
            xq = torch.randint(-127, 128, (M, K), dtype=torch.int8, device=dev, generator=g)
            xs = torch.rand(M, device=dev, generator=g) * 1e-2 + 1e-3
            ys = [torch.empty((M, N), dtype=torch.bfloat16, device=dev) for _ in range(3)]
            same = torch.equal(pq.qlinear_w4(xq, xs, *packed[0], ws, None, torch.bfloat16), pq.qlinear_w4(xq, xs, *packed[0], ws, None, torch.bfloat16, stream_rows=0))
            assert same, f"{M} x {N} x {K}: the streaming kernel and expand + int8 differ"
            for mode, nb in (("rotated", nbuf), ("resident", 1)):
                cands = [("(a)", lambda i: pq.qlinear_s8(xq, xs, wqs[i % nb], ws, None, torch.bfloat16, out=ys[0])),
                         ("(b)", lambda i: pq.qlinear_w4(xq, xs, *packed[i % nb], ws, None, torch.bfloat16, out=ys[1])),
                         ("(c)", lambda i: pq.qlinear_w4(xq, xs, *packed[i % nb], ws, None, torch.bfloat16, out=ys[2], stream_rows=0))]
                reps = max(200, 2 * nb)          # (a replay's own cost, a few us, is spread over at least 200 launches)
                graphs = [graph_of(fn, reps) for _, fn in cands]
                t = dict(zip("abc", time_graphs([gr for gr, _ in graphs], reps, rounds)))
                del graphs
                med = {k: float(np.median(v)) for k, v in t.items()}
                fed = f"rotation of {nb} weights, {nb * N * K / 2 / 1e6:.0f} MB packed: HBM-fed" if nb > 1 else "one weight: cache-resident"
                say(f"M={M} N={N} K={K}  {mode} ({fed})")
                say(f"  (a) int8 qlinear_s8     {fmt(t['a'])}   {N * K / med['a'] / 1e6:5.2f} TB/s of its weight bytes")
                say(f"  (b) qlinear_w4          {fmt(t['b'])}   {N * K * 0.5078125 / med['b'] / 1e6:5.2f} TB/s of its weight bytes; (b) / (a) = {med['b'] / med['a']:.3f} (byte floor 0.508)")
                say(f"  (c) expand + qlinear_s8 {fmt(t['c'])}   (c) / (a) = {med['c'] / med['a']:.3f}")
                if min(t["a"]) <= max(t["b"]):
                    not_faster.append(f"M={M} N={N} K={K} {mode}: (b) {fmt(t['b']).strip()} against (a) {fmt(t['a']).strip()}")
        del wqs, packed
        torch.cuda.empty_cache()
    say("# shapes at which (b) is not faster than (a) (ranges overlapping or inverted): " + ("; ".join(not_faster) if not_faster else "none"))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
