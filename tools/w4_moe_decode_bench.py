"""Dev tool (GPU box): the expert GEMMs of a mixture-of-experts DECODE step on int4 weights (pq.qlinear_w4_grouped, gemm_w4_grouped_stream.hip) against the int8
grouped streaming kernel they halve the bytes of, bf16 out.  Layers: Mixtral-like E = 8, top-2, 28672 x 4096 (gate + up) and 4096 x 14336 (down); 128 experts, top-8,
1536 x 2048 and 2048 x 768; each at T = 1, 4, 8, 32 tokens while M_total = T * top_k <= 64.  Per shape:
  (a)  qlinear_s8_grouped_stream on the int8 [E, N, K] weight: the yardstick, N K bytes per live expert;
  (b)  qlinear_w4_grouped: one launch on the packed weights, 0.508 N K bytes per live expert — the byte ratio is the floor of (b) / (a);
  (c)  qlinear_w4_grouped(stream_rows=0): ALL E experts expanded into the workspace, then the int8 tiles — what `stream_rows = 0` costs at decode.
Every candidate of a shape is captured into a hipGraph and the graphs are replayed in turn, round by round, in ONE process.  Launch i of a graph takes the next L =
min(T top_k, E) experts of a cyclic walk over `nstack` distinct weight stacks (rows spread evenly over those L experts; the routing is device data, so the walk only
changes offsets): an expert is read again after ALL nstack * E experts were, and nstack is chosen so that their PACKED bytes exceed 600 MB — no expert is
cache-resident for any candidate.  Even routing is the kindest case for every candidate alike; skewed routings are not measured here.
Changes no device setting.   usage: python tools/w4_moe_decode_bench.py [--quick] [--out profiles/r31_w4_moe_decode_bench.txt]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.addlnorm_bench import fmt, graph_of, time_graphs  # noqa: E402

LAYERS = (("Mixtral-like", 8, 2, ((28672, 4096), (4096, 14336))), ("128 experts", 128, 8, ((1536, 2048), (2048, 768))))
TOKENS = (1, 4, 8, 32)


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    import protoquant_amd as pq
    rounds = 5 if "--quick" in sys.argv else 15
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "r31_w4_moe_decode_bench.txt")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("# tools/w4_moe_decode_bench.py  (one MI355X, one process, bf16 out)")
    say(f"# {torch.cuda.get_device_name(0)}; {time.strftime('%Y-%m-%d')}; medians [min .. max] per call of hipGraph replays, the candidates of a shape replayed in turn")
    say("# (a) qlinear_s8_grouped_stream, int8 experts: the yardstick; (b) qlinear_w4_grouped, packed experts, 1 launch; (c) stream_rows = 0: expand all experts + int8 tiles")
    not_faster = []
    for name, E, top_k, shapes in LAYERS:
        for N, K in shapes:
            nstack = max(3, int(np.ceil(600e6 / (E * N * K / 2))))
            g = torch.Generator(device=dev).manual_seed(N + K)
            stacks = [pq.GroupedQLinear._from_parts(torch.randint(-127, 128, (E, N, K), dtype=torch.int8, device=dev, generator=g),
                                                    torch.rand((E, N), device=dev, generator=g) * 1e-3 + 1e-5, None) for _ in range(nstack)]
            packed = [pq.GroupedQLinearW4.from_grouped(m) for m in stacks]
            for T in TOKENS:
                M = T * top_k
                if M > 64:
                    continue
                L = min(M, E)
                walks = E // L                                                 # launches that walk one stack once
                offs = []
                for s in range(walks):                                         # rows spread evenly over experts s L .. s L + L - 1
                    c = np.zeros(E, np.int64)
                    c[s * L:(s + 1) * L] = M // L
                    offs.append(torch.from_numpy(np.concatenate([[0], np.cumsum(c)]).astype(np.int32)).to(dev))
                xq = torch.randint(-127, 128, (T, K), dtype=torch.int8, device=dev, generator=g)
                row_index = (torch.arange(M, device=dev, dtype=torch.int32) % T).contiguous()
                xs = torch.rand(M, device=dev, generator=g) * 1e-2 + 1e-3
                ys = [torch.empty((M, N), dtype=torch.bfloat16, device=dev) for _ in range(3)]

                def a(i):
                    m = stacks[i // walks % nstack]
                    return pq.qlinear_s8_grouped_stream(xq, xs, m.wq, m.ws, None, offs[i % walks], torch.bfloat16, row_index=row_index, out=ys[0])

                def b(i, rows=64, y=1):
                    m = packed[i // walks % nstack]
                    return pq.qlinear_w4_grouped(xq, xs, m.w4, m.gs, m.ws, None, offs[i % walks], torch.bfloat16, row_index=row_index, out=ys[y], stream_rows=rows)
                w8 = torch.stack([pq.w4_expand(packed[0].w4[e], packed[0].gs[e]) for e in range(E)])
                ref = pq.qlinear_s8_grouped_stream(xq, xs, w8, packed[0].ws, None, offs[0], torch.bfloat16, row_index=row_index)
                assert torch.equal(b(0), ref) and torch.equal(b(0, 0, 2), ref), f"{name} T={T} {N} x {K}: the int4 paths and the int8 kernel on the expanded weight differ"
                del w8, ref
                reps = max(200, 2 * walks * nstack)          # (a replay's own cost, a few us, is spread over at least 200 launches)
                graphs = [graph_of(fn, reps) for fn in (a, b, lambda i: b(i, 0, 2))]
                t = dict(zip("abc", time_graphs([gr for gr, _ in graphs], reps, rounds)))
                del graphs
                med = {k: float(np.median(v)) for k, v in t.items()}
                live = L * N * K
                say(f"{name}: E={E} top_k={top_k} T={T} (M_total={M}, {L} live experts) N={N} K={K}  rotation of {nstack} stacks, {nstack * E * N * K / 2 / 1e6:.0f} MB packed")
                say(f"  (a) int8 grouped stream   {fmt(t['a'])}   {live / med['a'] / 1e6:5.2f} TB/s of the live experts' weight bytes")
                say(f"  (b) qlinear_w4_grouped    {fmt(t['b'])}   {live * 0.5078125 / med['b'] / 1e6:5.2f} TB/s of the live experts' weight bytes; (b) / (a) = {med['b'] / med['a']:.3f} (byte floor 0.508)")
                say(f"  (c) expand all + tiles    {fmt(t['c'])}   (c) / (a) = {med['c'] / med['a']:.3f}")
                if min(t["a"]) <= max(t["b"]):
                    not_faster.append(f"{name} T={T} N={N} K={K}: (b) {fmt(t['b']).strip()} against (a) {fmt(t['a']).strip()}")
            del stacks, packed
            torch.cuda.empty_cache()
    say("# shapes at which (b) is not faster than (a) (ranges overlapping or inverted): " + ("; ".join(not_faster) if not_faster else "none"))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
