"""Dev tool (GPU box): the grouped int8 qlinear (pq.qlinear_s8_grouped: one launch over all experts of a mixture-of-experts layer) against the per-expert loop of
pq.qlinear_s8 on the SAME buffers — the gate+up and the down GEMM of one MoE layer, outputs compared bit for bit, both timed from hipGraph replays, interleaved round by
round.  The graphs walk a rotation of weight sets larger than the 256-MiB Infinity Cache, so the weights come from HBM as they do for a layer inside a model.
Cases: (a) Mixtral 8 x 7B  E = 8, k = 2, 4096 -> 2 x 14336 -> 4096;  (b) E = 128, k = 8, 2048 -> 2 x 768 -> 2048;  each at T = 4096 (prefill) and T = 32 (decode),
with balanced, Zipf-skewed and one-expert-takes-all routings (seeded).
--decode: the two GEMMs alone at T = 1, 8, 32 — the weight-streaming entry (pq.qlinear_s8_grouped_stream) against the tile entry (pq.qlinear_s8_grouped) on the same
buffers, with the bytes of the live experts' weights and the TB/s they imply.  usage: python tools/grouped_bench.py [--quick] [--rot] [--decode]"""
import subprocess
import sys
import time

import numpy as np
import torch

import os
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import protoquant_amd as pq  # noqa: E402
from protoquant_amd import _lib  # noqa: E402

CASES = [("a: Mixtral 8x7B", 8, 2, 4096, 14336), ("b: 128 small experts", 128, 8, 2048, 768)]
dev = torch.device("cuda:0")
quick = "--quick" in sys.argv
if "--rot" in sys.argv:
    _lib.set_option("PQ_GROUPED_ROT", "1")


def counts_for(kind, E, M, rng):
    if kind == "balanced":
        c = np.full(E, M // E)
        c[: M - c.sum()] += 1
        return c
    if kind == "one expert":
        c = np.zeros(E, dtype=np.int64)
        c[E // 2] = M
        return c
    w = 1.0 / np.arange(1, E + 1) ** 1.2                     # Zipf-skewed
    return np.bincount(rng.choice(E, size=M, p=w / w.sum()), minlength=E)


def sclk():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        return "; ".join(ln.strip() for ln in out.splitlines() if "sclk" in ln)[:200]
    except Exception as e:      # noqa: BLE001
        return f"(clock not read: {e})"


def bench_gemm(tag, E, N, K, M, off_np, rounds):
    """one grouped GEMM [M rows sorted by expert] x [E, N, K] against the per-expert loop; returns (grouped us, loop us, tile name)"""
    nrot = max(2, min(12, -(-320 * 2**20 // (E * N * K))))
    g = torch.Generator(device=dev).manual_seed(N + K + M)
    wrot = [torch.randint(-127, 128, (E, N, K), generator=g, device=dev, dtype=torch.int8) for _ in range(nrot)]
    ws = torch.rand(E, N, generator=g, device=dev) * 1e-2 + 1e-3
    xq = torch.randint(-127, 128, (M, K), generator=g, device=dev, dtype=torch.int8)
    xs = torch.rand(M, generator=g, device=dev) * 1e-2 + 1e-3
    off = torch.from_numpy(off_np.astype(np.int32)).to(dev)
    y_g = torch.empty((M, N), dtype=torch.bfloat16, device=dev)
    y_l = torch.empty((M, N), dtype=torch.bfloat16, device=dev)
    spans = [(e, int(off_np[e]), int(off_np[e + 1])) for e in range(E) if off_np[e + 1] > off_np[e]]

    def grouped(w):
        pq.qlinear_s8_grouped(xq, xs, w, ws, None, off, torch.bfloat16, out=y_g)

    def loop(w):
        for e, lo, hi in spans:
            pq.qlinear_s8(xq[lo:hi], xs[lo:hi], w[e], ws[e], None, torch.bfloat16, out=y_l[lo:hi])

    graphs = []
    for fn in (grouped, loop):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            fn(wrot[0])                                     # warm-up outside capture (code objects, workspaces)
        torch.cuda.current_stream().wait_stream(s)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for w in wrot:
                fn(w)
        graphs.append(gr)
    for gr in graphs:
        gr.replay()
    torch.cuda.synchronize()
    same = torch.equal(y_g.view(torch.int16), y_l.view(torch.int16))
    ts = [[], []]
    for _ in range(rounds):
        for i, gr in enumerate(graphs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            gr.replay()
            b.record()
            b.synchronize()
            ts[i].append(a.elapsed_time(b) * 1e3 / nrot)
    tg, tl = (float(np.median(t)) for t in ts)
    name = _lib.lib().pq_grouped_variant_name(E, M, N, K).decode()
    print(f"  {tag:<8} M={M:<6} N={N:<6} K={K:<6} grouped {tg:9.1f} us [{min(ts[0]):.1f} .. {max(ts[0]):.1f}]   per-expert loop ({len(spans)} launches) {tl:9.1f} us "
          f"[{min(ts[1]):.1f} .. {max(ts[1]):.1f}]   x{tl / tg:5.2f}   {name}   bits {'SAME' if same else 'DIFFER'}", flush=True)
    assert same, "grouped output differs from the per-expert loop"
    return tg, tl


def bench_decode_gemm(tag, E, N, K, M, off_np, rounds):
    """one grouped GEMM at decode size: streaming entry against tile entry, weight sets rotated (HBM-fed); returns (stream us, tiles us)"""
    live = int((np.diff(off_np) > 0).sum())
    nrot = max(2, min(16, -(-512 * 2**20 // (live * N * K))))          # the LIVE experts of the rotation: more than the Infinity Cache holds
    g = torch.Generator(device=dev).manual_seed(N + K + M)
    wrot = [torch.randint(-127, 128, (E, N, K), generator=g, device=dev, dtype=torch.int8) for _ in range(nrot)]
    ws = torch.rand(E, N, generator=g, device=dev) * 1e-2 + 1e-3
    xq = torch.randint(-127, 128, (M, K), generator=g, device=dev, dtype=torch.int8)
    xs = torch.rand(M, generator=g, device=dev) * 1e-2 + 1e-3
    off = torch.from_numpy(off_np.astype(np.int32)).to(dev)
    ys = [torch.empty((M, N), dtype=torch.bfloat16, device=dev) for _ in range(2)]
    graphs = []
    for fn, y in ((pq.qlinear_s8_grouped_stream, ys[0]), (pq.qlinear_s8_grouped, ys[1])):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            fn(xq, xs, wrot[0], ws, None, off, torch.bfloat16, out=y)
        torch.cuda.current_stream().wait_stream(s)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for w in wrot:
                fn(xq, xs, w, ws, None, off, torch.bfloat16, out=y)
        graphs.append(gr)
    for gr in graphs:
        gr.replay()
    torch.cuda.synchronize()
    same = torch.equal(ys[0].view(torch.int16), ys[1].view(torch.int16))
    ts = [[], []]
    for _ in range(rounds):
        for i, gr in enumerate(graphs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            gr.replay()
            b.record()
            b.synchronize()
            ts[i].append(a.elapsed_time(b) * 1e3 / nrot)
    t_s, t_t = (float(np.median(t)) for t in ts)
    nbytes = live * N * K
    plan = _lib.lib().pq_grouped_stream_plan_name(E, M, N, K).decode()
    print(f"  {tag:<8} M={M:<4} N={N:<6} K={K:<6} streaming {t_s:8.1f} us [{min(ts[0]):.1f} .. {max(ts[0]):.1f}] = {nbytes / t_s / 1e6:5.2f} TB/s   tiles {t_t:8.1f} us "
          f"[{min(ts[1]):.1f} .. {max(ts[1]):.1f}] = {nbytes / t_t / 1e6:5.2f} TB/s   x{t_t / t_s:5.2f}   {live} live experts = {nbytes / 1e6:.1f} MB ({nrot} weight sets)   {plan}   "
          f"bits {'SAME' if same else 'DIFFER'}", flush=True)
    assert same, "the streaming entry differs from the tile entry"
    del wrot, graphs
    torch.cuda.empty_cache()
    return t_s, t_t


def decode_main():
    print(f"# {torch.cuda.get_device_name(0)}; {time.strftime('%Y-%m-%d')}; the two grouped GEMMs of a MoE layer at decode sizes: pq.qlinear_s8_grouped_stream against pq.qlinear_s8_grouped; "
          "medians [min .. max] of hipGraph replays in turn, weight sets rotated (HBM-fed); TB/s = bytes of the live experts' weights / time")
    print(f"# clocks before: {sclk()}")
    rng = np.random.default_rng(0)
    for (name, E, k, H, inter) in CASES:
        for T in (1, 8, 32):
            M = T * k
            if M > 64:
                print(f"{name}  T={T} k={k}: {M} grouped rows — beyond the 64 the streaming entry serves; GroupedQLinear takes the tiles there whatever stream_rows says")
                continue
            for kind in (("balanced",) if E == 8 else ("balanced", "zipf")):
                c = np.bincount(rng.choice(E, size=M, replace=M > E), minlength=E) if kind == "balanced" and M <= E else counts_for(kind, E, M, rng)
                off = np.concatenate([[0], np.cumsum(c)])
                print(f"{name}  T={T} k={k} routing={kind}  (largest expert {int(c.max())} rows, {int((c > 0).sum())} of {E} experts live)")
                rounds = 5 if quick else 9
                s1, t1 = bench_decode_gemm("gate+up", E, 2 * inter, H, M, off, rounds)
                s2, t2 = bench_decode_gemm("down", E, H, inter, M, off, rounds)
                print(f"  layer (both GEMMs): streaming {s1 + s2:8.1f} us   tiles {t1 + t2:8.1f} us   x{(t1 + t2) / (s1 + s2):5.2f}")
    print(f"# clocks after: {sclk()}")


def main():
    if "--decode" in sys.argv:
        return decode_main()
    print(f"# {torch.cuda.get_device_name(0)}; {time.strftime('%Y-%m-%d')}; PQ_GROUPED_ROT={'1' if '--rot' in sys.argv else '0'}; medians of hipGraph replays, weights rotated (HBM-fed)")
    print(f"# clocks before: {sclk()}")
    rng = np.random.default_rng(0)
    for (name, E, k, H, inter) in CASES:
        for T in ((4096,) if quick else (4096, 32)):
            M = T * k
            for kind in ("balanced", "zipf", "one expert"):
                off = np.concatenate([[0], np.cumsum(counts_for(kind, E, M, rng))])
                print(f"{name}  T={T} k={k} routing={kind}  (largest expert {int(np.diff(off).max())} rows, {int((np.diff(off) > 0).sum())} of {E} experts used)")
                rounds = 5 if quick else 9
                g1, l1 = bench_gemm("gate+up", E, 2 * inter, H, M, off, rounds)
                g2, l2 = bench_gemm("down", E, H, inter, M, off, rounds)
                print(f"  layer (both GEMMs): grouped {g1 + g2:9.1f} us   per-expert loop {l1 + l2:9.1f} us   x{(l1 + l2) / (g1 + g2):5.2f}")
    print(f"# clocks after: {sclk()}")


if __name__ == "__main__":
    main()
