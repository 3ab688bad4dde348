"""Dev tool (GPU box): a whole MoEGatedMLP.forward with the library's routing / combine kernels (pq_moe_route, pq_moe_combine) against the same module on the torch
plumbing (torch_plumbing = True: route_plan / combine) — outputs compared bit for bit first, both timed from hipGraph replays in ONE process, interleaved round by round.
Per case also the routing alone and the combine alone, each HIP against torch; the combine walks a rotation of y buffers larger than the 256-MiB Infinity Cache, so its
rows come from HBM as they do behind a GEMM that has just streamed its weights (at decode sizes the rotation is capped at 12 buffers: those rows are cache-fed, and say so).
The expert weights need no rotation: one set is 0.6 GB (E = 128) or 1.4 GB (Mixtral).
Cases: (b) E = 128, k = 8, 2048 -> 2 x 768 -> 2048, balanced and Zipf routing;  (a) Mixtral 8 x 7B  E = 8, k = 2, 4096 -> 2 x 14336 -> 4096;  each at T = 4096, 32 and 1.
--decode: the decode sizes T = 1, 8, 32 of the same cases — the forward with GroupedQLinear.stream_rows = 64 (the weight-streaming grouped kernel for both GEMMs) against
stream_rows = 0 (the 64-row tiles), outputs compared bit for bit before timing, the two graphs replayed in turn.  Every forward of a graph has a routing of its own and
walks a rotation of module copies, so that the live experts' weights of one graph are more than the 256-MiB Infinity Cache holds (printed per row).
usage: python tools/moe_layer_bench.py [--quick] [--decode]
       python tools/moe_layer_bench.py --one-forward     (under rocprofv3 --kernel-trace: one forward per plumbing between marker kernels)
       python tools/moe_layer_bench.py --list <kernel_trace.csv>      (the kernels between the markers, in launch order)"""
import csv
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [("b: 128 small experts", 128, 8, 2048, 768, ("balanced", "zipf")), ("a: Mixtral 8x7B", 8, 2, 4096, 14336, ("balanced",))]
K1_RATE = 4.1e12       # bytes / s kernel K1 reaches on this part: the yardstick of the combine


def routing(kind, T, E, k, seed, dev):
    """topk ids (distinct per token) and renormalised weights as a router would hand them over: int64 ids, bf16 weights"""
    g = torch.Generator(device=dev).manual_seed(seed)
    logits = torch.randn(T, E, generator=g, device=dev)
    if kind == "zipf":
        logits = logits + 1.2 * torch.log(1.0 / torch.arange(1, E + 1, device=dev, dtype=torch.float32))[None, :]
    wts, ids = torch.topk(torch.softmax(logits, dim=1), k, dim=-1)
    return ids, (wts / wts.sum(dim=-1, keepdim=True)).to(torch.bfloat16)


def make_moe(E, H, inter, dev):
    import protoquant_amd as pq
    g = torch.Generator(device=dev).manual_seed(E + H)
    gu = pq.GroupedQLinear._from_parts(torch.randint(-127, 128, (E, 2 * inter, H), generator=g, device=dev, dtype=torch.int8),
                                       torch.rand(E, 2 * inter, generator=g, device=dev) * 2e-3 + 1e-4, None)
    dn = pq.GroupedQLinear._from_parts(torch.randint(-127, 128, (E, H, inter), generator=g, device=dev, dtype=torch.int8),
                                       torch.rand(E, H, generator=g, device=dev) * 2e-3 + 1e-4, None)
    return pq.MoEGatedMLP(gu, dn)


def graph_of(fn, reps):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn(0)                                               # warm-up outside capture (code objects, workspaces)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        keep = [fn(i) for i in range(reps)]
    return gr, keep


def time_pair(graphs, reps, rounds):
    """medians (us per call) of the graphs, replayed in turn round by round"""
    for gr in graphs:
        gr.replay()
    torch.cuda.synchronize()
    ts = [[] for _ in graphs]
    for _ in range(rounds):
        for i, gr in enumerate(graphs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            gr.replay()
            b.record()
            b.synchronize()
            ts[i].append(a.elapsed_time(b) * 1e3 / reps)
    return [(float(np.median(t)), min(t), max(t)) for t in ts]


def sclk():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        return "; ".join(ln.strip() for ln in out.splitlines() if "sclk" in ln)[:200]
    except Exception as e:      # noqa: BLE001
        return f"(clock not read: {e})"


def bench_case(name, E, k, H, inter, kind, T, rounds, dev):
    import protoquant_amd as pq
    from protoquant_amd.moe import combine, route_plan
    moe = make_moe(E, H, inter, dev)
    x = (torch.randn(T, H, device=dev) * 1.5).to(torch.bfloat16)
    ids, w = routing(kind, T, E, k, 7 + T, dev)
    counts = torch.bincount(ids.reshape(-1), minlength=E)
    print(f"{name}  T={T} k={k} routing={kind}  (largest expert {int(counts.max())} rows, {int((counts > 0).sum())} of {E} experts used)", flush=True)

    def forward(torch_plumbing):
        def fn(_):
            moe.torch_plumbing = torch_plumbing
            try:
                return moe(x, ids, w)
            finally:
                moe.torch_plumbing = False
        return fn
    reps = 2 if T >= 1024 else 8
    (g_hip, out_hip), (g_torch, out_torch) = graph_of(forward(False), reps), graph_of(forward(True), reps)
    g_hip.replay(); g_torch.replay()
    torch.cuda.synchronize()
    same = all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(out_hip, out_torch))
    (th, hlo, hhi), (tt, tlo, thi) = time_pair([g_hip, g_torch], reps, rounds)
    print(f"  forward   HIP plumbing {th:9.1f} us [{hlo:.1f} .. {hhi:.1f}]   torch plumbing {tt:9.1f} us [{tlo:.1f} .. {thi:.1f}]   x{tt / th:5.2f}   bits {'SAME' if same else 'DIFFER'}", flush=True)
    assert same, "the two plumbings give different outputs"
    del g_hip, g_torch, out_hip, out_torch

    # the routing alone (ids rotated: tiny buffers, cache-fed either way)
    ids_rot = [routing(kind, T, E, k, 100 + i, dev)[0] for i in range(4)]
    xs = torch.rand(T, device=dev)
    def torch_route(i):
        r = route_plan(ids_rot[i % 4], E)
        return r + (xs.index_select(0, r[0]),)               # (the gather of the row scales GroupedQLinear.forward does on this plumbing)
    (g1, o1), (g2, o2) = graph_of(lambda i: pq.moe_route(ids_rot[i % 4], E, xs=xs), 8), graph_of(torch_route, 8)
    g1.replay(); g2.replay()
    torch.cuda.synchronize()
    same_r = all(torch.equal(a.long(), b.long()) for ra, rb in zip(o1, o2) for a, b in zip(ra, rb))
    (th, hlo, hhi), (tt, tlo, thi) = time_pair([g1, g2], 8, rounds)
    print(f"  route     HIP {th:9.1f} us [{hlo:.1f} .. {hhi:.1f}]   torch (route_plan + the scale gather) {tt:9.1f} us [{tlo:.1f} .. {thi:.1f}]   x{tt / th:5.2f}   outputs {'SAME' if same_r else 'DIFFER'}", flush=True)
    assert same_r
    del g1, g2, o1, o2

    # the combine alone, rows of y from a rotation of buffers
    M = T * k
    ybytes = M * H * 2
    nrot = max(2, min(12, -(-320 * 2**20 // ybytes)))
    row_index, offsets, rows_of, slot_of = pq.moe_route(ids, E)
    ys = [torch.randn(M, H, device=dev).to(torch.bfloat16) for _ in range(nrot)]
    ro64, so64 = rows_of.long(), slot_of.long()
    (g1, o1), (g2, o2) = graph_of(lambda i: pq.moe_combine(ys[i % nrot], rows_of, slot_of, w), nrot), graph_of(lambda i: combine(ys[i % nrot], ro64, so64, w), nrot)
    g1.replay(); g2.replay()
    torch.cuda.synchronize()
    same_c = all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(o1, o2))
    (th, hlo, hhi), (tt, tlo, thi) = time_pair([g1, g2], nrot, rounds)
    floor = (k + 1) * T * H * 2
    fed = "HBM-fed" if nrot * ybytes > 256 * 2**20 else f"cache-fed: {nrot} x {ybytes / 2**20:.1f} MiB"
    print(f"  combine   HIP {th:9.1f} us [{hlo:.1f} .. {hhi:.1f}]   torch {tt:9.1f} us [{tlo:.1f} .. {thi:.1f}]   x{tt / th:5.2f}   {floor / 1e6:.1f} MB floor -> {floor / th / 1e6:.2f} TB/s = "
          f"{floor / th * 1e6 / K1_RATE:.2f} of K1's rate ({fed})   bits {'SAME' if same_c else 'DIFFER'}", flush=True)
    assert same_c
    del g1, g2, o1, o2, ys, moe
    pq.clear_workspaces()
    torch.cuda.empty_cache()


def bench_decode(name, E, k, H, inter, kind, T, rounds, dev, mods):
    """forward at stream_rows 64 against 0; forward i of a graph runs module copy i % len(mods) under routing i"""
    reps = 12 if E > 8 else 4
    xs_ = [(torch.randn(T, H, device=dev, generator=torch.Generator(device=dev).manual_seed(i)) * 1.5).to(torch.bfloat16) for i in range(reps)]
    routes = [routing(kind, T, E, k, 31 * T + i, dev) for i in range(reps)]
    per_expert = 3 * H * inter                                      # int8 bytes of one expert's gate+up and down
    live = [int((torch.bincount(ids.reshape(-1), minlength=E) > 0).sum()) for ids, _ in routes]
    union = [set() for _ in mods]
    for i, (ids, _) in enumerate(routes):
        union[i % len(mods)].update(ids.reshape(-1).tolist())
    distinct = sum(len(u) for u in union) * per_expert
    mean_bytes = float(np.mean(live)) * per_expert

    def forward(rows):
        def fn(i):
            m = mods[i % len(mods)]
            m.gate_up.stream_rows = m.down.stream_rows = rows
            return m(xs_[i], *routes[i])
        return fn
    (g_s, out_s), (g_t, out_t) = graph_of(forward(64), reps), graph_of(forward(0), reps)
    g_s.replay(); g_t.replay()
    torch.cuda.synchronize()
    same = all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(out_s, out_t))
    (ts, slo, shi), (tt, tlo, thi) = time_pair([g_s, g_t], reps, rounds)
    print(f"{name}  T={T} k={k} routing={kind}  ({np.mean(live):.1f} of {E} experts live per forward = {mean_bytes / 1e6:.0f} MB; {distinct / 2**20:.0f} MiB of distinct live weights per graph "
          f"of {reps} forwards over {len(mods)} module cop{'y' if len(mods) == 1 else 'ies'})", flush=True)
    print(f"  forward   stream_rows=64 {ts:9.1f} us [{slo:.1f} .. {shi:.1f}]   stream_rows=0 {tt:9.1f} us [{tlo:.1f} .. {thi:.1f}]   x{tt / ts:5.2f}   "
          f"weights alone at 5.0 TB/s: {mean_bytes / 5.0e6:.1f} us   bits {'SAME' if same else 'DIFFER'}", flush=True)
    assert same, "stream_rows 64 and 0 give different outputs"
    return tt / ts


def decode(dev, quick):
    print(f"# {torch.cuda.get_device_name(0)}; {time.strftime('%Y-%m-%d')}; MoEGatedMLP.forward at decode sizes, medians [min .. max] of hipGraph replays, the two paths replayed in turn; bf16")
    print(f"# clocks before: {sclk()}")
    import protoquant_amd as pq
    worst = {}
    for (name, E, k, H, inter, kinds) in CASES:
        mods = [make_moe(E, H, inter, dev) for _ in range(3 if E > 8 else 1)]
        for kind in kinds:
            for T in (1, 8, 32):
                r = bench_decode(name, E, k, H, inter, kind, T, 5 if quick else 11, dev, mods)
                worst[T * k] = min(worst.get(T * k, r), r)
        del mods
        pq.clear_workspaces()
        torch.cuda.empty_cache()
    print("# slowest ratio (tile path / streaming path) by grouped rows: " + ", ".join(f"{m} rows x{r:.2f}" for m, r in sorted(worst.items())))
    print(f"# clocks after: {sclk()}")


def one_forward(dev):
    """for a kernel trace: per plumbing, one warm forward (not listed) and then ONE forward between two marker kernels (torch's bitwise_not on 7 elements)"""
    name, E, k, H, inter, _ = CASES[0]
    moe = make_moe(E, H, inter, dev)
    T = 4096
    x = (torch.randn(T, H, device=dev) * 1.5).to(torch.bfloat16)
    ids, w = routing("balanced", T, E, k, 7, dev)
    mark = torch.arange(7, device=dev)
    for torch_plumbing in (True, False):
        moe.torch_plumbing = torch_plumbing
        moe(x, ids, w)
        torch.cuda.synchronize()
        mark.bitwise_not()
        moe(x, ids, w)
        mark.bitwise_not()
        torch.cuda.synchronize()
    print("one forward per plumbing done (torch first, then HIP)")


def list_trace(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    spans, cur = [], None
    for r in rows:
        nm = r["Kernel_Name"]
        if "bitwise_not" in nm:
            if cur is None:
                cur = []
            else:
                spans.append(cur)
                cur = None
        elif cur is not None:
            cur.append((nm, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    assert len(spans) == 2, f"expected two marked forwards, found {len(spans)}"

    def short(nm):
        nm = nm.replace("void ", "")
        cut = nm.find("(")
        return (nm if cut < 0 else nm[:cut])[:150]
    for title, span in zip(("torch plumbing (route_plan / combine)", "HIP plumbing (pq_moe_route / pq_moe_combine)"), spans):
        print(f"## one MoEGatedMLP.forward, {title}: {len(span)} kernels, {sum(d for _, d in span):.1f} us of kernel time")
        for nm, d in span:
            print(f"  {d:9.1f} us  {short(nm)}")


def main():
    if "--list" in sys.argv:
        return list_trace(sys.argv[sys.argv.index("--list") + 1])
    assert torch.cuda.is_available(), "needs the GPU: a timing taken anywhere else says nothing"
    dev = torch.device("cuda:0")
    if "--one-forward" in sys.argv:
        return one_forward(dev)
    quick = "--quick" in sys.argv
    if "--decode" in sys.argv:
        return decode(dev, quick)
    print(f"# {torch.cuda.get_device_name(0)}; {time.strftime('%Y-%m-%d')}; medians [min .. max] of hipGraph replays, the two plumbings replayed in turn; bf16")
    print(f"# clocks before: {sclk()}")
    for (name, E, k, H, inter, kinds) in CASES:
        for kind in kinds:
            for T in (4096, 32, 1):
                bench_case(name, E, k, H, inter, kind, T, 5 if quick else 11, dev)
    print(f"# clocks after: {sclk()}")


if __name__ == "__main__":
    main()
