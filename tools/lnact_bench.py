"""Dev tool (GPU box): K1l (layernorm_quantize: LayerNorm + per-token int8 quantisation in one kernel) against F.layer_norm followed by quantize() (K1), and K1u
(act_quantize: relu / tanh GELU / erf GELU + quantisation in one kernel) against the torch activation followed by quantize(), bf16.  Both candidates are captured into
hipGraphs and replayed in turn, round by round, in ONE process.  Every launch of a graph walks a rotation of input buffers larger than the 256-MiB Infinity Cache, so
the large shapes are fed from HBM (the small ones measure launches, not bytes).  Bytes per element: 2 read + 1 written = 3 for the fused kernels; the pairs move
2 + 2 (the torch op) + 2 + 1 (K1) = 7.
usage: python tools/lnact_bench.py [--quick] [> profiles/r15_lnact_bench.txt]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LN_SHAPES = ((4096, 768), (4096, 4096), (4096, 6144), (32, 4096), (1, 6144))          # GPT-2 small, a 4096-wide hidden state, StarCoder2-15B / GPT-NeoX-20B, decode
ACT_SHAPES = ((4096, 3072), (4096, 16384), (2048, 24576), (32, 16384), (1, 24576))    # the 4 H-wide intermediates of the same models
EPS = 1e-5
TORCH_ACT = {"relu": torch.relu, "gelu_tanh": lambda t: torch.nn.functional.gelu(t, approximate="tanh"), "gelu_erf": torch.nn.functional.gelu}


def graph_of(fn, reps):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn(0)                                               # warm-up outside capture (code objects)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        keep = [fn(i) for i in range(reps)]
    return gr, keep


def time_graphs(graphs, reps, rounds):
    """per graph, microseconds per launch of every round; the graphs are replayed in turn"""
    out = [[] for _ in graphs]
    for gr in graphs:
        gr.replay()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for i, gr in enumerate(graphs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            gr.replay()
            b.record()
            b.synchronize()
            out[i].append(a.elapsed_time(b) * 1e3 / reps)
    return out


def fmt(v):
    return f"{np.median(v):8.2f} us [{min(v):.2f} .. {max(v):.2f}]"


def run(label_f, label_p, fused, pair, rows, cols, nbuf, rounds):
    reps = 2 * nbuf if rows >= 1024 else 64
    graphs = [graph_of(fn, reps) for fn in (fused, pair)]
    tf, tp = time_graphs([g_ for g_, _ in graphs], reps, rounds)
    n = rows * cols
    print(f"  {label_f:<24s}{fmt(tf)}   {(3 * n + 4 * rows) / np.median(tf) / 1e6:5.2f} TB/s of its 3 B/elem")
    print(f"  {label_p:<24s}{fmt(tp)}   {(7 * n + 4 * rows) / np.median(tp) / 1e6:5.2f} TB/s of its 7 B/elem   pair / fused = x {np.median(tp) / np.median(tf):.2f}")
    del graphs


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    import protoquant_amd as pq
    rounds = 6 if "--quick" in sys.argv else 20
    dev = torch.device("cuda:0")
    print("# tools/lnact_bench.py  (one MI355X, one process)")
    print(f"# {torch.cuda.get_device_name(0)}; {time.strftime('%Y-%m-%d')}; medians [min .. max] per call of hipGraph replays, the two candidates replayed in turn; bf16")
    print("# fused = one launch, 3 B/elem; pair = the torch op, then quantize() (K1): 2 launches, 7 B/elem")
    for rows, cols in LN_SHAPES:
        nbuf = min(max(3, int(np.ceil(600e6 / (rows * cols * 2)))), 64)
        g = torch.Generator(device=dev).manual_seed(rows + cols)
        xs = [(torch.randn(rows, cols, generator=g, device=dev) + 0.3).to(torch.bfloat16) for _ in range(nbuf)]
        w = (1 + 0.1 * torch.randn(cols, generator=g, device=dev)).to(torch.bfloat16)
        b = (0.1 * torch.randn(cols, generator=g, device=dev)).to(torch.bfloat16)
        qa, ha = pq.layernorm_quantize(xs[0], w, b, EPS, return_h=True)
        hb = torch.nn.functional.layer_norm(xs[0], (cols,), w, b, EPS)
        torch.cuda.synchronize()
        frac = (ha != hb).float().mean().item()
        fed = "HBM-fed" if nbuf * rows * cols * 2 > 512e6 else "cache-resident: launch-bound"
        print(f"LayerNorm {rows} x {cols} bf16  (rotation of {nbuf} x {rows * cols * 2 / 2**20:.2f} MiB inputs: {fed}; stored h differs from F.layer_norm in {frac:.2e} of the elements)")
        run("fused (K1l)", "pair  (layer_norm + K1)", lambda i: pq.layernorm_quantize(xs[i % nbuf], w, b, EPS),
            lambda i: pq.quantize(torch.nn.functional.layer_norm(xs[i % nbuf], (cols,), w, b, EPS)), rows, cols, nbuf, rounds)
        del xs
        torch.cuda.empty_cache()
    for rows, cols in ACT_SHAPES:
        nbuf = min(max(3, int(np.ceil(600e6 / (rows * cols * 2)))), 64)
        g = torch.Generator(device=dev).manual_seed(rows + cols)
        xs = [(torch.randn(rows, cols, generator=g, device=dev) * 1.5).to(torch.bfloat16) for _ in range(nbuf)]
        fed = "HBM-fed" if nbuf * rows * cols * 2 > 512e6 else "cache-resident: launch-bound"
        for kind in ("relu", "gelu_tanh", "gelu_erf"):
            act = TORCH_ACT[kind]
            _, ha = pq.act_quantize(xs[0], kind, return_h=True)
            torch.cuda.synchronize()
            frac = (ha != act(xs[0])).float().mean().item()
            print(f"{kind} {rows} x {cols} bf16  (rotation of {nbuf} x {rows * cols * 2 / 2**20:.2f} MiB inputs: {fed}; stored h differs from torch's in {frac:.2e} of the elements)")
            run("fused (K1u)", "pair  (torch act + K1)", lambda i: pq.act_quantize(xs[i % nbuf], kind), lambda i: pq.quantize(act(xs[i % nbuf])), rows, cols, nbuf, rounds)
        del xs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
