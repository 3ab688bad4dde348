"""Dev tool (GPU box): the clamped-gate producer kernel (glu_quantize, both kinds) beside K1s (silu_mul_quantize) at the same shapes, and a whole GPT-OSS-sized expert
layer on the int8 path against the float module's eager loop.
producer: 4096 x 14336 and 8192 x 2880 bf16, g / u the halves of one [R, 2 I] tensor.  Every launch of a graph walks a rotation of input buffers larger than the 256-MiB
  Infinity Cache, so the rows come from HBM; the three kernels are replayed in turn, round by round, in ONE process.  Bytes = 2 x 2 B read + 1 B written per element.
layer:    E = 32 and 128, k = 4, H = I = 2880 (GPT-OSS 20b / 120b), T = 1, 16, 4096: MoEGatedMLP (alpha_sigmoid gate, biases; hipGraph replays) against transformers'
  GptOssExperts in bf16 (its Python loop over the experts reads the routing on the host: timed with events around eager calls).
usage: python tools/glu_quant_bench.py [--quick]
       python tools/glu_quant_bench.py --one-forward     (under rocprofv3 --kernel-trace: one forward of a tiny swapped GPT-OSS and DeepSeek-V4 experts layer between markers)
       python tools/glu_quant_bench.py --list <kernel_trace.csv>"""
import csv
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIMIT, ALPHA = 7.0, 1.702
PRODUCERS = (("silu_mul_quantize (K1s)", None), ("glu_quantize clamped_silu", "clamped_silu"), ("glu_quantize alpha_sigmoid", "alpha_sigmoid"))


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
    return f"{np.median(v):9.1f} us [{min(v):.1f} .. {max(v):.1f}]"


def producer_rows(dev, quick):
    import protoquant_amd as pq
    for rows, cols in ((4096, 14336), (8192, 2880)):
        nbuf = max(3, int(np.ceil(600e6 / (rows * 2 * cols * 2))))
        g = torch.Generator(device=dev).manual_seed(rows)
        bufs = [(torch.randn(rows, 2 * cols, generator=g, device=dev) * 3).to(torch.bfloat16) for _ in range(nbuf)]
        fns = []
        for _, kind in PRODUCERS:
            if kind is None:
                fns.append(lambda i: pq.silu_mul_quantize(bufs[i % nbuf][:, :cols], bufs[i % nbuf][:, cols:]))
            else:
                fns.append(lambda i, kind=kind: pq.glu_quantize(bufs[i % nbuf][:, :cols], bufs[i % nbuf][:, cols:], kind, LIMIT, ALPHA))
        reps = 2 * nbuf
        graphs = [graph_of(fn, reps) for fn in fns]
        times = time_graphs([g_ for g_, _ in graphs], reps, 6 if quick else 30)
        nbytes = rows * cols * 5 + rows * 4
        beyond = float((bufs[0].float().abs() > LIMIT).float().mean())
        print(f"producer  {rows} x {cols} bf16  (rotation of {nbuf} x {rows * 2 * cols * 2 / 2**20:.0f} MiB inputs: HBM-fed; {100 * beyond:.1f} % of the values beyond +-{LIMIT})")
        base = np.median(times[0])
        for (name, _), t in zip(PRODUCERS, times):
            print(f"  {name:28s} {fmt(t)}   {nbytes / np.median(t) / 1e6:5.2f} TB/s   x {np.median(t) / base:.2f} of K1s")
        del graphs, bufs
        torch.cuda.empty_cache()


def routing(T, E, k, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    wts, ids = torch.topk(torch.softmax(torch.randn(T, E, generator=g, device=dev), dim=1), k, dim=-1)
    return ids, (wts / wts.sum(dim=-1, keepdim=True)).to(torch.bfloat16)


def float_experts(E, H, inter, dev):
    """transformers' GptOssExperts in bf16 with seeded weights"""
    import transformers as tr
    from transformers.models.gpt_oss.modeling_gpt_oss import GptOssExperts
    cfg = tr.GptOssConfig(hidden_size=H, intermediate_size=inter, num_local_experts=E, num_experts_per_tok=4, num_hidden_layers=1, vocab_size=128, head_dim=64,
                          num_attention_heads=4, num_key_value_heads=2, experts_implementation="eager")
    with torch.device(dev):
        ex = GptOssExperts(cfg).to(torch.bfloat16)
    g = torch.Generator(device=dev).manual_seed(E)
    with torch.no_grad():
        for n, p in ex.named_parameters():
            p.copy_((torch.randn(p.shape, generator=g, device=dev) * (0.5 if n.endswith("bias") else 0.03)).to(torch.bfloat16))
    return ex.eval()


def layer_rows(dev, quick):
    import protoquant_amd as pq
    H = inter = 2880
    for E in ((32,) if quick else (32, 128)):
        ex = float_experts(E, H, inter, dev)
        parts = pq.clamped_experts_parts(ex)
        assert parts is not None and parts.gate_kind == "alpha_sigmoid"
        moe = pq.MoEGatedMLP.from_stacked(ex.gate_up_proj.detach(), ex.down_proj.detach(), ex.gate_up_proj_bias.detach(), ex.down_proj_bias.detach(), transposed=True,
                                          interleaved=True, gate_kind=parts.gate_kind, gate_limit=parts.limit, gate_alpha=parts.alpha)
        for T in (4096, 16, 1):
            xs = [(torch.randn(T, H, device=dev, generator=torch.Generator(device=dev).manual_seed(i)) * 1.5).to(torch.bfloat16) for i in range(4)]
            rts = [routing(T, E, 4, 10 + i, dev) for i in range(4)]
            with torch.no_grad():
                a, b = ex(xs[0], rts[0][0], rts[0][1]).float(), moe(xs[0], *rts[0]).float()
            cos = torch.nn.functional.cosine_similarity(a.reshape(1, -1), b.reshape(1, -1)).item()
            reps = 4
            gr, _ = graph_of(lambda i: moe(xs[i % 4], *rts[i % 4]), reps)
            t_int8 = time_graphs([gr], reps, 5 if quick else 20)[0]
            t_float = []
            with torch.no_grad():
                for i in range(2 if quick else 6):
                    ex(xs[i % 4], rts[i % 4][0], rts[i % 4][1])
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    ex(xs[(i + 1) % 4], rts[(i + 1) % 4][0], rts[(i + 1) % 4][1])
                    torch.cuda.synchronize()
                    t_float.append((time.perf_counter() - t0) * 1e6)
            used = int(torch.unique(rts[0][0]).numel())
            print(f"layer  GPT-OSS sized  E={E} k=4 H=I=2880 T={T}  ({used} of {E} experts used; cosine of the int8 layer to the float module {cos:.5f})")
            print(f"  MoEGatedMLP alpha_sigmoid (hipGraph) {fmt(t_int8)}   float GptOssExperts, eager loop (host clock) {fmt(t_float)}   x {np.median(t_float) / np.median(t_int8):.2f}")
            del gr
        del moe, ex
        pq.clear_workspaces()
        torch.cuda.empty_cache()


def one_forward(dev):
    """for a kernel trace: per family a tiny decoder swapped with gates="all", one warm forward, then ONE call of a swapped experts module between two marker kernels
    (torch's bitwise_not on 7 elements)"""
    import protoquant_amd as pq
    from tests import moe_models as M
    mark = torch.arange(7, device=dev)
    for family in ("gpt_oss", "deepseek_v4"):
        model = M.build(family, H=256, I=384, E=8, k=2).to(torch.bfloat16).to(dev).eval()
        block = M.sparse_blocks(model)[-1][1]
        assert pq.swap_moe_experts(model, gates="all") == 2
        ex = block.experts
        got = {}
        h = ex.register_forward_hook(lambda mod, args, out: got.update(args=tuple(a.detach().clone() for a in args)))
        ids = torch.randint(3, M.VOCAB, (2, 48), generator=torch.Generator().manual_seed(5)).to(dev)
        with torch.no_grad():
            model(ids)
            h.remove()
            torch.cuda.synchronize()
            mark.bitwise_not()
            ex(*got["args"])
            mark.bitwise_not()
            torch.cuda.synchronize()
    print("one experts forward per family done (gpt_oss first, then deepseek_v4)")


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
    for title, span in zip(("GPT-OSS (alpha_sigmoid, biases)", "DeepSeek-V4 (clamped_silu)"), spans):
        print(f"## one forward of a swapped experts module, tiny {title} decoder, T = 96, E = 8, k = 2: {len(span)} kernels, {sum(d for _, d in span):.1f} us of kernel time")
        for nm, d in span:
            print(f"  {d:9.1f} us  {short(nm)}")


def main():
    if "--list" in sys.argv:
        return list_trace(sys.argv[sys.argv.index("--list") + 1])
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    if "--one-forward" in sys.argv:
        return one_forward(dev)
    quick = "--quick" in sys.argv
    print("# tools/glu_quant_bench.py  (one MI355X, one process)")
    print(f"# {torch.cuda.get_device_name(0)}; {time.strftime('%Y-%m-%d')}; medians [min .. max] per launch of hipGraph replays, the candidates replayed in turn; bf16")
    producer_rows(dev, quick)
    layer_rows(dev, quick)


if __name__ == "__main__":
    main()
