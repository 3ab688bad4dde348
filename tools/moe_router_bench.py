"""Dev tool (GPU box): the expert selection behind a router's GEMM — moe_topk (kernel K-rt, one launch) against the eager chain of the family's router after its
F.linear, bf16, at (E, k) = (8, 2) Mixtral, (60, 4) Qwen2-MoE, (64, 8) OLMoE, (128, 8) Qwen3-MoE, (32, 4) GPT-OSS (topk_softmax) and 1, 32 and 4096 tokens:
  (a)  the eager chain: softmax in f32, topk, sum, division, cast (softmax_topk) or topk, softmax (topk_softmax);
  (b)  moe_topk.
Then a whole MoEGatedMLP layer including its router (F.linear, the selection, the experts) at ONE token, for a Mixtral-sized and a 128-expert layer (the layers of
tools/moe_layer_bench.py), with the eager selection and with moe_topk.
Every candidate of a shape is captured into a hipGraph and the graphs are replayed in turn, round by round, in ONE process; every launch of a graph reads another
buffer of a rotation of logits (the large shapes walk more than the Infinity Cache holds; the small ones measure launches, not bytes).  Changes no device setting.
usage: python tools/moe_router_bench.py [--quick] [--out profiles/r26_moe_router_bench.txt]"""
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.addlnorm_bench import fmt  # noqa: E402
from tools.gemma_bench import run  # noqa: E402
from tools.moe_layer_bench import make_moe  # noqa: E402

SHAPES = (("Mixtral", 8, 2, "softmax_topk"), ("Qwen2-MoE", 60, 4, "softmax_topk"), ("OLMoE", 64, 8, "softmax_topk"), ("Qwen3-MoE", 128, 8, "softmax_topk"),
          ("GPT-OSS", 32, 4, "topk_softmax"))
TOKENS = (1, 32, 4096)
LAYERS = (("Mixtral 8x7B", 8, 2, 4096, 14336), ("128 small experts", 128, 8, 2048, 768))
DT = torch.bfloat16


def eager_chain(logits, k, kind):
    """the routers' own lines after F.linear (Qwen3MoeTopKRouter with norm_topk_prob; GptOssTopKRouter)"""
    if kind == "softmax_topk":
        p = torch.nn.functional.softmax(logits, dtype=torch.float, dim=-1)
        v, ids = torch.topk(p, k, dim=-1)
        v /= v.sum(dim=-1, keepdim=True)
        return v.to(logits.dtype), ids
    v, ids = torch.topk(logits, k, dim=-1)
    return torch.nn.functional.softmax(v, dim=1, dtype=v.dtype), ids


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    import protoquant_amd as pq
    rounds = 6 if "--quick" in sys.argv else 20
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "r26_moe_router_bench.txt")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("# tools/moe_router_bench.py  (one MI355X, one process, bf16)")
    say(f"# {torch.cuda.get_device_name(0)}; {time.strftime('%Y-%m-%d')}; medians [min .. max] per call of hipGraph replays, the candidates of a shape replayed in turn")
    say("# (a) the eager chain of the family's router after its F.linear; (b) moe_topk (K-rt): 1 launch")
    slower = []
    for name, E, k, kind in SHAPES:
        for tokens in TOKENS:
            nbuf = 64 if tokens < 1024 else 512          # (a router's logits are small: only the widest rows at 4096 tokens outgrow the 256-MiB Infinity Cache)
            fed = "HBM-fed" if nbuf * tokens * E * 2 > 300e6 else "cache-resident: launch-bound"
            g = torch.Generator(device=dev).manual_seed(tokens + E)
            logits = [(torch.randn(tokens, E, generator=g, device=dev) * 2).to(DT) for _ in range(nbuf)]
            wk, ik = pq.moe_topk(logits[0], k, kind, renormalise=True)
            we, ie = eager_chain(logits[0], k, kind)
            torch.cuda.synchronize()
            agree = float((ik == ie).all(dim=1).float().mean())          # (bf16 logits tie: eager's order among equal probabilities is its own)
            cands = [("(a)", lambda i: eager_chain(logits[i % nbuf], k, kind)), ("(b)", lambda i: pq.moe_topk(logits[i % nbuf], k, kind, renormalise=True))]
            reps = nbuf
            t = dict(zip((n for n, _ in cands), run(cands, reps, rounds)))
            med = {n: float(np.median(v)) for n, v in t.items()}
            say(f"{name} ({kind}) E={E} k={k}: {tokens} tokens  (rotation of {nbuf}, {fed}; rows whose ids equal eager's: {agree:.4f})")
            say(f"  (a) eager chain        {fmt(t['(a)'])}")
            say(f"  (b) moe_topk           {fmt(t['(b)'])}   (a) / (b) = x {med['(a)'] / med['(b)']:.2f}")
            if med["(b)"] >= med["(a)"]:
                slower.append(f"{name} E={E} k={k} x {tokens}: (b) {med['(b)']:.2f} us >= (a) {med['(a)']:.2f} us")
            del cands, logits
    say("# shapes at which moe_topk is not faster than the eager chain: " + ("; ".join(slower) if slower else "none"))
    say("# a whole MoEGatedMLP layer with its router at ONE token: F.linear -> selection -> moe_route -> 2 grouped GEMMs + gate kernel -> moe_combine")
    for name, E, k, H, inter in LAYERS:
        moe = make_moe(E, H, inter, dev)
        g = torch.Generator(device=dev).manual_seed(E)
        wr = (torch.randn(E, H, generator=g, device=dev) * 0.05).to(DT)
        xs = [(torch.randn(1, H, generator=g, device=dev) * 1.5).to(DT) for _ in range(64)]

        def eager_layer(i):
            x = xs[i % 64]
            w, ids = eager_chain(F.linear(x, wr), k, "softmax_topk")
            return moe(x, ids, w)

        def hip_layer(i):
            x = xs[i % 64]
            w, ids = pq.moe_topk(F.linear(x, wr), k, "softmax_topk", True, ids_dtype=torch.int32)
            return moe(x, ids, w)

        cands = [("eager", eager_layer), ("hip", hip_layer)]
        t = dict(zip((n for n, _ in cands), run(cands, 64, rounds)))
        med = {n: float(np.median(v)) for n, v in t.items()}
        say(f"{name}: E={E} k={k} H={H} I={inter}, 1 token")
        say(f"  layer, eager selection {fmt(t['eager'])}")
        say(f"  layer, moe_topk        {fmt(t['hip'])}   eager / moe_topk = x {med['eager'] / med['hip']:.3f}  ({med['eager'] - med['hip']:+.2f} us)")
        del cands, moe
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
