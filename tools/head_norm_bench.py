"""Dev tool (GPU box): K1hn (head_rmsnorm), the per-head q_norm / k_norm of Qwen3 and Gemma-3, against what it replaces and what the library could do without it, bf16,
on the q slice and the k slice of a fused q/k/v output at the head geometries of Qwen3-8B, Qwen3-32B, Gemma-3-27B and Gemma-3-4B and 1, 32 and 4096 tokens.  Per slice:
  K1hn   one launch on the slice where it lies (4 B/elem);
  (a)    the eager module it replaces: Qwen3RMSNorm's / Gemma3RMSNorm's torch chain, op for op, on the same view;
  (b)    .contiguous() + the existing one-wave-per-row norm kernel on the copied rows (K1on, olmo_rmsnorm: the library's norm-alone row kernel — another gain, the same
         traffic: 4 B/elem for the copy + 4 B/elem for the norm).
Every candidate of a shape is captured into a hipGraph and the graphs are replayed in turn, round by round, in ONE process.  Every launch of a graph walks a rotation of
fused q/k/v buffers larger than the 256-MiB Infinity Cache, so the large shapes are fed from HBM (the small ones measure launches, not bytes).  Changes no device
setting.  The achieved TB/s of the 4 B/elem stands beside K1on's at similar bytes in profiles/r21_olmo_postnorm_bench.txt.
usage: python tools/head_norm_bench.py [--quick] [--out profiles/r25_head_norm_bench.txt]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.addlnorm_bench import fmt  # noqa: E402
from tools.gemma_bench import rotation, run  # noqa: E402

# model -> (query heads, key / value heads, head_dim, kind)
MODELS = {"Qwen3-8B": (32, 8, 128, "llama"), "Qwen3-32B": (64, 8, 128, "llama"), "Gemma-3-27B": (32, 16, 128, "gemma"), "Gemma-3-4B": (8, 4, 256, "gemma")}
TOKENS = (4096, 32, 1)
EPS = 1e-6
DT = torch.bfloat16


def eager_norm(x, w, kind):
    """transformers' Qwen3RMSNorm.forward / Gemma3RMSNorm.forward, op for op"""
    if kind == "llama":
        h = x.to(torch.float32)
        variance = h.pow(2).mean(-1, keepdim=True)
        h = h * torch.rsqrt(variance + EPS)
        return w * h.to(x.dtype)
    h = x.float()
    h = h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + EPS)
    h = h * (1.0 + w.float())
    return h.type_as(x)


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    import protoquant_amd as pq
    rounds = 6 if "--quick" in sys.argv else 20
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "r25_head_norm_bench.txt")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("# tools/head_norm_bench.py  (one MI355X, one process, bf16)")
    say(f"# {torch.cuda.get_device_name(0)}; {time.strftime('%Y-%m-%d')}; medians [min .. max] per call of hipGraph replays, the candidates of a shape replayed in turn")
    say("# K1hn 1 launch, 4 B/elem, on the q / k slice of the fused q/k/v output where it lies")
    say("# (a) the eager norm chain of the module it replaces; (b) .contiguous() + K1on (olmo_rmsnorm) on the copied rows: 2 launches, 4 + 4 B/elem")
    slower = []
    for model, (Hq, Hkv, D, kind) in MODELS.items():
        width = (Hq + 2 * Hkv) * D
        for tokens in TOKENS:
            nbuf = rotation(tokens, width, 1)
            g = torch.Generator(device=dev).manual_seed(tokens + width)
            qkvs = [torch.randn(1, tokens, width, generator=g, device=dev).to(DT) for _ in range(nbuf)]
            w = ((1.0 if kind == "llama" else 0.0) + 0.3 * torch.randn(D, generator=g, device=dev)).to(DT)
            for name, lo, H in (("q", 0, Hq), ("k", Hq * D, Hkv)):
                def view(i, lo=lo, H=H):
                    v = qkvs[i % nbuf][..., lo:lo + H * D].view(1, tokens, H, D)
                    return v.transpose(1, 2) if kind == "gemma" else v

                row_kernel = pq.rmsnorm_quantize if kind == "llama" else pq.gemma_rmsnorm_quantize
                got = pq.head_rmsnorm(view(0), w, EPS, kind)
                want = row_kernel(view(0).reshape(-1, D).contiguous(), w, EPS, return_h=True)[1]
                torch.cuda.synchronize()
                assert torch.equal(got.reshape(-1, D), want), f"{model} {name} x {tokens}: K1hn and the row kernel differ"
                cands = [("K1hn", lambda i: pq.head_rmsnorm(view(i), w, EPS, kind)), ("(a)", lambda i: eager_norm(view(i), w, kind)),
                         ("(b)", lambda i: pq.olmo_rmsnorm(view(i).reshape(-1, D).contiguous(), w, EPS))]
                reps = 2 * nbuf if tokens >= 1024 else 64
                t = dict(zip((n for n, _ in cands), run(cands, reps, rounds)))
                n = tokens * H * D
                fed = "HBM-fed" if nbuf * tokens * width * 2 > 512e6 else "cache-resident: launch-bound"
                med = {k: float(np.median(v)) for k, v in t.items()}
                say(f"{model} {name}: {tokens} tokens x {H} heads x {D}  ({n * 2 / 2**20:.2f} MiB of a {tokens} x {width} buffer, rotation of {nbuf}: {fed})")
                say(f"  K1hn                   {fmt(t['K1hn'])}   {4 * n / med['K1hn'] / 1e6:5.2f} TB/s of its 4 B/elem")
                say(f"  (a) eager chain        {fmt(t['(a)'])}   (a) / K1hn = x {med['(a)'] / med['K1hn']:.2f}")
                say(f"  (b) copy + K1on        {fmt(t['(b)'])}   (b) / K1hn = x {med['(b)'] / med['K1hn']:.2f}")
                for other in ("(a)", "(b)"):
                    if med["K1hn"] > med[other]:
                        slower.append(f"{model} {name} x {tokens}: K1hn {med['K1hn']:.2f} us > {other} {med[other]:.2f} us")
                del cands
            del qkvs
            torch.cuda.empty_cache()
    say("# shapes at which K1hn is slower than what it replaces: " + ("; ".join(slower) if slower else "none"))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
