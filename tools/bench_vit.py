"""Time the fused attention and ViT token kernels at ViT-B/16's shape, and the model's step.

attn_fwd and attn_bwd (its dK / dV and dQ kernels together: the binding launches both) are
alternated repeat by repeat with the yardstick: ``torch.nn.functional.scaled_dot_product_attention``
forward + backward on the same data INCLUDING the permutes and copies that take the packed
[B, S, 3, H, 64] buffer to its [B, H, S, 64] operands and its gradients back into the packed
layout.  TFLOP/s count 4 S^2 64 flops per head forward and 10 S^2 64 backward (five products).
Then ViT-B/16 training steps at the same batch.

    python tools/bench_vit.py [--batch 256] [--reps 7] [--iters 20] [--steps 10]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpi_pytorch_amd.ops import _ext  # noqa: E402
from tools.bench_grouped import batch_ms, timed_pair  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--seq", type=int, default=197)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    k = _ext.ext()
    dev = torch.device("cuda", 0)
    B, H, S, D = a.batch, a.heads, a.seq, a.heads * 64
    qkv = torch.randn(B, S, 3, H, 64, device=dev).to(torch.bfloat16)
    do = torch.randn(B, S, D, device=dev).to(torch.bfloat16)
    o, lse = k.attn_fwd(qkv)

    def sdpa():
        t = qkv.detach().requires_grad_()
        q, kk, v = t.permute(2, 0, 3, 1, 4)
        out = F.scaled_dot_product_attention(q, kk, v).permute(0, 2, 1, 3).reshape(B, S, D)
        out.backward(do)
        return t.grad

    def ours():
        out, l = k.attn_fwd(qkv)
        return k.attn_bwd(do, qkv, out, l)

    flop_f, flop_b = 4.0 * S * S * 64 * B * H, 10.0 * S * S * 64 * B * H
    print("B %d H %d S %d" % (B, H, S))
    print("%-22s %9s %19s %9s" % ("op", "ms", "min-max", "TFLOP/s"))
    for name, f, flops in (("attn_fwd", lambda: k.attn_fwd(qkv), flop_f),
                           ("attn_bwd (dkv + dq)", lambda: k.attn_bwd(do, qkv, o, lse), flop_b)):
        t = [batch_ms(f, a.iters) for _ in range(a.reps)]
        m = statistics.median(t)
        print("%-22s %9.4f %9.4f-%9.4f %9.1f" % (name, m, min(t), max(t), flops / m / 1e9), flush=True)
    tf, ts = timed_pair(ours, sdpa, a.reps, a.iters)
    mf, ms = statistics.median(tf), statistics.median(ts)
    print("%-22s %9.4f %9.4f-%9.4f %9.1f" % ("attn fwd + bwd", mf, min(tf), max(tf),
                                             (flop_f + flop_b) / mf / 1e9))
    print("%-22s %9.4f %9.4f-%9.4f %9.1f" % ("sdpa fwd + bwd + copies", ms, min(ts), max(ts),
                                             (flop_f + flop_b) / ms / 1e9))
    print("attention / sdpa time: %.2f" % (mf / ms), flush=True)

    img = torch.randn(B, 224, 224, 8, device=dev).to(torch.bfloat16)
    rows = k.patchify(img, 16)
    pr = torch.randn(B * 196, D, device=dev).to(torch.bfloat16)
    cls, pos = torch.zeros(D, device=dev), torch.randn(197 * D, device=dev)
    dx = torch.randn(B, 197, D, device=dev).to(torch.bfloat16)
    dc, dp = torch.zeros(D, device=dev), torch.zeros(197 * D, device=dev)
    for name, f, nbytes in (("patchify", lambda: k.patchify(img, 16), 2 * img.numel() * 2),
                            ("tokens_fwd", lambda: k.tokens_fwd(pr, cls, pos), 2 * dx.numel() * 2),
                            ("tokens_bwd", lambda: k.tokens_bwd(dx, dc, dp, True), 2 * dx.numel() * 2)):
        t = [batch_ms(f, a.iters) for _ in range(a.reps)]
        m = statistics.median(t)
        print("%-22s %9.4f %9.4f-%9.4f %7.1f GB/s" % (name, m, min(t), max(t), nbytes / m / 1e6),
              flush=True)
    del rows

    from mpi_pytorch_amd.engine import build_training
    from mpi_pytorch_amd.parallel import World
    model, _opt, step, _ = build_training("vit", 1000, dev, World(device=dev), 1e-3)
    torch.nn.init.normal_(model.heads.head.weight, std=0.02)
    model._mpa_arena.sync_shadow()
    y = torch.randint(0, 1000, (B,), device=dev)
    for _ in range(3):
        step(img, y)
    t = [batch_ms(lambda: step(img, y), a.steps) for _ in range(3)]
    m = statistics.median(t)
    print("vit_b_16 step, batch %d: %.1f ms, %.0f img/s (min-max %.1f-%.1f ms)" % (
        B, m, B / m * 1e3, min(t), max(t)), flush=True)


if __name__ == "__main__":
    main()
