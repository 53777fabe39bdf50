"""Time the shifted-window attention kernels at Swin-T's four stage shapes, and the model's step.

wattn_fwd and wattn_bwd are alternated repeat by repeat with two yardsticks:
 (a) a device-to-device copy that moves the same bytes (forward: qkv in, o out; backward: do, qkv
     and lse in, dqkv out): the kernel is expected to be bandwidth-bound, so time / copy time is
     the figure of merit;
 (b) the composed path on the same data: roll, window partition, pad to head dim 64,
     ``scaled_dot_product_attention`` with the additive bias + mask tensor, window reverse, roll
     back, forward and backward.
Then Swin-T training steps at the same batch.

    python tools/bench_swin.py [--batch 256] [--reps 7] [--iters 20] [--steps 10]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpi_pytorch_amd.ops import _ext, ref  # noqa: E402
from tools.bench_grouped import batch_ms, timed_pair  # noqa: E402

STAGES = [(3, 56), (6, 28), (12, 14), (24, 7)]  # (heads, map edge) at 224 x 224, window 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    k = _ext.ext()
    dev = torch.device("cuda", 0)
    B, ws, S2, BF = a.batch, 7, 49, torch.bfloat16
    print("batch %d, window %d; ms are medians of %d repeats of %d calls" % (B, ws, a.reps, a.iters))
    print("%-16s %8s %8s %6s %8s %8s %6s %9s %9s %6s" % (
        "H map shift", "fwd", "copy", "ratio", "bwd", "copy", "ratio", "fwd+bwd", "composed", "ratio"))
    for H, L in STAGES:
        for shift in ((0, 3) if L > ws else (0,)):
            n = B * L * L
            qkv = torch.randn(n, 3 * H * 32, device=dev).to(BF)
            do = torch.randn(n, H * 32, device=dev).to(BF)
            bias = torch.randn(H * 169, device=dev) * 0.5
            dbias = torch.zeros_like(bias)
            o, lse = k.wattn_fwd(qkv, bias, H, L, L, ws, shift)
            # (a) copies moving the kernels' bytes: a copy of m bytes reads m and writes m
            fb = (qkv.numel() + o.numel()) * 2
            bb = (do.numel() + 2 * qkv.numel()) * 2 + lse.numel() * 4
            src = torch.empty(max(fb, bb) // 2, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            # (b) the composed path
            idx = ref.swin_relative_index(ws).reshape(-1).to(dev)
            add = (bias.reshape(H, 169)[:, idx].reshape(1, 1, H, S2, S2)
                   + ref.swin_shift_mask(L, L, ws, shift).to(dev)[None, :, None]).to(BF)
            nw = L // ws

            def composed():
                t = qkv.detach().requires_grad_()
                x = t.reshape(B, L, L, 3 * H * 32)
                if shift:
                    x = torch.roll(x, (-shift, -shift), (1, 2))
                w = x.reshape(B, nw, ws, nw, ws, 3, H, 32).permute(5, 0, 1, 3, 6, 2, 4, 7)
                q, kk, v = F.pad(w.reshape(3, B, nw * nw, H, S2, 32), (0, 32))
                out = F.scaled_dot_product_attention(q, kk, v, attn_mask=add, scale=32 ** -0.5)[..., :32]
                out = out.reshape(B, nw, nw, H, ws, ws, 32).permute(0, 1, 4, 2, 5, 3, 6).reshape(B, L, L, H * 32)
                if shift:
                    out = torch.roll(out, (shift, shift), (1, 2))
                out.reshape(n, H * 32).backward(do)
                return t.grad

            def ours():
                out, l = k.wattn_fwd(qkv, bias, H, L, L, ws, shift)
                return k.wattn_bwd(do, qkv, l, bias, dbias, H, L, L, ws, shift, True)

            med = statistics.median
            tf, cf = timed_pair(lambda: k.wattn_fwd(qkv, bias, H, L, L, ws, shift),
                                lambda: dst[:fb // 2].copy_(src[:fb // 2]), a.reps, a.iters)
            tb, cb = timed_pair(lambda: k.wattn_bwd(do, qkv, lse, bias, dbias, H, L, L, ws, shift, True),
                                lambda: dst[:bb // 2].copy_(src[:bb // 2]), a.reps, a.iters)
            to, tc = timed_pair(ours, composed, a.reps, max(a.iters // 4, 2))
            print("%-16s %8.4f %8.4f %6.2f %8.4f %8.4f %6.2f %9.4f %9.4f %6.2f" % (
                "%d %dx%d %d" % (H, L, L, shift), med(tf), med(cf), med(tf) / med(cf), med(tb), med(cb),
                med(tb) / med(cb), med(to), med(tc), med(to) / med(tc)), flush=True)
            print("    min-max fwd %.4f-%.4f bwd %.4f-%.4f; %.1f / %.1f MB moved" % (
                min(tf), max(tf), min(tb), max(tb), fb / 1e6, bb / 1e6), flush=True)
            del src, dst, add

    from mpi_pytorch_amd.engine import build_training
    from mpi_pytorch_amd.parallel import World
    img = torch.randn(B, 224, 224, 8, device=dev).to(BF)
    model, _opt, step, _ = build_training("swin", 1000, dev, World(device=dev), 1e-3)
    y = torch.randint(0, 1000, (B,), device=dev)
    for _ in range(3):
        step(img, y)
    t = [batch_ms(lambda: step(img, y), a.steps) for _ in range(3)]
    m = statistics.median(t)
    print("swin_t step, batch %d: %.1f ms, %.0f img/s (min-max %.1f-%.1f ms)" % (
        B, m, B / m * 1e3, min(t), max(t)), flush=True)


if __name__ == "__main__":
    main()
