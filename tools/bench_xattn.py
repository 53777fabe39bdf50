"""Time the short-key cross-attention kernels at PVT v2 B2's four stage shapes, and the model's step.

xattn_fwd and xattn_bwd are alternated repeat by repeat with two yardsticks:
 (a) a device-to-device copy that moves the bytes the algorithm needs (forward: q and kv in, o
     and lse out; backward: do, q, kv, o and lse in, dq and dkv out; the dK / dV slab is the
     kernel's own traffic and is not counted): time / copy time is the figure of merit;
 (b) ``scaled_dot_product_attention`` on the same bf16 data (q, k, v as [B, H, S, 64] views),
     forward, and forward + backward against xattn_fwd + xattn_bwd.
Then PVT v2 B2 training steps at the same batch.

    python tools/bench_xattn.py [--batch 256] [--reps 7] [--iters 20] [--steps 10]
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

STAGES = [(1, 3136), (2, 784), (5, 196), (8, 49)]  # (heads, queries) at 224 x 224
SK = 49


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    k = _ext.ext()
    dev = torch.device("cuda", 0)
    B, BF = a.batch, torch.bfloat16
    print("batch %d, %d keys; ms are medians of %d repeats of %d calls" % (B, SK, a.reps, a.iters))
    print("%-10s %-12s %8s %8s %6s %8s %6s %8s %8s %6s %9s %9s %6s" % (
        "H Sq", "tpw walks", "fwd", "copy", "ratio", "sdpa", "ratio", "bwd", "copy", "ratio", "fwd+bwd",
        "sdpa", "ratio"))
    for H, Sq in STAGES:
        q = torch.randn(B, Sq, H * 64, device=dev).to(BF)
        kv = torch.randn(B, SK, 2 * H * 64, device=dev).to(BF)
        do = torch.randn(B, Sq, H * 64, device=dev).to(BF)
        tpw, walks, _ = k.xattn_plan(B, H, Sq, SK)
        fwd = lambda: k.xattn_fwd(q, kv, H)
        o, lse = fwd()
        bwd = lambda: k.xattn_bwd(do, q, kv, o, lse, H)
        fb = (2 * q.numel() + kv.numel()) * 2 + lse.numel() * 4
        bb = (4 * q.numel() + 2 * kv.numel()) * 2 + lse.numel() * 4
        src = torch.empty(bb // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        qh = q.reshape(B, Sq, H, 64).transpose(1, 2)
        kh, vh = kv.reshape(B, SK, 2, H, 64).permute(2, 0, 3, 1, 4)

        def sdpa():
            return F.scaled_dot_product_attention(qh, kh, vh)

        def sdpa_train():
            t, u = q.detach().requires_grad_(), kv.detach().requires_grad_()
            k2, v2 = u.reshape(B, SK, 2, H, 64).permute(2, 0, 3, 1, 4)
            out = F.scaled_dot_product_attention(t.reshape(B, Sq, H, 64).transpose(1, 2), k2, v2)
            out.transpose(1, 2).reshape(B, Sq, H * 64).backward(do)
            return t.grad, u.grad

        def ours_train():
            o2, l2 = k.xattn_fwd(q, kv, H)
            return k.xattn_bwd(do, q, kv, o2, l2, H)

        med = statistics.median
        tf, cf = timed_pair(fwd, lambda: dst[:fb // 2].copy_(src[:fb // 2]), a.reps, a.iters)
        tf2, sf = timed_pair(fwd, sdpa, a.reps, a.iters)
        tb, cb = timed_pair(bwd, lambda: dst[:bb // 2].copy_(src[:bb // 2]), a.reps, a.iters)
        to, ts = timed_pair(ours_train, sdpa_train, a.reps, max(a.iters // 4, 2))
        print("%-10s %-12s %8.4f %8.4f %6.2f %8.4f %6.2f %8.4f %8.4f %6.2f %9.4f %9.4f %6.2f" % (
            "%d %d" % (H, Sq), "%d %d" % (tpw, walks), med(tf), med(cf), med(tf) / med(cf), med(sf),
            med(tf2) / med(sf), med(tb), med(cb), med(tb) / med(cb), med(to), med(ts), med(to) / med(ts)),
            flush=True)
        print("    min-max fwd %.4f-%.4f bwd %.4f-%.4f sdpa fwd %.4f-%.4f fwd+bwd %.4f-%.4f sdpa %.4f-%.4f; "
              "%.1f / %.1f MB moved" % (min(tf), max(tf), min(tb), max(tb), min(sf), max(sf), min(to),
                                        max(to), min(ts), max(ts), fb / 1e6, bb / 1e6), flush=True)
        del src, dst

    from mpi_pytorch_amd.engine import build_training
    from mpi_pytorch_amd.parallel import World
    img = torch.randn(B, 224, 224, 8, device=dev).to(BF)
    model, _opt, step, _ = build_training("pvt_v2", 1000, dev, World(device=dev), 1e-3)
    y = torch.randint(0, 1000, (B,), device=dev)
    for _ in range(3):
        step(img, y)
    t = [batch_ms(lambda: step(img, y), a.steps) for _ in range(3)]
    m = statistics.median(t)
    print("pvt_v2 step, batch %d: %.1f ms, %.0f img/s (min-max %.1f-%.1f ms)" % (
        B, m, B / m * 1e3, min(t), max(t)), flush=True)


if __name__ == "__main__":
    main()
