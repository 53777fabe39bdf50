"""Time the neighbourhood attention kernels at NAT-Mini's four stage shapes, and the model's step.

na_fwd and na_bwd are alternated repeat by repeat with two yardsticks:
 (a) a device-to-device copy that moves the bytes the algorithm needs (forward: qkv in, o and
     lse out; backward: do, qkv and lse in, dqkv out; delta and the bias-gradient slab are the
     kernels' own traffic and are not counted): time / copy time is the figure of merit;
 (b) the composed ATen path on the same bf16 data: the index tables of ``ref.na_tables``, a gather
     of the 49 keys and values of every query ([B, H, N, 49, 32] each), ``softmax`` and two
     batched products; forward, and forward + backward against na_fwd + na_bwd.
Then NAT-Mini training steps at the same batch.

    python tools/bench_nattn.py [--batch 256] [--reps 7] [--iters 20] [--steps 10]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpi_pytorch_amd.ops import _ext, ref  # noqa: E402
from tools.bench_grouped import batch_ms, timed_pair  # noqa: E402

STAGES = [(2, 56), (4, 28), (8, 14), (16, 7)]  # (heads, map side) at 224 x 224


def composed(qkv, rpb, kidx, bidx, B, H, N):
    q, k, v = qkv.reshape(B, N, 3, H, 32).permute(2, 0, 3, 1, 4)
    kg, vg = k[:, :, kidx], v[:, :, kidx]  # [B, H, N, 49, 32]
    s = (kg @ q.unsqueeze(-1)).squeeze(-1).float() * 32 ** -0.5 + rpb.reshape(H, 169)[:, bidx]
    p = torch.softmax(s, -1).to(qkv.dtype)
    return (p.unsqueeze(-2) @ vg).squeeze(-2).transpose(1, 2).reshape(B * N, H * 32)


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
    print("batch %d; ms are medians of %d repeats of %d calls" % (B, a.reps, a.iters))
    print("%-8s %8s %8s %6s %8s %6s %8s %8s %6s %9s %9s %6s" % (
        "H map", "fwd", "copy", "ratio", "aten", "ratio", "bwd", "copy", "ratio", "fwd+bwd", "aten", "ratio"))
    for H, L in STAGES:
        N = L * L
        qkv = torch.randn(B * N, 3 * H * 32, device=dev).to(BF)
        do = torch.randn(B * N, H * 32, device=dev).to(BF)
        rpb = torch.randn(H * 169, device=dev) * 0.5
        drpb = torch.empty_like(rpb)
        kidx, bidx = (t.to(dev) for t in ref.na_tables(L, L))
        fwd = lambda: k.na_fwd(qkv, rpb, H, L, L)
        o, lse = fwd()
        bwd = lambda: k.na_bwd(do, qkv, lse, rpb, drpb, H, L, L, True)
        fb = (qkv.numel() + o.numel()) * 2 + lse.numel() * 4
        bb = (2 * qkv.numel() + o.numel()) * 2 + lse.numel() * 4
        src = torch.empty(bb // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)

        def aten():
            with torch.no_grad():
                return composed(qkv, rpb, kidx, bidx, B, H, N)

        def aten_train():
            t, r = qkv.detach().requires_grad_(), rpb.detach().requires_grad_()
            composed(t, r, kidx, bidx, B, H, N).backward(do)
            return t.grad, r.grad

        def ours_train():
            o2, l2 = k.na_fwd(qkv, rpb, H, L, L)
            return k.na_bwd(do, qkv, l2, rpb, drpb, H, L, L, True)

        med = statistics.median
        slow = max(a.iters // 4, 2)
        tf, cf = timed_pair(fwd, lambda: dst[:fb // 2].copy_(src[:fb // 2]), a.reps, a.iters)
        tf2, sf = timed_pair(fwd, aten, a.reps, slow)
        tb, cb = timed_pair(bwd, lambda: dst[:bb // 2].copy_(src[:bb // 2]), a.reps, a.iters)
        to, ts = timed_pair(ours_train, aten_train, a.reps, slow)
        print("%-8s %8.4f %8.4f %6.2f %8.4f %6.2f %8.4f %8.4f %6.2f %9.4f %9.4f %6.2f" % (
            "%d %d" % (H, L), med(tf), med(cf), med(tf) / med(cf), med(sf), med(tf2) / med(sf), med(tb),
            med(cb), med(tb) / med(cb), med(to), med(ts), med(to) / med(ts)), flush=True)
        print("    min-max fwd %.4f-%.4f bwd %.4f-%.4f aten fwd %.4f-%.4f fwd+bwd %.4f-%.4f aten %.4f-%.4f; "
              "%.1f / %.1f MB moved" % (min(tf), max(tf), min(tb), max(tb), min(sf), max(sf), min(to),
                                        max(to), min(ts), max(ts), fb / 1e6, bb / 1e6), flush=True)
        del src, dst

    from mpi_pytorch_amd.engine import build_training
    from mpi_pytorch_amd.parallel import World
    img = torch.randn(B, 224, 224, 8, device=dev).to(BF)
    model, _opt, step, _ = build_training("nat", 1000, dev, World(device=dev), 1e-3)
    y = torch.randint(0, 1000, (B,), device=dev)
    for _ in range(3):
        step(img, y)
    t = [batch_ms(lambda: step(img, y), a.steps) for _ in range(3)]
    m = statistics.median(t)
    print("nat step, batch %d: %.1f ms, %.0f img/s (min-max %.1f-%.1f ms)" % (
        B, m, B / m * 1e3, min(t), max(t)), flush=True)


if __name__ == "__main__":
    main()
