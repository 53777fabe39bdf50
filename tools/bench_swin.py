"""Time the shifted-window attention kernels at Swin-T's four stage shapes, and the model's step.

wattn_fwd and wattn_bwd are alternated repeat by repeat with two yardsticks:
 (a) a device-to-device copy that moves the same bytes (forward: qkv in, o out; backward: do, qkv
     and lse in, dqkv out): the kernel is expected to be bandwidth-bound, so time / copy time is
     the figure of merit;
 (b) the composed path on the same data: roll, window partition, pad to head dim 64,
     ``scaled_dot_product_attention`` with the additive bias + mask tensor, window reverse, roll
     back, forward and backward.
Then Swin-T training steps at the same batch.

``--v2`` times the cosine variant (wattn_cos_fwd / wattn_cos_bwd, Swin V2) at window 8 on the
256 x 256 stage shapes against the same two yardsticks (the composed path normalises q and k and
multiplies the temperature in), and against the plain wattn_* at the same shape in the same
run; then Swin-V2-T training steps.

    python tools/bench_swin.py [--v2] [--batch 256] [--reps 7] [--iters 20] [--steps 10]
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
STAGES_V2 = [(3, 64), (6, 32), (12, 16), (24, 8)]  # at 256 x 256, window 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--v2", action="store_true", help="the cosine variant at Swin V2's shapes")
    a = ap.parse_args()
    k = _ext.ext()
    dev = torch.device("cuda", 0)
    B, ws, BF = a.batch, 8 if a.v2 else 7, torch.bfloat16
    S2, nb = ws * ws, (2 * ws - 1) ** 2
    print("batch %d, window %d; ms are medians of %d repeats of %d calls" % (B, ws, a.reps, a.iters))
    print("%-16s %8s %8s %6s %8s %8s %6s %9s %9s %6s" % (
        "H map shift", "fwd", "copy", "ratio", "bwd", "copy", "ratio", "fwd+bwd", "composed", "ratio"))
    for H, L in (STAGES_V2 if a.v2 else STAGES):
        for shift in ((0, ws // 2) if L > ws else (0,)):
            n = B * L * L
            qkv = torch.randn(n, 3 * H * 32, device=dev).to(BF)
            do = torch.randn(n, H * 32, device=dev).to(BF)
            bias = torch.randn(H * nb, device=dev) * 0.5
            dbias = torch.zeros_like(bias)
            geom = (H, L, L, ws, shift)
            if a.v2:
                ls, dls = torch.full((H,), 2.3, device=dev), torch.zeros(H, device=dev)
                tau = ls.exp().reshape(1, 1, H, 1, 1).to(BF)
                fwd = lambda: k.wattn_cos_fwd(qkv, ls, bias, *geom)
                bwd = lambda l: k.wattn_cos_bwd(do, qkv, l, ls, bias, dbias, dls, *geom, True)
            else:
                fwd = lambda: k.wattn_fwd(qkv, bias, *geom)
                bwd = lambda l: k.wattn_bwd(do, qkv, l, bias, dbias, *geom, True)
            o, lse = fwd()
            # (a) copies moving the kernels' bytes: a copy of m bytes reads m and writes m
            fb = (qkv.numel() + o.numel()) * 2
            bb = (do.numel() + 2 * qkv.numel()) * 2 + lse.numel() * 4
            src = torch.empty(max(fb, bb) // 2, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            # (b) the composed path
            idx = ref.swin_relative_index(ws).reshape(-1).to(dev)
            add = (bias.reshape(H, nb)[:, idx].reshape(1, 1, H, S2, S2)
                   + ref.swin_shift_mask(L, L, ws, shift).to(dev)[None, :, None]).to(BF)
            nw = L // ws

            def composed():
                t = qkv.detach().requires_grad_()
                x = t.reshape(B, L, L, 3 * H * 32)
                if shift:
                    x = torch.roll(x, (-shift, -shift), (1, 2))
                w = x.reshape(B, nw, ws, nw, ws, 3, H, 32).permute(5, 0, 1, 3, 6, 2, 4, 7)
                q, kk, v = w.reshape(3, B, nw * nw, H, S2, 32)
                if a.v2:
                    q, kk = F.normalize(q, dim=-1) * tau, F.normalize(kk, dim=-1)
                q, kk, v = F.pad(q, (0, 32)), F.pad(kk, (0, 32)), F.pad(v, (0, 32))
                out = F.scaled_dot_product_attention(q, kk, v, attn_mask=add,
                                                     scale=1.0 if a.v2 else 32 ** -0.5)[..., :32]
                out = out.reshape(B, nw, nw, H, ws, ws, 32).permute(0, 1, 4, 2, 5, 3, 6).reshape(B, L, L, H * 32)
                if shift:
                    out = torch.roll(out, (shift, shift), (1, 2))
                out.reshape(n, H * 32).backward(do)
                return t.grad

            def ours():
                return bwd(fwd()[1])

            med = statistics.median
            tf, cf = timed_pair(fwd, lambda: dst[:fb // 2].copy_(src[:fb // 2]), a.reps, a.iters)
            tb, cb = timed_pair(lambda: bwd(lse), lambda: dst[:bb // 2].copy_(src[:bb // 2]), a.reps, a.iters)
            to, tc = timed_pair(ours, composed, a.reps, max(a.iters // 4, 2))
            print("%-16s %8.4f %8.4f %6.2f %8.4f %8.4f %6.2f %9.4f %9.4f %6.2f" % (
                "%d %dx%d %d" % (H, L, L, shift), med(tf), med(cf), med(tf) / med(cf), med(tb), med(cb),
                med(tb) / med(cb), med(to), med(tc), med(to) / med(tc)), flush=True)
            print("    min-max fwd %.4f-%.4f bwd %.4f-%.4f; %.1f / %.1f MB moved" % (
                min(tf), max(tf), min(tb), max(tb), fb / 1e6, bb / 1e6), flush=True)
            if a.v2:  # the plain kernels at the same shape, alternated with the cosine ones
                pf = timed_pair(fwd, lambda: k.wattn_fwd(qkv, bias, *geom), a.reps, a.iters)
                pb = timed_pair(lambda: bwd(lse), lambda: k.wattn_bwd(do, qkv, lse, bias, dbias, *geom, True),
                                a.reps, a.iters)
                print("    cosine / plain: fwd %.4f / %.4f = %.2f, bwd %.4f / %.4f = %.2f" % (
                    med(pf[0]), med(pf[1]), med(pf[0]) / med(pf[1]), med(pb[0]), med(pb[1]),
                    med(pb[0]) / med(pb[1])), flush=True)
            del src, dst, add

    from mpi_pytorch_amd.engine import build_training
    from mpi_pytorch_amd.parallel import World
    size, name = (256, "swin_v2") if a.v2 else (224, "swin")
    img = torch.randn(B, size, size, 8, device=dev).to(BF)
    model, _opt, step, _ = build_training(name, 1000, dev, World(device=dev), 1e-3)
    y = torch.randint(0, 1000, (B,), device=dev)
    for _ in range(3):
        step(img, y)
    t = [batch_ms(lambda: step(img, y), a.steps) for _ in range(3)]
    m = statistics.median(t)
    print(name + " step, batch %d: %.1f ms, %.0f img/s (min-max %.1f-%.1f ms)" % (
        B, m, B / m * 1e3, min(t), max(t)), flush=True)


if __name__ == "__main__":
    main()
