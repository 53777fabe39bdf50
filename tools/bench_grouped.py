"""Time ResNeXt-50 32x4d's distinct grouped 3x3 shapes (forward / dgrad / wgrad) at batch 256.

For each shape and pass: the grouped kernel (``gconv_*``) and the dense 3x3 conv (``conv_*``)
on the block-diagonal expanded weight, alternated repeat by repeat after both are warm, with
the median and min-max spread of each path's repeats; the achieved bytes/s against the
compulsory activation traffic (|x| + |y|) * 2 B; and ``bn_fwd_eval`` on a tensor of the
output's size - one read and one write of that tensor, the stream-rate yardstick of the same
box.  The operands are reused call after call, so tensors that fit the last-level cache are
read from it: the GB/s column is a cache-warm rate, not an HBM rate, for the grouped path,
the dense path and the yardstick alike.

    python tools/bench_grouped.py [--batch 256] [--reps 7] [--iters 200]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpi_pytorch_amd.ops import _ext  # noqa: E402

# (H = W of the input, C, groups, s): every grouped conv of resnext50_32x4d at 224 x 224
SHAPES = [(56, 128, 32, 1), (56, 256, 32, 2), (28, 256, 32, 1), (28, 512, 32, 2),
          (14, 512, 32, 1), (14, 1024, 32, 2), (7, 1024, 32, 1)]


def batch_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def timed_pair(f, g, reps, iters):
    """ms per call of f and g: both warmed, then `reps` timed batches of each, alternating."""
    for fn in (f, g):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    tf, tg = [], []
    for _ in range(reps):
        tf.append(batch_ms(f, iters))
        tg.append(batch_ms(g, iters))
    return tf, tg


def dense_weight(w, groups):
    """[C, 3, 3, Cg] grouped -> [C, 3, 3, C] block-diagonal."""
    C, _, _, Cg = w.shape
    d = torch.zeros(C, 3, 3, C, device=w.device, dtype=w.dtype)
    for g in range(groups):
        d[g * Cg:(g + 1) * Cg, :, :, g * Cg:(g + 1) * Cg] = w[g * Cg:(g + 1) * Cg]
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    k = _ext.ext()
    dev = torch.device("cuda", 0)
    e = torch.empty(0, device=dev)
    print("%-18s %-6s %9s %17s %8s | %9s %17s %7s | %8s %6s" % (
        "shape (HxW C s)", "op", "gconv ms", "min-max", "GB/s", "dense ms", "min-max", "ratio",
        "bn ms", "x bn"))
    for H, C, groups, s in SHAPES:
        P = (H - 1) // s + 1
        Cg = C // groups
        x = torch.randn(a.batch, H, H, C, device=dev).to(torch.bfloat16)
        w = (torch.randn(C, 3, 3, Cg, device=dev) * 0.2).to(torch.bfloat16)
        wd = dense_weight(w, groups)
        wdt = wd.permute(3, 1, 2, 0).contiguous()  # the arena's [C][R*S][K] copy for dgrad
        dy = torch.randn(a.batch, P, P, C, device=dev).to(torch.bfloat16)
        dw = torch.zeros(C, 3, 3, Cg, device=dev)
        dwd = torch.zeros(C, 3, 3, C, device=dev)
        st = torch.zeros(2, C, device=dev)
        ones, zeros = torch.ones(C, device=dev), torch.zeros(C, device=dev)
        nbytes = (x.numel() + dy.numel()) * 2
        bn = statistics.median(timed_pair(
            lambda: k.bn_fwd_eval(dy, ones, zeros, zeros, ones, 1e-5, e, True),
            lambda: None, a.reps, a.iters)[0])
        ops = (("fwd+st", lambda: k.gconv_fwd(x, w, s, s, 1, 1, st, zeros),
                lambda: k.conv_fwd(x, wd, e, s, s, 1, 1, False, st, zeros)),
               ("dgrad", lambda: k.gconv_dgrad(dy, w, H, H, s, s, 1, 1),
                lambda: k.conv_dgrad(dy, wd, H, H, s, s, 1, 1, wdt)),
               ("wgrad", lambda: k.gconv_wgrad(dy, x, dw, s, s, 1, 1, overwrite=True),
                lambda: k.conv_wgrad(dy, x, dwd, s, s, 1, 1, overwrite=True)))
        for name, f, g in ops:
            tf, tg = timed_pair(f, g, a.reps, a.iters)
            mf, mg = statistics.median(tf), statistics.median(tg)
            print("%-18s %-6s %9.4f %8.4f-%8.4f %8.1f | %9.4f %8.4f-%8.4f %7.2f | %8.4f %6.2f" % (
                "%dx%d %d s%d" % (H, H, C, s), name, mf, min(tf), max(tf), nbytes / mf / 1e6,
                mg, min(tg), max(tg), mg / mf, bn, mf / bn), flush=True)


if __name__ == "__main__":
    main()
