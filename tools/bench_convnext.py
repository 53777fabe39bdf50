"""Time ConvNeXt-Tiny's LayerNorm, GELU, layer-scale and 7x7 depthwise kernels at batch 256.

For each stage shape (H = W, C) and op: the kernel, alternated repeat by repeat with the stream
yardstick ``bn_fwd_eval`` (one read and one write of a tensor) on the op's largest operand, the
median and min-max spread of the op's repeats, the bytes the op must move (its bf16 operands
and results, each once) and the ratio of its time to the yardstick's time for the same bytes.
Operands are reused call after call: tensors that fit the last-level cache are read from it,
for the op and the yardstick alike.

    python tools/bench_convnext.py [--batch 256] [--reps 7] [--iters 50]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpi_pytorch_amd.ops import _ext  # noqa: E402
from tools.bench_grouped import timed_pair  # noqa: E402

SHAPES = [(56, 96), (28, 192), (14, 384), (7, 768)]  # every stage of convnext_tiny at 224 x 224


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    k = _ext.ext()
    dev = torch.device("cuda", 0)
    e = torch.empty(0, device=dev)
    print("%-12s %-14s %9s %17s %8s %8s %6s" % ("shape", "op", "ms", "min-max", "GB/s", "bn ms",
                                                 "x bn"))
    for H, C in SHAPES:
        def t(c):
            return torch.randn(a.batch, H, H, c, device=dev).to(torch.bfloat16)
        x, dy, h, da = t(C), t(C), t(4 * C), t(4 * C)
        w = (torch.randn(C, 7, 7, 1, device=dev) * 0.1).to(torch.bfloat16)
        dw = torch.zeros(C, 7, 7, 1, device=dev)
        p, g3, b4 = torch.rand(C, device=dev), torch.zeros(3, C, device=dev), torch.zeros(4 * C, device=dev)
        stat = k.ln_fwd(x, p, p, p, 1e-6)[1]
        acc = torch.zeros_like(x)
        # (name, call, tensors moved once in units of |x|, yardstick operand)
        ops = (("ln_fwd", lambda: k.ln_fwd(x, p, p, p, 1e-6), 2, x),
               ("ln_bwd", lambda: k.ln_bwd(dy, x, p, p, stat, g3[0], g3[1], g3[2], True), 3, x),
               ("gelu_fwd", lambda: k.gelu_fwd(h), 8, h),
               ("gelu_bwd", lambda: k.gelu_bwd(da, h, b4), 12, h),
               ("scale_add_fwd", lambda: k.scale_add_fwd(x, p, dy), 3, x),
               ("scale_add_bwd", lambda: k.scale_add_bwd(dy, x, p, g3[0], True), 3, x),
               ("dw7_fwd", lambda: k.dwconv_fwd(x, w, 1, 1, 3, 3, e, e), 2, x),
               ("dw7_dgrad+acc", lambda: k.dwconv_dgrad(dy, w, H, H, 1, 1, 3, 3, acc), 3, x),
               ("dw7_wgrad", lambda: k.dwconv_wgrad(dy, x, dw, 1, 1, 3, 3, overwrite=True), 2, x))
        for name, f, units, big in ops:
            c = big.shape[-1]
            ones, zeros = torch.ones(c, device=dev), torch.zeros(c, device=dev)
            tf, tb = timed_pair(f, lambda: k.bn_fwd_eval(big, ones, zeros, zeros, ones, 1e-5, e, False),
                                a.reps, a.iters)
            mf, mb = statistics.median(tf), statistics.median(tb)
            nbytes = units * x.numel() * 2
            same = mb * nbytes / (2 * big.numel() * 2)  # the yardstick's time for the op's bytes
            print("%-12s %-14s %9.4f %8.4f-%8.4f %8.1f %8.4f %6.2f" % (
                "%dx%d %d" % (H, H, C), name, mf, min(tf), max(tf), nbytes / mf / 1e6, same,
                mf / same), flush=True)


if __name__ == "__main__":
    main()
