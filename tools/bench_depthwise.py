"""Time MNASNet-1.0's distinct depthwise shapes (forward / dgrad / wgrad) at batch 256.

For each shape: median and min-max spread of the kernel time over repeated timed batches
(after warm-up), the achieved bytes/s against the compulsory traffic (|x| + |y|) * 2 B, and
beside it ``bn_fwd_eval`` on a tensor of the output's size - one read and one write of that
tensor, the stream-rate yardstick of the same box.

    python tools/bench_depthwise.py [--batch 256] [--reps 7] [--iters 20]
"""
import argparse
import statistics
import sys
import os

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpi_pytorch_amd.ops import _ext  # noqa: E402

# (H = W of the input, C, k, s): every depthwise layer of mnasnet1_0 at 224 x 224
SHAPES = [(112, 32, 3, 1), (112, 48, 3, 2), (56, 72, 3, 1), (56, 72, 5, 2), (28, 120, 5, 1),
          (28, 240, 5, 2), (14, 480, 5, 1), (14, 480, 3, 1), (14, 576, 3, 1), (14, 576, 5, 2),
          (7, 1152, 5, 1), (7, 1152, 3, 1)]


def timed(fn, reps, iters):
    """ms per call: `reps` timed batches of `iters` calls after one warm-up batch."""
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    k = _ext.ext()
    dev = torch.device("cuda", 0)
    e = torch.empty(0, device=dev)
    print("%-22s %-6s %9s %17s %9s | %9s %9s" % ("shape (HxW C k s)", "op", "ms", "min-max",
                                                  "GB/s", "bn ms", "bn GB/s"))
    for H, C, ks, s in SHAPES:
        p = ks // 2
        P = (H + 2 * p - ks) // s + 1
        x = torch.randn(a.batch, H, H, C, device=dev).to(torch.bfloat16)
        w = (torch.randn(C, ks, ks, 1, device=dev) * 0.2).to(torch.bfloat16)
        dy = torch.randn(a.batch, P, P, C, device=dev).to(torch.bfloat16)
        dw = torch.zeros(C, ks, ks, 1, device=dev)
        st = torch.zeros(2, C, device=dev)
        ones, zeros = torch.ones(C, device=dev), torch.zeros(C, device=dev)
        nbytes = (x.numel() + dy.numel()) * 2
        bn = timed(lambda: k.bn_fwd_eval(dy, ones, zeros, zeros, ones, 1e-5, e, True), a.reps,
                   a.iters)
        ops = (("fwd+st", lambda: k.dwconv_fwd(x, w, s, s, p, p, st, zeros)),
               ("dgrad", lambda: k.dwconv_dgrad(dy, w, H, H, s, s, p, p)),
               ("wgrad", lambda: k.dwconv_wgrad(dy, x, dw, s, s, p, p, overwrite=True)))
        for name, fn in ops:
            med, lo, hi = timed(fn, a.reps, a.iters)
            print("%-22s %-6s %9.4f %8.4f-%8.4f %9.1f | %9.4f %9.1f" % (
                "%dx%d %d k%d s%d" % (H, H, C, ks, s), name, med, lo, hi, nbytes / med / 1e6,
                bn[0], 2 * dy.numel() * 2 / bn[0] / 1e6))


if __name__ == "__main__":
    main()
