"""Time the squeeze-excite / activation-gate kernels (se.hip) at MobileNetV3-Large's five SE
shapes at batch 256.

For each shape: median and min-max spread of every kernel over repeated timed batches (after a
warm-up batch), the achieved bytes/s against the kernel's compulsory traffic over the expanded
tensor, then the whole SE segment forward + backward (8 streaming launches, the gate kernels
and both fc weight gradients) next to ``bn_fwd_train`` + ``bn_bwd`` on the same tensor - the
cost of the same layer without a gate.

    python tools/bench_se.py [--batch 256] [--reps 7] [--iters 20] [--act 2]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpi_pytorch_amd.ops import _ext  # noqa: E402

# (H = W, expanded channels, squeeze width)
SHAPES = [(28, 72, 24), (28, 120, 32), (14, 480, 120), (14, 672, 168), (7, 960, 240)]


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
    ap.add_argument("--act", type=int, default=2)
    a = ap.parse_args()
    k = _ext.ext()
    dev = torch.device("cuda", 0)
    e = torch.empty(0, device=dev)
    N, act = a.batch, a.act
    print("%-16s %-18s %9s %17s %9s" % ("shape (HxW C)", "op", "ms", "min-max", "GB/s"))
    for H, C, Cs in SHAPES:
        z = torch.randn(N, H, H, C, device=dev).to(torch.bfloat16)
        du = torch.randn(N, H, H, C, device=dev).to(torch.bfloat16)
        gamma, beta = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.3
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        cnt = torch.zeros((), dtype=torch.long, device=dev)
        stats = k.bn_stats(z, rm)
        mean, rstd, aff = k.bn_stats_affine(z, stats, gamma, beta, rm, rv, 0.01, 1e-3, cnt)
        w1 = (torch.randn(Cs, 1, 1, C, device=dev) / C ** 0.5).to(torch.bfloat16)
        w2 = (torch.randn(C, 1, 1, Cs, device=dev) / Cs ** 0.5).to(torch.bfloat16)
        b1, b2 = torch.zeros(Cs, device=dev), torch.zeros(C, device=dev)
        g1, g2 = torch.zeros(Cs, 1, 1, C, device=dev), torch.zeros(C, 1, 1, Cs, device=dev)
        gb1, gb2 = torch.zeros(Cs, device=dev), torch.zeros(C, device=dev)
        pooled = k.act_pool(z, aff, act)
        h, gate = k.se_gate(pooled, w1, b1, w2, b2)
        dgate = k.act_gate_bwd_pool(du, z, aff, act)
        dpre2, dpre1, dpool = k.se_gate_bwd(dgate, h, gate, w1, w2, 1.0 / (H * H))
        sums = k.act_gate_bwd_sums(du, z, aff, act, gate, dpool, mean, rstd)
        big = z.numel() * 2  # bytes of one pass over the expanded tensor

        def fwd():
            p = k.act_pool(z, aff, act)
            _h, g = k.se_gate(p, w1, b1, w2, b2)
            return k.act_gate_fwd(z, aff, act, g)

        def bwd():
            dg = k.act_gate_bwd_pool(du, z, aff, act)
            d2, d1, dp = k.se_gate_bwd(dg, h, gate, w1, w2, 1.0 / (H * H))
            k.se_fc_wgrad(d2, h, g2, gb2, overwrite=True)
            k.se_fc_wgrad(d1, pooled, g1, gb1, overwrite=True)
            s = k.act_gate_bwd_sums(du, z, aff, act, gate, dp, mean, rstd)
            return k.act_gate_bwd_dx(du, z, aff, act, gate, dp, mean, rstd, gamma, s)

        def bn_pair():
            k.bn_fwd_train(z, stats, gamma, beta, rm, rv, 0.01, 1e-3, e, True, cnt)
            k.bn_bwd(du, z, e, mean, rstd, gamma, gb2, gb2, True, False, beta)

        ops = (("act_pool", 1, lambda: k.act_pool(z, aff, act)),
               ("se_gate", 0, lambda: k.se_gate(pooled, w1, b1, w2, b2)),
               ("act_gate_fwd", 2, lambda: k.act_gate_fwd(z, aff, act, gate)),
               ("act_gate_bwd_pool", 2, lambda: k.act_gate_bwd_pool(du, z, aff, act)),
               ("se_gate_bwd", 0, lambda: k.se_gate_bwd(dgate, h, gate, w1, w2, 1.0 / (H * H))),
               ("se_fc_wgrad x2", 0, lambda: (k.se_fc_wgrad(dpre2, h, g2, gb2, overwrite=True),
                                              k.se_fc_wgrad(dpre1, pooled, g1, gb1, overwrite=True))),
               ("act_gate_bwd_sums", 2, lambda: k.act_gate_bwd_sums(du, z, aff, act, gate, dpool,
                                                                    mean, rstd)),
               ("act_gate_bwd_dx", 3, lambda: k.act_gate_bwd_dx(du, z, aff, act, gate, dpool, mean,
                                                                rstd, gamma, sums)),
               ("segment fwd", 3, fwd), ("segment bwd", 7, bwd), ("segment fwd+bwd", 10,
                                                                  lambda: (fwd(), bwd())),
               ("bn_fwd_train+bn_bwd", 7, bn_pair))
        for name, passes, fn in ops:
            med, lo, hi = timed(fn, a.reps, a.iters)
            rate = "%9.1f" % (passes * big / med / 1e6) if passes else "%9s" % "-"
            print("%-16s %-18s %9.4f %8.4f-%8.4f %s" % ("%dx%d %d" % (H, H, C), name, med, lo, hi,
                                                         rate))


if __name__ == "__main__":
    main()
