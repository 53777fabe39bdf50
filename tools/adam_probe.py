"""Time the fused Adam kernel in isolation (warm and after a 4 GiB cache-evicting write)
at ResNet-18 / ResNet-50-ish / VGG-16 parameter counts, and report achieved HBM bandwidth
(30 bytes per parameter: fp32 master/m/v read+write, fp32 grad read, bf16 shadow write).

With ``--recipe`` also the training recipe's kernels at the same sizes: ``adam_step_dev``
(Adam with lr / gradient scale read from the device record; same traffic) interleaved with
``adam_step``, and the gradient-norm pass ``grad_sqnorm`` + ``hyper_update`` (4 bytes per
parameter, read only).

With ``--layerwise`` the optimizer phase of ``adam`` (the yardstick), ``adamw``, ``lamb``
and ``lars`` on the segment plan of the ResNet-18 headline arena (64,500 classes), in one
process: AdamW moves Adam's 30 bytes per parameter, LAMB 46 (stage 1 reads p, g, m, v again),
LARS 30 against SGD-momentum's 22 (two norm passes).

With ``--ema`` the weight EMA's kernels ``ema_update`` (12 bytes per parameter) and
``ema_update_multi`` (the BN running statistics, one launch) beside ``adam`` on the same
arena, in one process.

    python tools/adam_probe.py [--recipe | --layerwise | --ema]
"""
import sys

import torch

from mpi_pytorch_amd.ops import _ext


def _time(fn, flush, cold, iters=12):
    ts = []
    for it in range(iters):
        if cold:
            flush.fill_(float(it))
        e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if it >= 2:
            ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def layerwise(k, dev, flush):
    from mpi_pytorch_amd.models import initialize_model
    from mpi_pytorch_amd.optim import build_segment_plan
    from mpi_pytorch_amd.parallel.arena import ParamArena
    arena = ParamArena(initialize_model("resnet18", 64500, False, False)[0], torch.device("cpu"),
                       shadow=False)
    seg, chunk_seg = build_segment_plan(arena, True, int(k.seg_chunk()))
    n = arena.n_train
    print("resnet18 / 64,500 classes: %d elements, %d segments, %d chunks of <= %d"
          % (n, seg.shape[0], chunk_seg.numel(), k.seg_chunk()), flush=True)
    seg, chunk_seg = seg.to(dev), chunk_seg.to(dev)
    p = torch.randn(n, device=dev)
    g = torch.randn(n, device=dev) * 1e-2
    m = torch.zeros(n, device=dev)
    v = torch.zeros(n, device=dev)
    sh = torch.empty(n, dtype=torch.bfloat16, device=dev)
    st = torch.zeros(1, device=dev)
    hyper = torch.zeros(8, device=dev)
    hyper[0], hyper[1] = 1e-3, 1.0
    part = torch.zeros(2, chunk_seg.numel(), device=dev)
    ratio = torch.ones(seg.shape[0], device=dev)
    norms = torch.zeros(seg.shape[0], 2, device=dev)

    def adam():
        k.adam_step_dev(p, g, m, v, sh, st, hyper, 0.9, 0.999, 1e-8, 0.0)

    def adamw():
        k.lamb_step_dev(p, g, m, v, sh, st, hyper, seg, chunk_seg, ratio, 0.9, 0.999, 1e-8, 0.01,
                        True)

    def lamb():
        k.lamb_norms(p, g, m, v, st, hyper, seg, chunk_seg, part[0], part[1], 0.9, 0.999, 1e-8,
                     0.01)
        k.trust_ratio(seg, chunk_seg, part[0], part[1], hyper, 0, 0.0, 0.01, ratio, norms)
        k.lamb_step_dev(p, g, m, v, sh, st, hyper, seg, chunk_seg, ratio, 0.9, 0.999, 1e-8, 0.01,
                        False)

    def sgd():
        k.sgd_step_dev(p, g, m, sh, st, hyper, 0.9, 0.0, 0.0, False)

    def lars():
        k.seg_sqnorm(p, seg, chunk_seg, hyper, False, part[0])
        k.seg_sqnorm(g, seg, chunk_seg, hyper, True, part[1])
        k.trust_ratio(seg, chunk_seg, part[0], part[1], hyper, 1, 0.001, 0.01, ratio, norms)
        k.lars_step_dev(p, g, m, sh, st, hyper, seg, chunk_seg, ratio, 0.9, 0.0, 0.01, False)

    # (adam runs first and last: the spread between equal runs is the yardstick)
    runs = [("adam", adam, 30), ("adamw", adamw, 30), ("lamb", lamb, 46), ("sgd", sgd, 22),
            ("lars", lars, 30), ("adam", adam, 30)]
    for cold in (False, True):
        for name, fn, bpp in runs:
            us, lo, hi = _time(fn, flush, cold)
            print(f"{name:13s} n={n / 1e6:7.2f}M {'cold' if cold else 'warm'}: {us:8.1f} us "
                  f"(min {lo:.1f}, max {hi:.1f})  {bpp * n / us / 1e6:6.2f} TB/s", flush=True)


def ema(k, dev, flush):
    """The weight EMA's two kernels beside ``adam`` on the ResNet-18 headline arena:
    ``ema_update`` moves 12 bytes per parameter (p read, ema read and written),
    ``ema_update_multi`` the same per element of the model's 40 BN running statistics."""
    from mpi_pytorch_amd.models import initialize_model
    from mpi_pytorch_amd.parallel.arena import ParamArena, _align
    model = initialize_model("resnet18", 64500, False, False)[0]
    n = ParamArena(model, torch.device("cpu"), shadow=False).n_train
    bufs = [torch.randn(b.numel(), device=dev) for b in model.buffers() if b.is_floating_point()]
    rows, off = [], 0
    for b in bufs:
        rows.append([b.data_ptr(), off, b.numel()])
        off += _align(b.numel())
    table_host = torch.tensor(rows, dtype=torch.int64)
    table = table_host.to(dev)
    ema_buf = torch.zeros(off, device=dev)
    nb = sum(b.numel() for b in bufs)
    print("resnet18 / 64,500 classes: %d elements, %d float buffers of %d elements"
          % (n, len(bufs), nb), flush=True)
    p = torch.randn(n, device=dev)
    e = torch.randn(n, device=dev)
    g = torch.randn(n, device=dev) * 1e-2
    m = torch.zeros(n, device=dev)
    v = torch.zeros(n, device=dev)
    sh = torch.empty(n, dtype=torch.bfloat16, device=dev)
    st = torch.ones(1, device=dev)

    def adam():
        k.adam_step(p, g, m, v, sh, st, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0)

    def ema_update():
        k.ema_update(e, p, st, 0.9998, True)

    def ema_multi():
        k.ema_update_multi(ema_buf, table, table_host, bufs, st, 0.9998, True)

    # (adam and ema_update run twice: the spread between equal runs is the yardstick)
    runs = [("adam", adam, 30 * n), ("ema_update", ema_update, 12 * n),
            ("ema_update_multi", ema_multi, 12 * nb), ("adam", adam, 30 * n),
            ("ema_update", ema_update, 12 * n)]
    for cold in (False, True):
        for name, fn, nbytes in runs:
            us, lo, hi = _time(fn, flush, cold)
            print(f"{name:17s} n={n / 1e6:7.2f}M {'cold' if cold else 'warm'}: {us:8.1f} us "
                  f"(min {lo:.1f}, max {hi:.1f})  {nbytes / us / 1e6:6.3f} TB/s", flush=True)


def main():
    recipe = "--recipe" in sys.argv[1:]
    k = _ext.load()
    if "--ema" in sys.argv[1:]:
        dev = torch.device("cuda:0")
        return ema(k, dev, torch.empty(1 << 30, dtype=torch.float32, device=dev))
    if "--layerwise" in sys.argv[1:]:
        dev = torch.device("cuda:0")
        return layerwise(k, dev, torch.empty(1 << 30, dtype=torch.float32, device=dev))
    dev = torch.device("cuda:0")
    flush = torch.empty(1 << 30, dtype=torch.float32, device=dev)
    for n in (11_689_512, 44_549_160, 138_357_544):
        n = (n + 7) // 8 * 8
        p = torch.randn(n, device=dev)
        g = torch.randn(n, device=dev) * 1e-2
        m = torch.zeros(n, device=dev)
        v = torch.zeros(n, device=dev)
        sh = torch.empty(n, dtype=torch.bfloat16, device=dev)
        st = torch.zeros(1, device=dev)
        hyper = torch.zeros(8, device=dev)
        hyper[0], hyper[1] = 1e-3, 1.0
        ws = torch.zeros(k.grad_sqnorm_grid_cap(), device=dev)

        def adam():
            k.adam_step(p, g, m, v, sh, st, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0)

        def adam_dev():
            k.adam_step_dev(p, g, m, v, sh, st, hyper, 0.9, 0.999, 1e-8, 0.0)

        def norm():  # both launches of a clipped step: partials, then sum + hyper record
            parts = k.grad_sqnorm(g, ws)
            k.hyper_update(st, hyper, ws, parts, 0, 1e-3, 0.0, 0.0, 0.0, 0.1, 0.0, 1e30, 1.0)

        def norm1():  # the streaming pass alone
            k.grad_sqnorm(g, ws)

        runs = [("adam", adam, 30)]
        if recipe:
            # (adam / adam_dev alternate twice: the spread between equal runs is the yardstick)
            runs += [("adam_dev", adam_dev, 30), ("adam", adam, 30), ("adam_dev", adam_dev, 30),
                     ("sqnorm", norm1, 4), ("sqnorm+hyper", norm, 4)]
        for cold in (False, True):
            for name, fn, bpp in runs:
                us, lo, hi = _time(fn, flush, cold)
                print(f"{name:13s} n={n / 1e6:7.2f}M {'cold' if cold else 'warm'}: {us:8.1f} us "
                      f"(min {lo:.1f}, max {hi:.1f})  {bpp * n / us / 1e6:6.2f} TB/s", flush=True)
        del p, g, m, v, sh


if __name__ == "__main__":
    main()
