"""Depthwise conv kernels (csrc/kernels/conv_dw.hip) against float64 ``F.conv2d(groups=C)`` and
its autograd, the statistics epilogue, two MNASNet blocks against the fp32 CPU path, and a
bitwise-repeatable MNASNet training step.

The checks take the implementation as an argument: ``tests/test_mnasnet_cpu.py`` runs them
with ``ref`` on the CPU, which shows that the reference alone meets them."""
import pytest
import torch
import torch.nn.functional as F

from mpi_pytorch_amd.ops import ref

# (N, H, W, C, k, s).  Tiles are 8 x 8, or 16 x 16 above 512 blocks (dw_plan.h), and a block
# takes at most 8 channel vectors (72 channels run as 5 + 4).
ROUNDING_CASE = (3, 33, 35, 72, 5, 1)    # 5 x 5 tiles x 2 chunks: halos cross tile edges
CASES = [
    (2, 9, 11, 8, 3, 1),       # smaller than a tile in H, one channel vector
    (2, 15, 13, 24, 5, 2),     # odd extents, last window half in the padding
    (2, 14, 14, 48, 3, 2),     # even extents under stride 2
    (1, 7, 7, 1152, 3, 1),     # the 7 x 7 tail, 18 chunks
    ROUNDING_CASE,
    (5, 18, 18, 120, 5, 2),    # wgrad: 2 + 2 + 1 images per reduction slice
    (2, 18, 20, 4096, 5, 1),   # 512 chunks: the 16 x 16 tile (2 x 2 of them), fwd and dgrad
    (2, 18, 20, 4096, 3, 2),   # the 16 x 16 tile of the stride-2 gather dgrad
]


def _ints(shape, lo, hi, seed, dev, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).to(dtype).to(dev)


def _want64(x, w, dy, s):
    """(z, dx, dw) of the depthwise conv in float64 (NHWC / [C, k, k, 1] like the kernels)."""
    C, k = w.shape[0], w.shape[1]
    xn = x.double().cpu().permute(0, 3, 1, 2).requires_grad_()
    wn = w.double().cpu().permute(0, 3, 1, 2).requires_grad_()
    z = F.conv2d(xn, wn, None, s, k // 2, 1, C)
    dx, dw = torch.autograd.grad(z, (xn, wn), dy.double().cpu().permute(0, 3, 1, 2))
    return (z.detach().permute(0, 2, 3, 1), dx.permute(0, 2, 3, 1), dw.permute(0, 2, 3, 1))


def _same(got, want):
    return torch.equal(got.double().cpu(), want)


def check_exact(k, dev, case):
    """Small-integer operands: every partial sum is an exact fp32 integer and every output an
    exact bf16 one (<= 25 * 4 * 2 + 4 = 204 < 256), so any summation order gives ``want``."""
    N, H, W, C, ks, s = case
    p = ks // 2
    P, Q = (H + 2 * p - ks) // s + 1, (W + 2 * p - ks) // s + 1
    x = _ints((N, H, W, C), -4, 4, 1, dev)
    w = _ints((C, ks, ks, 1), -2, 2, 2, dev)
    dy = _ints((N, P, Q, C), -4, 4, 3, dev)
    z, dx, dw = _want64(x, w, dy, s)
    e = torch.empty(0, device=dev)
    assert _same(k.dwconv_fwd(x, w, s, s, p, p, e, e), z)
    assert _same(k.dwconv_dgrad(dy, w, H, W, s, s, p, p), dx)
    acc = _ints((N, H, W, C), -4, 4, 4, dev)
    assert _same(k.dwconv_dgrad(dy, w, H, W, s, s, p, p, acc.clone()), dx + acc.double().cpu())
    g = torch.full((C, ks, ks, 1), float("nan"), device=dev)
    k.dwconv_wgrad(dy, x, g, s, s, p, p, overwrite=True)
    assert _same(g, dw)
    g0 = _ints((C, ks, ks, 1), -9, 9, 5, dev, torch.float32)
    g = g0.clone()
    k.dwconv_wgrad(dy, x, g, s, s, p, p, overwrite=False)
    assert _same(g, dw + g0.double().cpu())


def check_rounding(k, dev):
    """Random-normal operands.  fwd / dgrad: one bf16 rounding (2^-8 relative) of an fp32 sum
    of <= 25 exact products (<= 26 roundings of 2^-24 on the sum of magnitudes).  wgrad stays
    fp32; n = 74 is its longest addition chain for this shape: a thread's 7 dy pixels x 2 images
    (14 FMAs), the block's 10 slots, then the 50 slab rows (25 tiles x 2 image slices)."""
    N, H, W, C, ks, s = ROUNDING_CASE
    p = ks // 2
    torch.manual_seed(7)
    x = torch.randn(N, H, W, C).to(torch.bfloat16).to(dev)
    w = (torch.randn(C, ks, ks, 1) * 0.2).to(torch.bfloat16).to(dev)
    dy = torch.randn(N, H, W, C).to(torch.bfloat16).to(dev)
    z, dx, dw = _want64(x, w, dy, s)
    za, dxa, dwa = _want64(x.abs(), w.abs(), dy.abs(), s)  # sums of the terms' magnitudes
    e = torch.empty(0, device=dev)
    u = 2.0 ** -24
    got = k.dwconv_fwd(x, w, s, s, p, p, e, e).double().cpu()
    assert bool(((got - z).abs() <= 2.0 ** -8 * z.abs() + 26 * u * za).all())
    got = k.dwconv_dgrad(dy, w, H, W, s, s, p, p).double().cpu()
    assert bool(((got - dx).abs() <= 2.0 ** -8 * dx.abs() + 26 * u * dxa).all())
    g = torch.empty(C, ks, ks, 1, device=dev)
    k.dwconv_wgrad(dy, x, g, s, s, p, p, overwrite=True)
    assert bool(((g.double().cpu() - dw).abs() <= 74 * u * dwa).all())


pytestmark = pytest.mark.gpu


def C():
    from mpi_pytorch_amd.ops import _ext
    return _ext.ext()


@pytest.mark.parametrize("case", CASES)
def test_exact_against_float64(gpu, case):
    check_exact(C(), gpu, case)


def test_rounding_against_float64(gpu):
    check_rounding(C(), gpu)


@pytest.mark.parametrize("case", [CASES[1], ROUNDING_CASE, CASES[6]])
def test_statistics_epilogue(gpu, case):
    N, H, W, Cc, ks, s = case
    p = ks // 2
    torch.manual_seed(11)
    x = (torch.randn(N, H, W, Cc, device=gpu) + 0.3).to(torch.bfloat16)
    w = (torch.randn(Cc, ks, ks, 1, device=gpu) * 0.2).to(torch.bfloat16)
    shift = torch.randn(Cc, device=gpu) * 0.1
    st, st_r = torch.zeros(2, Cc, device=gpu), torch.zeros(2, Cc, device=gpu)
    z = C().dwconv_fwd(x, w, s, s, p, p, st, shift)
    ref.dwconv_fwd(x, w, s, s, p, p, st_r, shift)
    rel = float((st - st_r).abs().max() / (st_r.abs().max() + 1e-6))
    assert rel < 2e-2, rel
    # BN fed the epilogue's statistics against BN computing its own: the two statistics differ
    # by fp32 summation order (~1e-6 of y's scale, the 1e-5 term), which moves y by at most
    # one bf16 step (2^-7 relative)
    gamma, beta = torch.rand(Cc, device=gpu) + 0.5, torch.randn(Cc, device=gpu)
    ys = []
    for stats in (st, torch.empty(0, device=gpu)):
        rm, rv = torch.zeros(Cc, device=gpu), torch.ones(Cc, device=gpu)
        ys.append(C().bn_fwd_train(z, stats, gamma, beta, rm, rv, 0.1, 1e-5,
                                   torch.empty(0, device=gpu), True,
                                   torch.zeros((), dtype=torch.long, device=gpu))[0].float())
    assert bool(((ys[0] - ys[1]).abs() <= 2.0 ** -7 * torch.maximum(ys[0].abs(), ys[1].abs())
                 + 1e-5).all())


def _cos(a, b):
    a, b = a.double().cpu().flatten(), b.double().cpu().flatten()
    return float(a @ b / (a.norm() * b.norm() + 1e-30))


@pytest.mark.parametrize("cin,cout,stride", [(40, 80, 2), (80, 80, 1)])
def test_block_parity_with_cpu_fp32(gpu, cin, cout, stride):
    from mpi_pytorch_amd.models.mnasnet import _InvertedResidual
    from mpi_pytorch_amd.parallel.arena import ParamArena
    torch.manual_seed(3)
    bc = _InvertedResidual(cin, cout, 5, stride, 6)
    bg = _InvertedResidual(cin, cout, 5, stride, 6)
    # BN affines away from their initial (1, 0): with beta = 0 a BN -> ReLU -> depthwise -> BN
    # chain is invariant to the first gamma, whose true gradient is then 0 and its cosine noise
    for m in bc.modules():
        if type(m).__name__ == "BatchNorm2d":
            torch.nn.init.uniform_(m.weight, 0.5, 1.5)
            torch.nn.init.normal_(m.bias, 0.0, 0.5)
    bg.load_state_dict(bc.state_dict())
    bg = bg.to(gpu)
    x = torch.randn(4, 14, 14, cin).to(torch.bfloat16)
    res = []
    for blk, dev in ((bc, torch.device("cpu")), (bg, gpu)):
        ParamArena(blk, dev)
        blk.train()
        xi = x.to(dev).float().requires_grad_() if dev.type == "cpu" else \
            x.to(dev).requires_grad_()
        y = blk(xi)
        torch.manual_seed(4)
        dy = torch.randn(y.shape).to(torch.bfloat16).to(dev).to(y.dtype)
        y.backward(dy)
        if dev.type == "cuda":
            torch.cuda.synchronize()
        res.append([y.detach(), xi.grad] + [q.grad for q in blk.parameters()])
    names = ["y", "dx"] + [n for n, _ in bc.named_parameters()]
    cos = {n: round(_cos(a, b), 4) for n, a, b in zip(names, *res)}
    assert min(cos.values()) >= 0.99, cos


def test_mnasnet_training_steps_bitwise(gpu, monkeypatch):
    from mpi_pytorch_amd.engine import build_training
    from mpi_pytorch_amd.parallel import World
    monkeypatch.setenv("MPA_DETERMINISTIC", "1")
    old = C().deterministic()
    C().set_deterministic(1)
    try:
        g = torch.Generator().manual_seed(1)
        x = (torch.randn(8, 64, 64, 8, generator=g) * (torch.arange(8) < 3)).to(gpu, torch.bfloat16)
        y = torch.randint(0, 10, (8,), generator=g).to(gpu)
        outs = []
        from mpi_pytorch_amd.ops.functional import DropoutRNG
        rng = DropoutRNG.state()  # (the classifier's dropout draws from a process-wide counter)
        for _ in range(2):
            torch.manual_seed(0)
            DropoutRNG.set_state(rng)
            model, _opt, step, _ = build_training("mnasnet", 10, gpu, World(device=gpu), 1e-3)
            losses = torch.stack([step(x, y).clone() for _ in range(3)])
            torch.cuda.synchronize()
            outs.append((losses.cpu(), model._mpa_arena.master.cpu().clone()))
        assert bool(torch.isfinite(outs[0][0]).all())
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    finally:
        C().set_deterministic(int(old))
