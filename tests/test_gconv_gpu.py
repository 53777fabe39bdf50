"""Grouped 3x3 conv kernels (csrc/kernels/conv_group.hip) against float64
``F.conv2d(groups=)`` and its autograd, the statistics epilogue, two ResNeXt bottlenecks
against the fp32 CPU path, and bitwise-repeatable ResNeXt-50 training steps.

The checks take the implementation as an argument: ``tests/test_resnext_cpu.py`` runs them
with ``ref`` on the CPU, which shows that the reference alone meets them."""
import pytest
import torch
import torch.nn.functional as F

from mpi_pytorch_amd.ops import ref

# (N, H, W, C, groups, s).  Tiles are 8 x 16 output pixels (4 x 16 in the stride-2 forward and
# weight gradient, 8 x 32 dx pixels in the stride-2 dgrad); a block takes 4 slabs of 16 channels.
CASE_D = (3, 33, 35, 64, 16, 1)      # Cg 4, 5 x 3 tiles: halos cross tile edges
CASE_E2 = (2, 14, 14, 128, 4, 2)     # Cg 32 under stride 2
CASES = [
    (2, 7, 11, 32, 8, 1),      # a) smaller than one tile, two slabs, Cg 4
    (2, 15, 13, 48, 6, 2),     # b) odd extents, last window half in the padding, Cg 8, 3 slabs
    (2, 18, 36, 64, 4, 2),     # c) even extents, Cg 16, 3 x 2 tiles of the forward and the gather
    CASE_D,
    (2, 7, 7, 1024, 32, 1),    # e) the 7 x 7 tail at full width, Cg 32
    CASE_E2,
    (5, 10, 18, 32, 8, 2),     # f) wgrad: 2 + 2 + 1 images per reduction slice, Cg 4
    (1, 5, 6, 16, 2, 1),       # Cg 8 under stride 1
    # wgrad's fold: 4 tiles x 4 chunks x 130 images = 2,080 blocks, so 3 images per block, 44
    # slices, 176 partial rows folded in chunks of 3 (the last chunk has 2) to 59 heads; Cg 16
    (130, 9, 17, 256, 16, 1),
]
# operand ranges with 9 Cg max|x| max|w| <= 256 (Cg 32: 288, asserted on the reference)
RANGES = {4: (3, 2), 8: (3, 1), 16: (1, 1), 32: (1, 1)}


def _ints(shape, m, seed, dev, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-m, m + 1, shape, generator=g).to(dtype).to(dev)


def _want64(x, w, dy, s, groups):
    """(z, dx, dw) of the grouped conv in float64 (NHWC / [C, 3, 3, Cg] like the kernels)."""
    xn = x.double().cpu().permute(0, 3, 1, 2).requires_grad_()
    wn = w.double().cpu().permute(0, 3, 1, 2).requires_grad_()
    z = F.conv2d(xn, wn, None, s, 1, 1, groups)
    dx, dw = torch.autograd.grad(z, (xn, wn), dy.double().cpu().permute(0, 3, 1, 2))
    return (z.detach().permute(0, 2, 3, 1), dx.permute(0, 2, 3, 1), dw.permute(0, 2, 3, 1))


def _same(got, want):
    return torch.equal(got.double().cpu(), want)


def check_exact(k, dev, case):
    """Small-integer operands: every partial sum is an exact fp32 integer and every output an
    exact bf16 one (|sum| <= 256), so any summation order gives ``want``."""
    N, H, W, C, groups, s = case
    Cg = C // groups
    P, Q = (H - 1) // s + 1, (W - 1) // s + 1
    mx, mw = RANGES[Cg]
    x = _ints((N, H, W, C), mx, 1, dev)
    w = _ints((C, 3, 3, Cg), mw, 2, dev)
    dy = _ints((N, P, Q, C), mx, 3, dev)
    z, dx, dw = _want64(x, w, dy, s, groups)
    assert float(z.abs().max()) <= 256 and float(dx.abs().max()) <= 256
    e = torch.empty(0, device=dev)
    assert _same(k.gconv_fwd(x, w, s, s, 1, 1, e, e), z)
    assert _same(k.gconv_dgrad(dy, w, H, W, s, s, 1, 1), dx)
    g = torch.full((C, 3, 3, Cg), float("nan"), device=dev)
    k.gconv_wgrad(dy, x, g, s, s, 1, 1, overwrite=True)
    assert _same(g, dw)
    g0 = _ints((C, 3, 3, Cg), 9, 5, dev, torch.float32)
    g = g0.clone()
    k.gconv_wgrad(dy, x, g, s, s, 1, 1, overwrite=False)
    assert _same(g, dw + g0.double().cpu())


def check_rounding(k, dev, case):
    """Random-normal operands.  fwd / dgrad: one bf16 rounding (2^-8 relative) of an fp32 sum of
    n = 9 Cg exact products; wgrad stays fp32 with n = N P Q.  The sum's bound is 2 n u S with
    u = 2^-24 and S the sum of the terms' magnitudes: (n - 1) u holds for any order of
    round-to-nearest additions, and the factor 2 covers an MFMA accumulate that truncates."""
    N, H, W, C, groups, s = case
    Cg = C // groups
    P, Q = (H - 1) // s + 1, (W - 1) // s + 1
    torch.manual_seed(7)
    x = torch.randn(N, H, W, C).to(torch.bfloat16).to(dev)
    w = (torch.randn(C, 3, 3, Cg) * 0.2).to(torch.bfloat16).to(dev)
    dy = torch.randn(N, P, Q, C).to(torch.bfloat16).to(dev)
    z, dx, dw = _want64(x, w, dy, s, groups)
    za, dxa, dwa = _want64(x.abs(), w.abs(), dy.abs(), s, groups)  # sums of the magnitudes
    e = torch.empty(0, device=dev)
    u, n = 2.0 ** -24, 9 * Cg
    got = k.gconv_fwd(x, w, s, s, 1, 1, e, e).double().cpu()
    assert bool(((got - z).abs() <= 2.0 ** -8 * z.abs() + 2 * n * u * za).all())
    got = k.gconv_dgrad(dy, w, H, W, s, s, 1, 1).double().cpu()
    assert bool(((got - dx).abs() <= 2.0 ** -8 * dx.abs() + 2 * n * u * dxa).all())
    g = torch.empty(C, 3, 3, Cg, device=dev)
    k.gconv_wgrad(dy, x, g, s, s, 1, 1, overwrite=True)
    assert bool(((g.double().cpu() - dw).abs() <= 2 * N * P * Q * u * dwa).all())


pytestmark = pytest.mark.gpu


def C():
    from mpi_pytorch_amd.ops import _ext
    return _ext.ext()


@pytest.mark.parametrize("case", CASES)
def test_exact_against_float64(gpu, case):
    check_exact(C(), gpu, case)


@pytest.mark.parametrize("case", [CASE_D, CASE_E2])
def test_rounding_against_float64(gpu, case):
    check_rounding(C(), gpu, case)


@pytest.mark.parametrize("case", [CASES[1], CASE_D])
def test_statistics_epilogue(gpu, case):
    N, H, W, Cc, groups, s = case
    torch.manual_seed(11)
    x = (torch.randn(N, H, W, Cc, device=gpu) + 0.3).to(torch.bfloat16)
    w = (torch.randn(Cc, 3, 3, Cc // groups, device=gpu) * 0.2).to(torch.bfloat16)
    shift = torch.randn(Cc, device=gpu) * 0.1
    st, st_r = torch.zeros(2, Cc, device=gpu), torch.zeros(2, Cc, device=gpu)
    z = C().gconv_fwd(x, w, s, s, 1, 1, st, shift)
    ref.gconv_fwd(x, w, s, s, 1, 1, st_r, shift)
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


@pytest.mark.parametrize("cin,stride", [(64, 2), (256, 1)])
def test_block_parity_with_cpu_fp32(gpu, cin, stride):
    from mpi_pytorch_amd.models.layers import BatchNorm2d, Conv2d
    from mpi_pytorch_amd.models.resnet import Bottleneck, Downsample
    from mpi_pytorch_amd.parallel.arena import ParamArena

    def make():
        ds = None
        if stride != 1 or cin != 256:
            ds = Downsample(Conv2d(cin, 256, 1, stride, 0, bias=False), BatchNorm2d(256))
        return Bottleneck(cin, 64, stride, ds, groups=32, width_per_group=4)
    torch.manual_seed(3)
    bc, bg = make(), make()
    # BN affines away from their initial (1, 0): with beta = 0 a BN -> ReLU -> conv -> BN chain
    # is invariant to the first gamma, whose true gradient is then 0 and its cosine noise
    for m in bc.modules():
        if type(m).__name__ == "BatchNorm2d":
            torch.nn.init.uniform_(m.weight, 0.5, 1.5)
            torch.nn.init.normal_(m.bias, 0.0, 0.5)
    bg.load_state_dict(bc.state_dict())
    bg = bg.to(gpu)
    x = torch.randn(4, 14, 14, cin).to(torch.bfloat16)
    res = []
    for blk, dev in ((bg, gpu), (bc, torch.device("cpu"))):
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


def test_resnext_training_steps_bitwise(gpu, monkeypatch):
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
        for _ in range(2):
            torch.manual_seed(0)
            model, _opt, step, _ = build_training("resnext50", 10, gpu, World(device=gpu), 1e-3)
            losses = torch.stack([step(x, y).clone() for _ in range(3)])
            torch.cuda.synchronize()
            outs.append((losses.cpu(), model._mpa_arena.master.cpu().clone()))
        assert bool(torch.isfinite(outs[0][0]).all())
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    finally:
        C().set_deterministic(int(old))
