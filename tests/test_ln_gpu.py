"""LayerNorm, GELU, layer-scale (csrc/kernels/ln.hip) and 7x7 depthwise kernels against float64,
one ConvNeXt block against the fp32 CPU path, and a bitwise-repeatable training step.

The checks take the implementation as an argument: ``tests/test_convnext_cpu.py`` runs them
with ``ref`` on the CPU, which shows that the reference alone meets them."""
import math

import pytest
import torch

import test_depthwise_gpu as dg
from mpi_pytorch_amd.ops import ref

U = 2.0 ** -24   # fp32 unit roundoff
B = 2.0 ** -8    # bf16 unit roundoff

# (M, C): one vector; odd vector count with a masked tail; the four ConvNeXt widths; a whole
# wave per row; several slab rows per launch with two trips per block
LN_SHAPES = [(1, 8), (5, 40), (98, 96), (37, 192), (1003, 384), (300, 768), (9, 2048), (20011, 96)]
SCALE_SHAPES = [(1, 8), (98, 96), (4099, 40)]
GELU_ROWS = [1, 37, 4099]
# (N, H, W, C): smaller than a tile; the 7 x 7 tail in 16 chunks; 72 channels as 6 + 3 vectors
# with halos across tile edges; 640 blocks of 16 x 16 tiles at 96 channels (dw_plan.h)
DW7_CASES = [(2, 9, 11, 8), (1, 7, 7, 768), (3, 33, 35, 72), (64, 18, 20, 96)]


def _ints(shape, lo, hi, seed, dev, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).to(dtype).to(dev)


def _d(t):
    return t.double().cpu()


def check_ln_exact(k, dev, M, C, pre, act=torch.bfloat16):
    """Row i holds +a_i and -a_i in equal counts (a_i a power of two), eps = 0: mean 0, rstd
    1 / a_i and xhat = +-1 are exact, so y, stat, dgamma and dbeta equal the float64 values
    bit for bit in any summation order."""
    g = torch.Generator().manual_seed(M * 31 + C)
    sign = torch.stack([torch.randperm(C, generator=g) % 2 for _ in range(min(M, 64))]) * 2.0 - 1.0
    sign = sign.repeat((M + 63) // 64, 1)[:M]
    a = 2.0 ** ((torch.arange(M) % 8) - 3.0)
    gamma, beta = _ints((C,), -3, 3, 1, dev), _ints((C,), -3, 3, 2, dev)
    pb = _ints((C,), -3, 3, 3, dev) if pre else torch.empty(0, device=dev)
    t = sign * a[:, None]
    x = (t - (pb.cpu() if pre else 0)).to(act).to(dev)
    y, stat = k.ln_fwd(x, pb, gamma, beta, 0.0)
    assert torch.equal(_d(y), sign.double() * _d(gamma) + _d(beta))
    assert torch.equal(_d(stat), torch.stack([torch.zeros(M), 1 / a], 1).double())
    dy = _ints((M, C), -2, 2, 4, dev, act)
    want_g, want_b = (_d(dy) * sign.double()).sum(0), _d(dy).sum(0)
    for overwrite in (True, False):
        g0 = _ints((2, C), -9, 9, 5, dev)
        dg, db = g0.clone()
        if overwrite:
            dg.fill_(float("nan"))
            db.fill_(float("nan"))
        k.ln_bwd(dy, x, pb, gamma, stat, dg, db, torch.empty(0, device=dev), overwrite)
        assert torch.equal(_d(dg), want_g if overwrite else want_g + _d(g0[0]))
        assert torch.equal(_d(db), want_b if overwrite else want_b + _d(g0[1]))


def check_ln_rounding(k, dev, M, C, pre, act=torch.bfloat16):
    """Random normals against float64.  The kernel rounds: t = x + pre_bias (1); the row sums
    over a chain of n <= 8 * 4 + 6 = 38 additions (a lane's 32 channels, then 6 shuffle steps)
    and a division, for the mean and again for the centred variance; sqrt, reciprocal, the
    product with rstd (3).  Carried through d = t - mean and rstd this is at most
    K = 2 * 38 + 8 = 84 roundings on the magnitude mag = |xhat| + rstd (|t| + mean_c |t|) of
    xhat's computation; the affine is one fused multiply-add, then one bf16 rounding:
        |y - y64| <= 2^-8 |y64| + K u (|gamma| mag + |beta|).
    dx = rstd (g - mean_c(g) - xhat mean_c(g xhat)) multiplies two such factors (2 K):
        |dx - dx64| <= 2^-8 |dx64| + 2 K u rstd (|g| + mean_c|g| + mag mean_c(|g| mag)).
    The parameter gradients stay fp32; their longest addition chain is a lane's 2 trips, the
    block's <= 256 row slots, a fold chunk of <= 3 rows and <= 64 heads: n = 325 on the sum of
    the terms' magnitudes (dgamma's terms carry xhat's K roundings too); dpre_bias sums the
    stored dx, so it is compared with the sum of the returned dx."""
    torch.manual_seed(M + C)
    x = torch.randn(M, C).to(act).to(dev)
    dy = torch.randn(M, C).to(act).to(dev)
    gamma, beta = (torch.rand(C) + 0.5).to(dev), torch.randn(C).to(dev)
    pb = (torch.randn(C) * 0.1).to(dev) if pre else torch.empty(0, device=dev)
    eps, K, n = 1e-6, 84, 325
    t = _d(x) + (_d(pb) if pre else 0)
    mean = t.mean(1, keepdim=True)
    rstd = 1 / torch.sqrt(((t - mean) ** 2).mean(1, keepdim=True) + eps)
    xh, g64, b64 = (t - mean) * rstd, _d(gamma), _d(beta)
    mag = xh.abs() + rstd * (t.abs() + t.abs().mean(1, keepdim=True))
    y, stat = k.ln_fwd(x, pb, gamma, beta, eps)
    y64 = xh * g64 + b64
    assert bool(((_d(y) - y64).abs() <= B * y64.abs() + K * U * (g64.abs() * mag + b64.abs())).all())
    assert torch.allclose(_d(stat), torch.cat([mean, rstd], 1), rtol=K * U, atol=K * U)
    gg = _d(dy) * g64
    dx64 = rstd * (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True))
    dxm = rstd * (gg.abs() + gg.abs().mean(1, keepdim=True) + mag * (gg.abs() * mag).mean(1, keepdim=True))
    dg, db, dp = torch.empty(3, C, device=dev)
    dx = k.ln_bwd(dy, x, pb, gamma, stat, dg, db, dp if pre else torch.empty(0, device=dev), True)
    assert bool(((_d(dx) - dx64).abs() <= B * dx64.abs() + 2 * K * U * dxm).all())
    assert bool(((_d(db) - _d(dy).sum(0)).abs() <= n * U * _d(dy).abs().sum(0)).all())
    assert bool(((_d(dg) - (_d(dy) * xh).sum(0)).abs() <= (n + K) * U * (_d(dy).abs() * mag).sum(0)).all())
    if pre:
        assert bool(((_d(dp) - _d(dx).sum(0)).abs() <= n * U * _d(dx).abs().sum(0)).all())


def check_ln_refusals(k, dev, act=torch.bfloat16):
    for shape in ((4, 12), (4, 2056), (0, 96)):
        x = torch.zeros(shape, dtype=act, device=dev)
        p = torch.zeros(shape[1], device=dev)
        with pytest.raises((RuntimeError, ValueError)):
            k.ln_fwd(x, torch.empty(0, device=dev), p, p, 1e-6)


def check_gelu(k, dev, M, act=torch.bfloat16):
    """a = h Phi(h) and dh = da (Phi(h) + h phi(h)) against float64 erf: one bf16 rounding plus
    the fp32 error of erf, E = 2^-22.  (The fp32 oracle's own largest distance to float64 over
    this grid, measured on the CPU, is |erf32 - erf64| = 5.8e-8 = 2^-24, one ulp at 1; fp32 math
    libraries specify erf to a few ulps rather than correctly rounded, so E is four of them.)  erf's
    error enters a as |h| E / 2 and dh as |da| E / 2; the remaining fp32 operations (4 for a;
    the exponential with its argument's rounding, h^2 / 2 + 2, and 4 more for dh) act on the
    magnitudes of their terms.  With h = 0 the derivative is exactly 0.5, so for even integer
    da the stored dh and every partial sum of dbias are exact."""
    C, E = 40, 2.0 ** -22
    torch.manual_seed(M)
    grid = torch.tensor([0.0, 0.5, -0.5, 3.0, -3.0, 8.0, -8.0])
    h = torch.randn(M, C) * 2
    h.view(-1)[:7] = grid
    h, da = h.to(act).to(dev), torch.randn(M, C).to(act).to(dev)
    h64, da64 = _d(h), _d(da)
    cdf = 0.5 * (1 + torch.erf(h64 / math.sqrt(2)))
    pdf = torch.exp(-0.5 * h64 * h64) / math.sqrt(2 * math.pi)
    a64, der = h64 * cdf, cdf + h64 * pdf
    a = _d(k.gelu_fwd(h))
    assert bool(((a - a64).abs() <= B * a64.abs() + h64.abs() * E / 2 + 4 * U * a64.abs()).all())
    dh = _d(k.gelu_bwd(da, h, torch.empty(0, device=dev)))
    fp32 = da64.abs() * (E / 2 + U * (4 * cdf + (h64 * h64 / 2 + 6) * (h64 * pdf).abs()))
    assert bool(((dh - da64 * der).abs() <= B * (da64 * der).abs() + fp32).all())
    da = (_ints((M, C), -4, 4, 6, dev) * 2).to(act)
    db0 = _ints((C,), -9, 9, 7, dev)
    db = db0.clone()
    dh = k.gelu_bwd(da, torch.zeros(M, C, dtype=act, device=dev), db)
    assert torch.equal(_d(dh), _d(da) / 2) and torch.equal(_d(db), _d(db0) + _d(da).sum(0) / 2)


def check_scale_add(k, dev, M, C, act=torch.bfloat16):
    """Small integers: every product and sum is exact in bf16 / fp32."""
    y, res = _ints((M, C), -4, 4, 1, dev, act), _ints((M, C), -8, 8, 2, dev, act)
    dout, gamma = _ints((M, C), -2, 2, 3, dev, act), _ints((C,), -3, 3, 4, dev)
    assert torch.equal(_d(k.scale_add_fwd(y, gamma, res)), _d(res) + _d(gamma) * _d(y))
    want = (_d(dout) * _d(y)).sum(0)
    for overwrite in (True, False):
        g0 = _ints((C,), -9, 9, 5, dev)
        dg = torch.full_like(g0, float("nan")) if overwrite else g0.clone()
        dy = k.scale_add_bwd(dout, y, gamma, dg, overwrite)
        assert torch.equal(_d(dy), _d(gamma) * _d(dout))
        assert torch.equal(_d(dg), want if overwrite else want + _d(g0))


def check_dw7_exact(k, dev, case):
    """``check_exact`` of test_depthwise_gpu.py at k = 7 with x, dy, w in [-2, 2] and the
    accumulate operand in [-4, 4]: 49 * 4 + 4 = 200 < 256, every bf16 output exact."""
    N, H, W, C = case
    x, w = dg._ints((N, H, W, C), -2, 2, 1, dev), dg._ints((C, 7, 7, 1), -2, 2, 2, dev)
    dy, acc = dg._ints((N, H, W, C), -2, 2, 3, dev), dg._ints((N, H, W, C), -4, 4, 4, dev)
    z, dx, dw = dg._want64(x, w, dy, 1)
    e = torch.empty(0, device=dev)
    assert dg._same(k.dwconv_fwd(x, w, 1, 1, 3, 3, e, e), z)
    assert dg._same(k.dwconv_dgrad(dy, w, H, W, 1, 1, 3, 3), dx)
    assert dg._same(k.dwconv_dgrad(dy, w, H, W, 1, 1, 3, 3, acc.clone()), dx + _d(acc))
    g = torch.full((C, 7, 7, 1), float("nan"), device=dev)
    k.dwconv_wgrad(dy, x, g, 1, 1, 3, 3, overwrite=True)
    assert dg._same(g, dw)
    g0 = dg._ints((C, 7, 7, 1), -9, 9, 5, dev, torch.float32)
    g = g0.clone()
    k.dwconv_wgrad(dy, x, g, 1, 1, 3, 3, overwrite=False)
    assert dg._same(g, dw + _d(g0))


pytestmark = pytest.mark.gpu


def C():
    from mpi_pytorch_amd.ops import _ext
    return _ext.ext()


@pytest.mark.parametrize("pre", [False, True])
@pytest.mark.parametrize("shape", LN_SHAPES)
def test_layer_norm_against_float64(gpu, shape, pre):
    check_ln_exact(C(), gpu, *shape, pre)
    check_ln_rounding(C(), gpu, *shape, pre)


def test_layer_norm_refusals(gpu):
    check_ln_refusals(C(), gpu)


@pytest.mark.parametrize("M", GELU_ROWS)
def test_gelu_against_float64(gpu, M):
    check_gelu(C(), gpu, M)


@pytest.mark.parametrize("shape", SCALE_SHAPES)
def test_scale_add_exact(gpu, shape):
    check_scale_add(C(), gpu, *shape)


@pytest.mark.parametrize("case", DW7_CASES)
def test_depthwise_7x7_exact(gpu, case):
    check_dw7_exact(C(), gpu, case)


def test_block_parity_with_cpu_fp32(gpu):
    from mpi_pytorch_amd.models.convnext import CNBlock
    from mpi_pytorch_amd.parallel.arena import ParamArena
    torch.manual_seed(3)
    bc, bg = CNBlock(96, 0.5), CNBlock(96, 0.5)
    for p in bc.parameters():  # away from the zero biases and unit scales of the initialisation
        if p.dim() == 1:
            torch.nn.init.normal_(p, 0.5, 0.5)
    for m in (bc.block[0], bc.block[3], bc.block[5]):
        m.init_(lambda w: torch.nn.init.normal_(w, std=w[0].numel() ** -0.5))
    bg.load_state_dict(bc.state_dict())
    bg = bg.to(gpu)
    x = torch.randn(2, 14, 14, 96).to(torch.bfloat16)
    res = []
    for blk, dev in ((bc, torch.device("cpu")), (bg, gpu)):
        ParamArena(blk, dev)
        xi = (x.float() if dev.type == "cpu" else x.to(dev)).requires_grad_()
        y = blk(xi)
        torch.manual_seed(4)
        y.backward(torch.randn(y.shape).to(torch.bfloat16).to(dev).to(y.dtype))
        res.append([y.detach(), xi.grad] + [q.grad for q in blk.parameters()])
    names = ["y", "dx"] + [n for n, _ in bc.named_parameters()]
    cos = {n: round(dg._cos(a, b), 4) for n, a, b in zip(names, *res)}
    assert min(cos.values()) >= 0.99, cos


def test_convnext_training_step_bitwise(gpu, monkeypatch):
    from mpi_pytorch_amd.engine import build_training
    from mpi_pytorch_amd.models.convnext import ConvNeXt
    from mpi_pytorch_amd import models
    from mpi_pytorch_amd.parallel import World
    monkeypatch.setenv("MPA_DETERMINISTIC", "1")
    monkeypatch.setitem(models.LN_ARCH, "convnext",
                        ("convnext_reduced", lambda n: ConvNeXt((1, 1, 1, 1), (24, 48, 96, 192), n), 64))
    old = C().deterministic()
    C().set_deterministic(1)
    try:
        g = torch.Generator().manual_seed(1)
        x = (torch.randn(8, 64, 64, 8, generator=g) * (torch.arange(8) < 3)).to(gpu, torch.bfloat16)
        y = torch.randint(0, 10, (8,), generator=g).to(gpu)
        outs = []
        for _ in range(2):
            torch.manual_seed(0)
            model, _opt, step, _ = build_training("convnext", 10, gpu, World(device=gpu), 1e-3)
            loss = step(x, y).clone()
            torch.cuda.synchronize()
            outs.append((loss.cpu(), model._mpa_arena.grad.cpu().clone(),
                         model._mpa_arena.master.cpu().clone()))
        assert bool(torch.isfinite(outs[0][0]).all())
        assert all(torch.equal(a, b) for a, b in zip(*outs))
    finally:
        C().set_deterministic(int(old))
