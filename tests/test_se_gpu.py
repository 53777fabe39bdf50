"""Squeeze-excite / activation-gate kernels (csrc/kernels/se.hip) against float64 formulas
written out here, two MobileNetV3 SE blocks against the fp32 CPU path, and a bitwise-repeatable
MobileNetV3 training step.

The checks take the implementation as an argument: ``tests/test_mobilenetv3_cpu.py`` runs them
with ``ref`` on the CPU, which shows that the reference alone meets them."""
import math

import pytest
import torch
import torch.nn.functional as F

# (N, H, W, C, Cs)
EXACT_CASES = [(2, 4, 16, 8, 8),      # one vector, one slab
               (3, 8, 8, 72, 24),     # 9 vectors: a non-power-of-two vector count
               (2, 32, 32, 24, 8)]    # several slabs per image
ROUNDING_CASES = [(3, 7, 7, 960, 240),   # several trips of the gate loops, odd H W
                  (3, 28, 28, 72, 24),
                  (2, 14, 14, 8, 8)]
U = 2.0 ** -24


def _ints(shape, lo, hi, seed, dev, dtype=torch.bfloat16, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(lo, hi + 1, shape, generator=g) * scale).to(dtype).to(dev)


def _d(t):
    return t.double().cpu()


def _act(t, act):
    return torch.relu(t) if act == 1 else t * torch.clamp(t + 3, 0, 6) / 6


def _der(t, act):
    if act == 1:
        return (t > 0).double()
    return torch.where(t <= -3, 0.0, torch.where(t >= 3, 1.0, t / 3 + 0.5))


def _plan(N, HW, C):
    """se_plan.h: (pixel slots per block, pixels per slab, slabs per image)."""
    cv = C // 8
    chunks = -(-cv // 128)
    nslots = 256 // -(-cv // chunks)
    want = max(1, min(-(-2048 // (N * chunks)), -(-HW // (nslots * 4))))
    pps = -(-HW // want)
    return nslots, pps, -(-HW // pps)


def _chain(N, HW, C):
    """Longest addition chain of a streaming reduction: a thread's pixels, the block's slots,
    the image's slabs."""
    nslots, pps, slabs = _plan(N, HW, C)
    return -(-pps // nslots) + nslots + slabs


def _rows_chain(I):
    """rows_matvec over I inputs: (8 FMAs + 1 add) per trip, the shuffle tree, the bias."""
    iv = I // 8
    G = min(64, 1 << (iv - 1).bit_length())
    return 9 * -(-iv // G) + int(math.log2(G)) + 1


def _cols_chain(R, I):
    """cols_matvec over R rows of I columns: a slot's rows, then the slots."""
    nslots = 256 // (I // 8)
    return -(-R // nslots) + nslots


def _le(got, want, bound):
    return bool(((_d(got) - want).abs() <= bound).all())


def check_exact(k, dev, case):
    """Small integers and halves: t, every product and every partial sum is an exact fp32 value
    (|t| <= 11, |g xhat| <= 72 in quarters, sums below 2^24 quarters), so any summation order
    gives the float64 result."""
    N, H, W, C, Cs = case
    z, du = _ints((N, H, W, C), -4, 4, 1, dev), _ints((N, H, W, C), -4, 4, 2, dev)
    aff = torch.stack([_ints((C,), -2, 2, 3, dev, torch.float32),
                       _ints((C,), -3, 3, 4, dev, torch.float32)])
    gate = _ints((N, C), 0, 2, 5, dev, torch.float32, 0.5)
    dpool = _ints((N, C), -4, 4, 6, dev, torch.float32, 0.5)
    mean = _ints((C,), -2, 2, 7, dev, torch.float32)
    rstd = 2.0 ** _ints((C,), -1, 1, 8, dev, torch.float32)
    t = _d(z) * _d(aff[0]) + _d(aff[1])
    a = torch.relu(t)
    g4, d4 = _d(gate)[:, None, None, :], _d(dpool)[:, None, None, :]
    assert torch.equal(_d(k.act_pool(z, aff, 1)), a.mean((1, 2)))
    assert torch.equal(_d(k.act_gate_fwd(z, aff, 1, gate)), a * g4)
    assert torch.equal(_d(k.act_gate_bwd_pool(du, z, aff, 1)), (_d(du) * a).sum((1, 2)))
    g = (_d(du) * g4 + d4) * (t > 0)
    xh = (_d(z) - _d(mean)) * _d(rstd)
    want = torch.stack([g.sum((0, 1, 2)), (g * xh).sum((0, 1, 2))])
    assert torch.equal(_d(k.act_gate_bwd_sums(du, z, aff, 1, gate, dpool, mean, rstd)), want)
    dpre = _ints((N, C), -4, 4, 9, dev, torch.float32)
    inp = _ints((N, Cs), -4, 4, 10, dev, torch.float32)
    dw, db = _d(dpre).t() @ _d(inp), _d(dpre).sum(0)
    gw = torch.full((C, 1, 1, Cs), float("nan"), device=dev)
    gb = torch.full((C,), float("nan"), device=dev)
    k.se_fc_wgrad(dpre, inp, gw, gb, overwrite=True)
    assert torch.equal(_d(gw).reshape(C, Cs), dw) and torch.equal(_d(gb), db)
    k.se_fc_wgrad(dpre, inp, gw, gb, overwrite=False)
    assert torch.equal(_d(gw).reshape(C, Cs), 2 * dw) and torch.equal(_d(gb), 2 * db)


def rounding_inputs(dev, case, seed=7):
    N, H, W, C, Cs = case
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    f = lambda t: t.to(dev)  # noqa: E731
    return dict(
        z=f(r(N, H, W, C).bfloat16()), du=f(r(N, H, W, C).bfloat16()),
        aff=f(torch.stack([torch.rand(C, generator=g) + 0.5, r(C) * 0.5])),
        w1=f((r(Cs, 1, 1, C) / C ** 0.5).bfloat16()), b1=f(r(Cs) * 0.1),
        w2=f((r(C, 1, 1, Cs) / Cs ** 0.5).bfloat16()), b2=f(r(C) * 0.5),
        pooled=f(r(N, C)), h=f(torch.relu(r(N, Cs))), gate=f(torch.clamp(r(N, C) * 0.4 + 0.5, 0, 1)),
        dgate=f(r(N, C)), dpool=f(r(N, C) * 0.1), mean=f(r(C) * 0.3),
        rstd=f(torch.rand(C, generator=g) + 0.5), gamma=f(torch.rand(C, generator=g) + 0.5),
        sums=f(r(2, C) * N * H * W * 0.1))


def check_rounding(k, dev, act, case):
    """Random-normal operands against float64.  Bounds: one bf16 rounding (2^-8 relative) where
    the output is bf16, plus n 2^-24 times the sum of the terms' magnitudes, n counted from
    se.hip:

    * t is one FMA (1 rounding on T = |aff0 z| + |aff1|); hardswish adds t + 3, two products and
      the rounded constant 1/6, and is 1.5-Lipschitz in t: act(t) is within 6 u T, |act(t)| <= T;
    * a streaming reduction adds ``_chain`` times (a thread's pixels, the block's slots, the
      image's slabs: 13 for 7 x 7 x 960, 39 for 28 x 28 x 72, 258 for 14 x 14 x 8), the pool one
      more for 1 / HW; the BN sums add the fold of N slabs rows (no more than N slabs);
    * a gate row is (8 FMAs + 1 add) per trip, log2(lanes) shuffle adds and the bias
      (``_rows_chain``: 25 over 960 inputs); hardsigmoid adds 3 roundings on a value <= 1 and
      has slope 1/6, so h's bound enters the gate through |W2| / 6;
    * a transposed product is a slot's rows then the slots (``_cols_chain``);
    * g = (du gate + dpool) act'(t): one FMA, the derivative (t / 3 + 0.5: an FMA with a rounded
      constant, 1/3-Lipschitz in t, <= 1.5) and one product: within u G0 (6 + T / 3) with
      G0 = |du gate| + |dpool|; xhat is two roundings on X = (|z| + |mean|) rstd;
    * dz = k1 ((g - m1) - xhat m2): k1, m1, m2 one or two roundings each, two subtractions, one
      product: 8 u on k1 (|g| + |m1| + X |m2|)."""
    N, H, W, C, Cs = case
    HW = H * W
    d = rounding_inputs(dev, case)
    z, du, aff = d["z"], d["du"], d["aff"]
    z64, du64 = _d(z), _d(du)
    t = z64 * _d(aff[0]) + _d(aff[1])
    T = z64.abs() * _d(aff[0]).abs() + _d(aff[1]).abs()
    a = _act(t, act)
    chain = _chain(N, HW, C)
    # the pools
    assert _le(k.act_pool(z, aff, act), a.mean((1, 2)), (chain + 1 + 6) * U * T.mean((1, 2)))
    assert _le(k.act_gate_bwd_pool(du, z, aff, act), (du64 * a).sum((1, 2)),
               (chain + 6) * U * (du64.abs() * T).sum((1, 2)))
    # forward scale; an empty gate is a gate of ones, bitwise
    g4 = _d(d["gate"])[:, None, None, :]
    want = a * g4
    assert _le(k.act_gate_fwd(z, aff, act, d["gate"]), want, 2.0 ** -8 * want.abs() + 8 * U * T * g4)
    e = torch.empty(0, device=dev)
    ones = torch.ones(N, C, device=dev)
    assert torch.equal(k.act_gate_fwd(z, aff, act, e), k.act_gate_fwd(z, aff, act, ones))
    # gate forward
    w1, w2 = _d(d["w1"]).reshape(Cs, C), _d(d["w2"]).reshape(C, Cs)
    s64, b1, b2 = _d(d["pooled"]), _d(d["b1"]), _d(d["b2"])
    h64 = torch.relu(s64 @ w1.t() + b1)
    gate64 = torch.clamp(h64 @ w2.t() + b2 + 3, 0, 6) / 6
    eh = _rows_chain(C) * U * (s64.abs() @ w1.abs().t() + b1.abs())
    eg = (eh @ w2.abs().t() + _rows_chain(Cs) * U * (h64 @ w2.abs().t() + b2.abs())) / 6 + 3 * U
    h, gate = k.se_gate(d["pooled"], d["w1"], d["b1"], d["w2"], d["b2"])
    assert _le(h, h64, eh) and _le(gate, gate64, eg)
    # gate backward
    dg, hh, gg = _d(d["dgate"]), _d(d["h"]), _d(d["gate"])
    p2 = torch.where((gg > 0) & (gg < 1), dg / 6, 0.0)
    p1 = (p2 @ w2) * (hh > 0)
    e2 = 2 * U * p2.abs()
    e1 = e2 @ w2.abs() + _cols_chain(C, Cs) * U * (p2.abs() @ w2.abs())
    e0 = (e1 @ w1.abs() + (_cols_chain(Cs, C) + 1) * U * (p1.abs() @ w1.abs())) / HW
    dpre2, dpre1, dpool = k.se_gate_bwd(d["dgate"], d["h"], d["gate"], d["w1"], d["w2"], 1.0 / HW)
    assert _le(dpre2, p2, e2) and _le(dpre1, p1, e1) and _le(dpool, (p1 @ w1) / HW, e0)
    # fc weight gradient (N FMAs per element)
    gw = torch.empty(C, 1, 1, Cs, device=dev)
    k.se_fc_wgrad(d["dgate"], d["h"], gw, e, overwrite=True)
    assert _le(gw.reshape(C, Cs), dg.t() @ hh, N * U * (dg.abs().t() @ hh))
    # BN sums and input gradient
    d4 = _d(d["dpool"])[:, None, None, :]
    mean, rstd = _d(d["mean"]), _d(d["rstd"])
    g = (du64 * g4 + d4) * _der(t, act)
    G0 = du64.abs() * g4 + d4.abs()
    eg = U * G0 * (6 + T / 3)
    xh, X = (z64 - mean) * rstd, (z64.abs() + mean.abs()) * rstd
    n = chain + N * _plan(N, HW, C)[2]
    want = torch.stack([g.sum((0, 1, 2)), (g * xh).sum((0, 1, 2))])
    bound = torch.stack([(eg + n * U * 1.5 * G0).sum((0, 1, 2)),
                         ((eg + (n + 2) * U * 1.5 * G0) * X).sum((0, 1, 2))])
    args = (du, z, aff, act, d["gate"], d["dpool"], d["mean"], d["rstd"])
    assert _le(k.act_gate_bwd_sums(*args), want, bound)
    assert torch.equal(k.act_gate_bwd_sums(du, z, aff, act, e, e, d["mean"], d["rstd"]),
                       k.act_gate_bwd_sums(du, z, aff, act, ones, e, d["mean"], d["rstd"]))
    M = N * HW
    m1, m2, k1 = _d(d["sums"][0]) / M, _d(d["sums"][1]) / M, _d(d["gamma"]) * rstd
    want = k1 * (g - m1 - xh * m2)
    bound = 2.0 ** -8 * want.abs() + k1 * (eg + 8 * U * (1.5 * G0 + m1.abs() + X * m2.abs()))
    assert _le(k.act_gate_bwd_dx(*args, d["gamma"], d["sums"]), want, bound)
    assert _le(k.act_gate_bwd_dx(du, z, aff, act, d["gate"], d["dpool"], e, e, e, e), g,
               2.0 ** -8 * g.abs() + eg)
    assert torch.equal(k.act_gate_bwd_dx(du, z, aff, act, e, e, e, e, e, e),
                       k.act_gate_bwd_dx(du, z, aff, act, ones, e, e, e, e, e))


def check_hardswish_points(k, dev):
    """t = -3, 0, 3 exactly: forward 0, 0, 3; the derivative is torch's own at those points (only
    the open interval (-3, 3) takes t / 3 + 0.5: torch gives 0, 0.5, 1)."""
    z = torch.tensor([-3.0, 0.0, 3.0]).repeat_interleave(8).reshape(1, 3, 1, 8).bfloat16().to(dev)
    aff = torch.stack([torch.ones(8), torch.zeros(8)]).to(dev)
    e = torch.empty(0, device=dev)
    assert torch.equal(_d(k.act_gate_fwd(z, aff, 2, e)).flatten()[::8], torch.tensor([0.0, 0.0, 3.0]).double())
    t = torch.tensor([-3.0, 0.0, 3.0], dtype=torch.float64, requires_grad=True)
    (want,) = torch.autograd.grad(F.hardswish(t).sum(), t)
    got = k.act_gate_bwd_dx(torch.ones_like(z), z, aff, 2, e, e, e, e, e, e)
    assert torch.equal(_d(got).flatten()[::8], want), (got.flatten()[::8], want)


def check_repeatable(k, dev):
    d = rounding_inputs(dev, ROUNDING_CASES[0])
    N, H, W, C, Cs = ROUNDING_CASES[0]

    def run():
        gw, gb = torch.empty(C, 1, 1, Cs, device=dev), torch.empty(C, device=dev)
        k.se_fc_wgrad(d["dgate"], d["h"], gw, gb, overwrite=True)
        return [k.act_pool(d["z"], d["aff"], 2), k.act_gate_bwd_pool(d["du"], d["z"], d["aff"], 2),
                k.act_gate_bwd_sums(d["du"], d["z"], d["aff"], 2, d["gate"], d["dpool"], d["mean"],
                                    d["rstd"]), gw, gb,
                *k.se_gate(d["pooled"], d["w1"], d["b1"], d["w2"], d["b2"]),
                *k.se_gate_bwd(d["dgate"], d["h"], d["gate"], d["w1"], d["w2"], 1.0 / (H * W))]
    assert all(torch.equal(a, b) for a, b in zip(run(), run()))


pytestmark = pytest.mark.gpu


def C():
    from mpi_pytorch_amd.ops import _ext
    return _ext.ext()


@pytest.mark.parametrize("case", EXACT_CASES)
def test_exact_against_float64(gpu, case):
    check_exact(C(), gpu, case)


@pytest.mark.parametrize("case", ROUNDING_CASES)
@pytest.mark.parametrize("act", [1, 2])
def test_rounding_against_float64(gpu, act, case):
    check_rounding(C(), gpu, act, case)


def test_hardswish_points(gpu):
    check_hardswish_points(C(), gpu)


def test_reductions_repeat_bitwise(gpu):
    check_repeatable(C(), gpu)


def _cos(a, b):
    a, b = a.double().cpu().flatten(), b.double().cpu().flatten()
    return float(a @ b / (a.norm() * b.norm() + 1e-30))


# features.13 (hardswish, 112 -> 160, k5, s2, exp 672) and features.5 (ReLU, 40 -> 40, k5, s1,
# exp 120, residual)
@pytest.mark.parametrize("cfg", [(112, 5, 672, 160, True, True, 2), (40, 5, 120, 40, True, False, 1)])
def test_block_parity_with_cpu_fp32(gpu, cfg):
    from mpi_pytorch_amd.models.mobilenetv3 import _InvertedResidual
    from mpi_pytorch_amd.parallel.arena import ParamArena
    torch.manual_seed(3)
    bc, bg = _InvertedResidual(*cfg), _InvertedResidual(*cfg)
    # BN affines away from their initial (1, 0), as in test_depthwise_gpu.py
    for m in bc.modules():
        if type(m).__name__ == "BatchNorm2d":
            torch.nn.init.uniform_(m.weight, 0.5, 1.5)
            torch.nn.init.normal_(m.bias, 0.0, 0.5)
    bg.load_state_dict(bc.state_dict())
    bg = bg.to(gpu)
    x = torch.randn(4, 14, 14, cfg[0]).to(torch.bfloat16)
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
    assert any("fc1.bias" in n for n in names)
    cos = {n: round(_cos(a, b), 4) for n, a, b in zip(names, *res)}
    assert min(cos.values()) >= 0.99, cos


def test_mobilenet_v3_training_steps_bitwise(gpu, monkeypatch):
    from mpi_pytorch_amd.engine import build_training
    from mpi_pytorch_amd.ops.functional import DropoutRNG
    from mpi_pytorch_amd.parallel import World
    monkeypatch.setenv("MPA_DETERMINISTIC", "1")
    old = C().deterministic()
    C().set_deterministic(1)
    try:
        g = torch.Generator().manual_seed(1)
        x = (torch.randn(8, 64, 64, 8, generator=g) * (torch.arange(8) < 3)).to(gpu, torch.bfloat16)
        y = torch.randint(0, 10, (8,), generator=g).to(gpu)
        outs = []
        rng = DropoutRNG.state()  # (the classifier's dropout draws from a process-wide counter)
        for _ in range(2):
            torch.manual_seed(0)
            DropoutRNG.set_state(rng)
            model, _opt, step, _ = build_training("mobilenet_v3", 10, gpu, World(device=gpu), 1e-3)
            losses = torch.stack([step(x, y).clone() for _ in range(3)])
            torch.cuda.synchronize()
            outs.append((losses.cpu(), model._mpa_arena.master.cpu().clone()))
        assert bool(torch.isfinite(outs[0][0]).all())
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    finally:
        C().set_deterministic(int(old))
