"""Cosine window attention (wattn.hip's cosine variant) and the continuous position bias (cpb.hip)
against float64, one Swin V2 block pair against the fp32 CPU path, and a bitwise-repeatable
Swin V2 training step.

The checks take the implementation as an argument: ``tests/test_swin_v2_cpu.py`` runs them with
``ref`` on the CPU, which shows that the reference alone meets them."""
import math
import types

import pytest
import torch
import torch.nn.functional as F

import test_attention_gpu as ag
import test_depthwise_gpu as dg
import test_wattn_gpu as wg

U, R, BF = ag.U, ag.R, ag.BF
LN100 = math.log(100.0)

# (B, H, Hf, Wf, ws, shift): 15 padded rows and all nine regions; the 3-wave block with wrap on
# both axes; ws^2 = 16; ws^2 = 64 without padding (the V2 window); wpb = 2 and 130 slab rows (the
# logit-scale column through walk and slab sum)
CASES = [(1, 1, 7, 7, 7, 3), (2, 3, 14, 14, 7, 3), (1, 2, 8, 8, 4, 1), (1, 1, 16, 16, 8, 4),
         (65, 8, 8, 8, 4, 2)]
CPB_CASES = [(H, ws) for H in (1, 3, 24) for ws in (4, 7, 8)]


def _inputs(case, dev):
    """wg._inputs with a bias in [0, 16] and logit scales: head 0 below the clamp, head 1 above"""
    qkv, do, bias = wg._inputs(case, dev)
    ls = torch.linspace(2.0, 3.0, case[1])
    if case[1] > 1:
        ls[1] = 5.0
    return qkv, do, 16 * torch.sigmoid(2 * bias), ls.to(dev)


def _float64(qkv, bias, ls, case):
    q, k, v, add, mask, idx = wg._scores(qkv, bias, case)
    qn, kn = F.normalize(q, dim=-1, eps=1e-12), F.normalize(k, dim=-1, eps=1e-12)
    tau = ag._d(ls).clamp(max=LN100).exp().reshape(1, -1, 1, 1)
    rq, rk = (1 / t.norm(dim=-1, keepdim=True).clamp_min(1e-12) for t in (q, k))
    return qn, kn, rq, rk, v, tau, add, mask, idx


def check_cos_against_float64(k_, dev, case):
    """wg.check_against_float64 re-derived for s = tau c + bias + mask, c = (q . k) rq rk.  c is
    the 32-term fp32 chain (32) times two inverse norms, each a 32-term sum of squares, a square
    root and a reciprocal (2 x 34, the root's halving not counted), two products (2); tau is an
    exp (2) and a product (1); then the two adds (2), minus the maximum or lse (1) and exp
    (<= 2 ulp with its argument):  cp = 108 A + 4, A the largest tau sum_d |q^_d| |k^_d| + |bias| +
    |mask|.  c1 = 2 cp + 3 + 2 S + 2 and the bounds on o, lse and dV are those of the plain kernel.
    Backward, with c2 = 2 cp + 2 S + 6, mag and Gm as there: the dQ operand is dS tau rk_j, which
    replaces the scale's 2 by tau (3), rk (34) and two products (2); t_i = sum_j dS c adds c's own
    error (32 + 68 + 2 = 102, relative to C^ = sum_d |q^| |k^| <= 1), an S-term sum whose S is in c2,
    and the coefficient tau t_i rq_i q^_i (3 + 34 + 34 + 5 = 76); the subtraction and the outer
    product (3) and the outer rq_i (35):  c3 = c2 + 37 + 102 + 76 + 3 + 35 = c2 + 253,
        E = (2 2^-8 + c3 u) mag + 66 Gm u P64,
        |dQ - dQ64| <= 2^-8 |dQ64| + tau rq_i (sum_j E_ij |k^_j| + |q^_i| sum_j E_ij C^_ij),
    the mirror image for dK.  dbias is the plain kernel's bound.  d tau_h is a chain of 16 terms in
    the lane, 4 adds per window of the walk, a 6-step wave sum and the slab rows, at most
    22 + 4 nWt, times tau (4):  |dlogit - dlogit64| <= tau sum ((c2 + 102 + 26 + 4 nWt) u mag +
    66 Gm u P64 + 2^-126 (1 + |dP64| + D)) C^; the clamped head's is exactly 0."""
    B, H, Hf, Wf, ws, shift = case
    S = ws * ws
    qkv, do, bias, ls = _inputs(case, dev)
    qn, kn, rq, rk, v, tau, add, mask, idx = _float64(qkv, bias, ls, case)
    c, chat = qn @ kn.transpose(-1, -2), qn.abs() @ kn.abs().transpose(-1, -2)
    cp = 108 * float((tau * chat + add.abs() + mask.abs()).max()) + 4
    c1 = 2 * cp + 3 + 2 * S + 2
    s = tau * c + add + mask
    p = torch.softmax(s, -1)
    o64 = p @ v
    o, lse = k_.wattn_cos_fwd(qkv, ls, bias, H, Hf, Wf, ws, shift)
    assert o.shape == (B * Hf * Wf, H * 32) and lse.shape == (s.shape[0], H, S)
    assert bool(((wg._textbook(o, case, 32) - o64).abs() <= R * o64.abs() + (R + c1 * U) * (p @ v.abs())).all())
    assert torch.allclose(ag._d(lse), torch.logsumexp(s, -1), rtol=0, atol=(c1 + 2) * U * (1 + float(s.abs().max())))
    # backward, lse as given
    d64 = wg._textbook(do, case, 32)
    p = torch.exp(s - ag._d(lse)[..., None])
    dp = d64 @ v.transpose(-1, -2)
    dsum = (p * dp.abs()).sum(-1, keepdim=True)
    ds, mag = p * (dp - (p * dp).sum(-1, keepdim=True)), p * (dp.abs() + dsum)
    gm = float((d64.abs() @ v.abs().transpose(-1, -2)).max())
    c2 = 2 * cp + 2 * S + 6
    dbias, dls = torch.full_like(bias, float("nan")), torch.full_like(ls, float("nan"))
    dqkv = k_.wattn_cos_bwd(do, qkv, lse, ls, bias, dbias, dls, H, Hf, Wf, ws, shift, True)
    dq, dk, dv = (wg._textbook(dqkv[:, i * H * 32:(i + 1) * H * 32], case, 32) for i in range(3))
    dv64 = p.transpose(-1, -2) @ d64
    assert bool(((dv - dv64).abs() <= R * dv64.abs() + (R + c1 * U) * (p.transpose(-1, -2) @ d64.abs())).all())
    t, u = (ds * c).sum(-1, keepdim=True), (ds * c).sum(-2).unsqueeze(-1)
    dq64, dk64 = tau * rq * (ds @ kn - t * qn), tau * rk * (ds.transpose(-1, -2) @ qn - u * kn)
    E = (2 * R + (c2 + 253) * U) * mag + 66 * gm * U * p
    ec = E * chat
    assert bool(((dq - dq64).abs() <= R * dq64.abs() + tau * rq * (E @ kn.abs() + qn.abs() * ec.sum(-1, keepdim=True))).all())
    assert bool(((dk - dk64).abs() <= R * dk64.abs()
                 + tau * rk * (E.transpose(-1, -2) @ qn.abs() + kn.abs() * ec.sum(-2).unsqueeze(-1))).all())
    nb, nwt = (2 * ws - 1) ** 2, s.shape[0]
    fold = lambda x: torch.zeros(H, nb, dtype=torch.float64).index_add_(1, idx.reshape(-1), x.sum(0).reshape(H, S * S))
    tiny = 2.0 ** -126 * (1 + dp.abs() + dsum)
    berr = fold((c2 + nwt + S) * U * mag + 66 * gm * U * p + tiny)
    assert bool(((ag._d(dbias).reshape(H, nb) - fold(ds)).abs() <= berr).all())
    live = ag._d(ls) < LN100
    dl64 = tau.reshape(-1) * t.sum((0, 2, 3)) * live
    lerr = tau.reshape(-1) * (((c2 + 128 + 4 * nwt) * U * mag + 66 * gm * U * p + tiny) * chat).sum((0, 2, 3))
    assert bool(((ag._d(dls) - dl64).abs() <= lerr).all()) and bool((ag._d(dls)[~live] == 0).all())
    assert H == 1 or (not bool(live[1]) and bool(live[0]) and float(dl64[0].abs()) > 0)
    # accumulate into the sinks, and two runs are bitwise equal
    acc, lacc = torch.ones_like(bias), torch.ones_like(ls)
    dqkv2 = k_.wattn_cos_bwd(do, qkv, lse, ls, bias, acc, lacc, H, Hf, Wf, ws, shift, False)
    assert torch.equal(dqkv2, dqkv) and torch.equal(acc, 1 + dbias) and torch.equal(lacc, 1 + dls)
    assert all(torch.equal(a, b) for a, b in zip(k_.wattn_cos_fwd(qkv, ls, bias, H, Hf, Wf, ws, shift), (o, lse)))


def check_zero_row(k_, dev):
    """A real token whose q and k are all zeros has cosine 0 with everything: o is finite, and
    that token's o is softmax(bias + mask) v of its row within the forward bound (cp with the
    cosine's terms left in: they bound the other rows' error too)."""
    case = (1, 1, 7, 7, 7, 0)
    qkv, _, bias, ls = _inputs(case, dev)
    qkv[24, :64] = 0
    qn, _, _, _, v, tau, add, mask, _ = _float64(qkv, bias, ls, case)
    o = wg._textbook(k_.wattn_cos_fwd(qkv, ls, bias, 1, 7, 7, 7, 0)[0], case, 32)
    assert bool(torch.isfinite(o).all()) and float(qn[0, 0, 24].abs().max()) == 0
    p = torch.softmax((add + mask)[0, 0, 24], -1)
    c1 = 2 * (108 * float((tau + add.abs()).max()) + 4) + 3 + 2 * 49 + 2
    assert bool(((o[0, 0, 24] - p @ v[0, 0]).abs() <= R * (p @ v[0, 0]).abs() + (R + c1 * U) * (p @ v[0, 0].abs())).all())


def check_cpb(k_, dev, H, ws):
    """The table and the MLP's gradients against float64 autograd over coordinates built the way
    torchvision builds them.  A coordinate is a division, a log2 (<= 2 ulp), an add and a
    division: 6 u; a hidden unit two multiply-adds: (6 + 2) u Hm, Hm = |w1| |coord| + |b1|; z a
    512-term sum: 520 u sum_u |w2| Hm; the sigmoid's slope is at most 1/4 and exp, add and divide
    cost 4 u:  eb = 16 (520 u sum_u |w2| Hm / 4 + 4 u).  Backward: the slope b (1 - b / 16) <= 4 is
    taken from the stored table (eb) in three roundings: Ez = |dbias| (eb + 16 u); the sums over
    T entries, H heads and the products add (T + 9) u, (H + 1) u, (T + 7) u of the absolute
    terms; a unit whose pre-activation is within its own error 8 u Hm of zero may be gated either way."""
    gen = torch.Generator().manual_seed(100 * H + ws)
    w1, b1 = torch.randn(512, 2, generator=gen), torch.randn(512, generator=gen) * 0.5
    w2, db = torch.randn(H, 512, generator=gen) * 0.1, torch.randn(H * (2 * ws - 1) ** 2, generator=gen)
    ch = torch.arange(-(ws - 1), ws, dtype=torch.float32)
    table = torch.stack(torch.meshgrid([ch, ch], indexing="ij")).permute(1, 2, 0).contiguous().unsqueeze(0)
    table[:, :, :, 0] /= ws - 1
    table[:, :, :, 1] /= ws - 1
    table *= 8
    table = torch.sign(table) * torch.log2(torch.abs(table) + 1.0) / 3.0
    co = table.double().reshape(-1, 2)
    p64 = [t.double().requires_grad_() for t in (w1, b1, w2)]
    pre = co @ p64[0].t() + p64[1]
    b64 = (16 * torch.sigmoid(torch.relu(pre) @ p64[2].t())).t()          # [H, T]
    T = co.shape[0]
    hm = co.abs() @ w1.double().abs().t() + b1.double().abs()             # [T, 512]
    eb = 16 * (520 * U * (hm @ w2.double().abs().t()).t() / 4 + 4 * U)
    dv = [t.to(dev) for t in (w1, b1, w2)]
    bias = k_.cpb_fwd(*dv, H, ws)
    assert bias.shape == (H * T,) and bias.dtype == torch.float32
    assert bool(((ag._d(bias).reshape(H, T) - b64).abs() <= eb).all())
    b64.backward(db.double().reshape(H, T))
    dz = (db.double().reshape(H, T) * b64 * (1 - b64 / 16)).detach()
    ez = db.double().reshape(H, T).abs() * (eb + 16 * U)
    hid, w2a = torch.relu(pre).detach(), w2.double().abs()
    dh_all = dz.t() @ w2.double()
    eh = ez.t() @ w2a + (H + 1) * U * (dz.abs().t() @ w2a) + (pre.detach().abs() <= 8 * U * hm) * dh_all.abs()
    dh = (dh_all * (pre > 0)).abs()
    bounds = [eh.t() @ co.abs() + (T + 7) * U * (dh.t() @ co.abs()), eh.sum(0) + T * U * dh.sum(0),
              ez @ hid + dz.abs() @ (8 * U * hm) + (T + 9) * U * (dz.abs() @ hid)]
    got = [torch.full_like(t, float("nan")) for t in dv]
    k_.cpb_bwd(db.to(dev), bias, *dv, *got, H, ws, True)
    for g, p, bound in zip(got, p64, bounds):
        assert bool(((ag._d(g) - p.grad).abs() <= bound + 2.0 ** -126).all())
    acc = [torch.ones_like(t) for t in dv]
    k_.cpb_bwd(db.to(dev), bias, *dv, *acc, H, ws, False)
    assert all(torch.equal(a, 1 + g) for a, g in zip(acc, got)) and torch.equal(k_.cpb_fwd(*dv, H, ws), bias)


def check_cos_refusals(k_, dev):
    cos = lambda qkv, bias, H, *geom: k_.wattn_cos_fwd(qkv, torch.zeros(H, device=qkv.device), bias, H, *geom)
    wg.check_wattn_refusals(types.SimpleNamespace(wattn_fwd=cos), dev)  # a valid logit scale, wg's cases
    z = lambda *shape, dt=BF: torch.zeros(*shape, dtype=dt, device=dev)
    for ls in (z(2, dt=torch.float32), z(1, dt=torch.float64), z(1)):  # length, dtype
        with pytest.raises((RuntimeError, ValueError)):
            k_.wattn_cos_fwd(z(49, 96), ls, z(169, dt=torch.float32), 1, 7, 7, 7, 0)
    f = lambda *shape: z(*shape, dt=torch.float32)
    for w1, b1, w2, H, ws in ((f(512, 3), f(512), f(3, 512), 3, 7), (f(512, 2), f(256), f(3, 512), 3, 7),
                              (f(512, 2), f(512), f(4, 512), 3, 7), (f(512, 2), f(512), f(3, 512), 3, 1),
                              (f(512, 2), f(512), f(3, 512), 3, 9), (f(512, 2), f(512), z(3, 512), 3, 7)):
        with pytest.raises((RuntimeError, ValueError)):
            k_.cpb_fwd(w1, b1, w2, H, ws)


pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CASES)
def test_cosine_window_attention_against_float64(gpu, case):
    check_cos_against_float64(ag.C(), gpu, case)


def test_cosine_window_attention_zero_row(gpu):
    check_zero_row(ag.C(), gpu)


@pytest.mark.parametrize("H,ws", CPB_CASES)
def test_position_bias_against_float64(gpu, H, ws):
    check_cpb(ag.C(), gpu, H, ws)


def test_cosine_window_attention_refusals(gpu):
    check_cos_refusals(ag.C(), gpu)


def test_swin_v2_block_pair_parity_with_cpu_fp32(gpu):
    from mpi_pytorch_amd.models.swin import SwinBlockV2
    from mpi_pytorch_amd.parallel.arena import ParamArena
    torch.manual_seed(3)
    mk = lambda: torch.nn.Sequential(SwinBlockV2(64, 2, 4, 0), SwinBlockV2(64, 2, 4, 2))
    bc, bg = mk(), mk()
    for p in bc.parameters():  # away from the zero biases and unit scales of the initialisation
        if p.dim() == 1:
            torch.nn.init.normal_(p, 0.5, 0.5)
    bc.load_state_dict(bc.state_dict())  # (the import holds the k third of the qkv bias at zero)
    bg.load_state_dict(bc.state_dict())
    bg = bg.to(gpu)
    x = torch.randn(2 * 8 * 8, 64).to(BF)
    res = []
    for blk, dev in ((bc, torch.device("cpu")), (bg, gpu)):
        ParamArena(blk, dev)
        xi = (x.float() if dev.type == "cpu" else x.to(dev)).requires_grad_()
        y = blk[1](blk[0](xi * 1, 8, 8), 8, 8)
        torch.manual_seed(4)
        y.backward(torch.randn(y.shape).to(BF).to(dev).to(y.dtype))
        res.append([y.detach(), xi.grad] + [q.grad for q in blk.parameters()])
    names = ["y", "dx"] + [n for n, _ in bc.named_parameters()]
    cos = {n: round(dg._cos(a, b), 4) for n, a, b in zip(names, *res)}
    assert min(cos.values()) >= 0.99, cos


def test_swin_v2_training_step_bitwise(gpu, monkeypatch):
    from mpi_pytorch_amd.engine import build_training
    from mpi_pytorch_amd.models.swin import PatchMergingV2, SwinBlockV2, SwinTransformer
    from mpi_pytorch_amd import models
    from mpi_pytorch_amd.parallel import World
    monkeypatch.setitem(models.WINDOW_V2_ARCH, "swin_v2", (
        "swin_v2_reduced", lambda n: SwinTransformer(4, 64, (1, 1), (2, 4), 4, n, SwinBlockV2, PatchMergingV2), 32))
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(8, 32, 32, 8, generator=g) * (torch.arange(8) < 3)).to(gpu, BF)
    y = torch.randint(0, 10, (8,), generator=g).to(gpu)
    outs = []
    for _ in range(2):
        torch.manual_seed(0)
        model, _opt, step, _ = build_training("swin_v2", 10, gpu, World(device=gpu), 1e-3)
        loss = step(x, y).clone()
        torch.cuda.synchronize()
        outs.append((loss.cpu(), model._mpa_arena.grad.cpu().clone(), model._mpa_arena.master.cpu().clone()))
    assert bool(torch.isfinite(outs[0][0]).all()) and float(outs[0][1].abs().sum()) > 0
    assert all(torch.equal(a, b) for a, b in zip(*outs))
