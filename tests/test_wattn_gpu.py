"""Shifted-window attention (csrc/kernels/wattn.hip) and ``unpatchify`` against float64, one
Swin block pair against the fp32 CPU path, and a bitwise-repeatable Swin training step.

The checks take the implementation as an argument: ``tests/test_swin_cpu.py`` runs them with
``ref`` on the CPU, which shows that the reference alone meets them."""
import math

import pytest
import torch

import test_attention_gpu as ag
import test_depthwise_gpu as dg
from mpi_pytorch_amd.ops import ref

U, R, BF = ag.U, ag.R, ag.BF
SCALE = 32 ** -0.5

# (B, H, Hf, Wf, ws, shift): one window with 15 padded keys / query rows; all nine regions in one
# window, every row wraps; the 3-wave block, wrap on both axes; non-square map, 4-wave block;
# 1-wave blocks; ws^2 = 16 (one MFMA tile, three padded key sub-tiles); ws^2 = 64 (no padding); two
# head groups per window; and a long walk: wattn_plan gives 4 waves, 2 head groups, 260 windows,
# wpb = 2 windows per backward block, 130 slab rows
CASES = [(1, 1, 7, 7, 7, 0), (1, 1, 7, 7, 7, 3), (2, 3, 14, 14, 7, 3), (1, 4, 14, 7, 7, 2),
         (1, 5, 7, 14, 7, 3), (1, 2, 8, 8, 4, 1), (1, 1, 16, 16, 8, 4), (2, 6, 14, 14, 7, 0),
         (65, 8, 8, 8, 4, 2)]
UNIFORM_CASES = [(1, 2, 8, 8, 4, 0), (1, 1, 16, 16, 8, 0)]
UNPATCH_CASES = ag.PATCH_CASES + [(2, 8, 12, 96, 2)]


def _inputs(case, dev, gain=1.0):
    B, H, Hf, Wf, ws, shift = case
    gen = torch.Generator().manual_seed(sum(p * v for p, v in zip((1, 7, 31, 57, 101, 211), case)))
    qkv = (torch.randn(B * Hf * Wf, 3 * H * 32, generator=gen) * gain).to(BF)
    do = torch.randn(B * Hf * Wf, H * 32, generator=gen).to(BF)
    bias = torch.randn(H * (2 * ws - 1) ** 2, generator=gen) * 0.5
    return qkv.to(dev), do.to(dev), bias.to(dev)


def _textbook(t, case, width):
    """[B nW, H, ws^2, width] float64 windows of rows t: roll, then reshape / permute partition"""
    _, H, Hf, Wf, ws, shift = case
    return ref.window_partition(ag._d(t), Hf, Wf, ws, shift).reshape(-1, ws * ws, H, width).transpose(1, 2)


def _scores(qkv, bias, case):
    """q, k, v and the float64 scores from the explicit index table and mask tensor"""
    B, H, Hf, Wf, ws, shift = case
    q, k, v = (_textbook(qkv[:, i * H * 32:(i + 1) * H * 32], case, 32) for i in range(3))
    idx = ref.swin_relative_index(ws)
    add = ag._d(bias).reshape(H, -1)[:, idx.reshape(-1)].reshape(1, H, ws * ws, ws * ws)
    mask = ref.swin_shift_mask(Hf, Wf, ws, shift).double().repeat(B, 1, 1)[:, None]
    return q, k, v, add, mask, idx


def check_against_float64(k_, dev, case):
    """Random bf16 normals, bias table N(0, 0.5), against float64 of the textbook formulation.
    The bounds are check_rounding's (test_attention_gpu.py), re-derived for this kernel.  A score
    is a 32-term fp32 chain (32), times 32^-1/2 as one fp32 constant (its rounding and the
    product's: 2), plus bias and plus mask (two adds: 2), minus the maximum or lse (1), through exp
    (<= 2 ulp with its argument): relative error cp u of every P, cp = 38 A + 4, A the largest
    sum_d |q_d| |k_d| 32^-1/2 + |bias| + |mask|.  Forward, S = ws^2 keys in one tile: the error
    enters numerator and row sum (2 cp), the form's one-tile term (3 T, T = 1: nothing is rescaled),
    two S-term fp32 sums (2 S), the division and the lse sum (2):  c1 = 2 cp + 3 + 2 S + 2,
        |o - o64| <= 2^-8 |o64| + (2^-8 + c1 u) sum_j P64 |V|,   and the same for dV with |dO|.
    The backward takes lse as given (P64 = exp(s64 - lse)); delta_i = sum_j P_ij dP_ij is computed
    from P and dP, so its error is relative to D_i = sum_j P64 |dP64| (>= |delta64|), which takes
    |delta64|'s place in the form.  dP is a 32-term chain on G = sum_d |dO| |V|, entering dS
    directly and through delta (2 * 33 Gm u on P64, Gm = max G); P's error enters dS twice (2 cp),
    delta is an S-term sum (S), the product, the dQ sum (S) and the scale (2):
        c2 = 2 cp + 2 S + 6,   mag = P64 (|dP64| + D),
        |dQ - dQ64| <= 2^-8 |dQ64| + 32^-1/2 sum_j ((2 2^-8 + c2 u) mag + 66 Gm u P64) |K|
    (dS is a bf16 operand: 2^-8, the second 2^-8 is the form's allowance), and the same for dK.
    dbias is an fp32 sum of the unrounded dS over the entries that share an index, a chain of at
    most nWt + S terms (walk, fold, slab rows): only c u terms,
        |dbias - dbias64| <= sum ((c2 + nWt + S) u mag + 66 Gm u P64 + 2^-126 (1 + |dP64| + D)).
    The last term is fp32 underflow, which the relative model leaves out: an index whose entries
    are all masked sums P of about e^-100, below the smallest normal number 2^-126, where a P or
    a product may be flushed to zero."""
    B, H, Hf, Wf, ws, shift = case
    S = ws * ws
    qkv, do, bias = _inputs(case, dev)
    q, k, v, add, mask, idx = _scores(qkv, bias, case)
    kt = k.transpose(-1, -2)
    cp = 38 * float((q.abs() @ kt.abs() * SCALE + add.abs() + mask.abs()).max()) + 4
    c1 = 2 * cp + 3 + 2 * S + 2
    s = q @ kt * SCALE + add + mask
    p = torch.softmax(s, -1)
    o64 = p @ v
    o, lse = k_.wattn_fwd(qkv, bias, H, Hf, Wf, ws, shift)
    assert o.shape == (B * Hf * Wf, H * 32) and lse.shape == (s.shape[0], H, S)
    assert bool(((_textbook(o, case, 32) - o64).abs() <= R * o64.abs() + (R + c1 * U) * (p @ v.abs())).all())
    assert torch.allclose(ag._d(lse), torch.logsumexp(s, -1), rtol=0, atol=(c1 + 2) * U * (1 + float(s.abs().max())))
    # backward, lse as given
    d64 = _textbook(do, case, 32)
    p = torch.exp(s - ag._d(lse)[..., None])
    dp = d64 @ v.transpose(-1, -2)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    mag = p * (dp.abs() + (p * dp.abs()).sum(-1, keepdim=True))
    gm = float((d64.abs() @ v.abs().transpose(-1, -2)).max())
    c2 = 2 * cp + 2 * S + 6
    dbias = torch.full_like(bias, float("nan"))
    dqkv = k_.wattn_bwd(do, qkv, lse, bias, dbias, H, Hf, Wf, ws, shift, True)
    dq, dk, dv = (_textbook(dqkv[:, i * H * 32:(i + 1) * H * 32], case, 32) for i in range(3))
    dv64 = p.transpose(-1, -2) @ d64
    assert bool(((dv - dv64).abs() <= R * dv64.abs() + (R + c1 * U) * (p.transpose(-1, -2) @ d64.abs())).all())
    err = (2 * R + c2 * U) * mag + 66 * gm * U * p
    dq64, dk64 = ds @ k * SCALE, ds.transpose(-1, -2) @ q * SCALE
    assert bool(((dq - dq64).abs() <= R * dq64.abs() + (err @ k.abs()) * SCALE).all())
    assert bool(((dk - dk64).abs() <= R * dk64.abs() + (err.transpose(-1, -2) @ q.abs()) * SCALE).all())
    nb = (2 * ws - 1) ** 2
    fold = lambda t: torch.zeros(H, nb, dtype=torch.float64).index_add_(1, idx.reshape(-1), t.sum(0).reshape(H, S * S))
    dsum = (p * dp.abs()).sum(-1, keepdim=True)
    berr = fold((c2 + s.shape[0] + S) * U * mag + 66 * gm * U * p + 2.0 ** -126 * (1 + dp.abs() + dsum))
    assert bool(((ag._d(dbias).reshape(H, nb) - fold(ds)).abs() <= berr).all())
    # accumulate into the sink, and two runs are bitwise equal
    acc = torch.ones_like(bias)
    dqkv2 = k_.wattn_bwd(do, qkv, lse, bias, acc, H, Hf, Wf, ws, shift, False)
    assert torch.equal(dqkv2, dqkv) and torch.equal(acc, 1 + dbias)
    assert all(torch.equal(a, b) for a, b in zip(k_.wattn_fwd(qkv, bias, H, Hf, Wf, ws, shift), (o, lse)))


def check_window_isolation(k_, dev, case):
    """New q, k, v for one window's tokens leave o of every other window bitwise unchanged.  In a
    shifted case, new values for the tokens of one region of a window leave o of that window's
    other tokens unchanged to the bf16 bit: a masked P is at most e^(-100 + spread), spread the
    range of the unmasked scores; with spread < 12 it is below 2^-126, the smallest normal
    fp32 and bf16 number, which neither the row sum (>= 1) nor an fp32 accumulator sees."""
    B, H, Hf, Wf, ws, shift = case
    qkv, _, bias = _inputs(case, dev, gain=0.5)
    rows = ref.window_partition(torch.arange(B * Hf * Wf)[:, None], Hf, Wf, ws, shift)[..., 0]
    w0 = rows.shape[0] - 1  # the last window: all nine regions when shifted
    region = ref.swin_shift_mask(Hf, Wf, ws, shift)[w0 % (rows.shape[0] // B), 0] == 0  # token 0's
    o = k_.wattn_fwd(qkv, bias, H, Hf, Wf, ws, shift)[0]
    for changed in ([rows[w0]] if shift == 0 else [rows[w0], rows[w0][region]]):
        new = qkv.clone()
        gen = torch.Generator().manual_seed(5)
        new[changed.to(dev)] = (torch.randn(len(changed), 3 * H * 32, generator=gen) * 0.5).to(BF).to(dev)
        for t in (qkv, new):
            q, k, _, add, _, _ = _scores(t, bias, case)
            s = (q @ k.transpose(-1, -2) * SCALE + add)[w0]
            assert -100 + float(s.max() - s.min()) < math.log(2.0 ** -126)
        keep = torch.ones(B * Hf * Wf, dtype=torch.bool)
        keep[changed] = False
        o2 = k_.wattn_fwd(new, bias, H, Hf, Wf, ws, shift)[0]
        assert torch.equal(o2.cpu()[keep], o.cpu()[keep]) and not torch.equal(o2.cpu()[~keep], o.cpu()[~keep])


def check_uniform(k_, dev, case):
    """All keys of a head equal, no shift, zero bias, ws^2 a power of two, small integers: every
    score of a row is the same number, so P is 1 / ws^2 (exactly, once rounded to bf16 in the
    backward): o is the exact window mean of v and dv the exact window mean of do."""
    B, H, Hf, Wf, ws, shift = case
    gen = torch.Generator().manual_seed(ws)
    n = B * Hf * Wf
    q, v = ag._ints((n, H * 32), -2, 2, gen), ag._ints((n, H * 32), -3, 3, gen)
    key = ag._ints((1, H * 32), -2, 2, gen).expand(n, H * 32)
    qkv = torch.cat([q, key, v], 1).to(BF).to(dev)
    do = ag._ints((n, H * 32), -3, 3, gen).to(BF).to(dev)
    bias = torch.zeros(H * (2 * ws - 1) ** 2, device=dev)
    o, lse = k_.wattn_fwd(qkv, bias, H, Hf, Wf, ws, shift)
    mean = lambda t: _textbook(t, case, 32).mean(2, keepdim=True).expand(-1, -1, ws * ws, -1)
    assert torch.equal(_textbook(o, case, 32), mean(v))
    dqkv = k_.wattn_bwd(do, qkv, lse, bias, torch.empty_like(bias), H, Hf, Wf, ws, shift, True)
    assert torch.equal(_textbook(dqkv[:, 2 * H * 32:], case, 32), mean(do))


def check_wattn_refusals(k_, dev):
    z = lambda *shape, dt=BF: torch.zeros(*shape, dtype=dt, device=dev)
    bad = [(z(81, 96), 1, 9, 9, 9, 0),                             # ws^2 > 64
           (z(210, 96), 1, 15, 14, 7, 0), (z(210, 96), 1, 14, 15, 7, 0),  # map no multiple of ws
           (z(49, 96), 1, 7, 7, 7, 7), (z(49, 96), 1, 7, 7, 7, -1),       # shift outside [0, ws)
           (z(49, 192), 1, 7, 7, 7, 0),                            # head dim 64
           (z(49, 96, dt=torch.float64), 1, 7, 7, 7, 0),           # dtype
           (z(96, 49).t(), 1, 7, 7, 7, 0)]                         # not contiguous
    for qkv, H, Hf, Wf, ws, shift in bad:
        with pytest.raises((RuntimeError, ValueError)):
            k_.wattn_fwd(qkv, z(H * (2 * ws - 1) ** 2, dt=torch.float32), H, Hf, Wf, ws, shift)
    with pytest.raises((RuntimeError, ValueError)):  # bias dtype
        k_.wattn_fwd(z(49, 96), z(169), 1, 7, 7, 7, 0)


def check_unpatchify(k_, dev, B, Hi, Wi, C, P):
    gen = torch.Generator().manual_seed(Hi + Wi)
    x = torch.randn(B, Hi, Wi, C, generator=gen).to(BF).to(dev)
    back = k_.unpatchify(k_.patchify(x, P), Hi, Wi, P)
    assert back.shape == x.shape and torch.equal(back, x)


pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CASES)
def test_window_attention_against_float64(gpu, case):
    check_against_float64(ag.C(), gpu, case)


@pytest.mark.parametrize("case", [c for c in CASES if c[0] * c[2] * c[3] > c[4] ** 2 or c[5]])
def test_window_attention_isolation(gpu, case):
    check_window_isolation(ag.C(), gpu, case)


@pytest.mark.parametrize("case", UNIFORM_CASES)
def test_window_attention_uniform_exact(gpu, case):
    check_uniform(ag.C(), gpu, case)


def test_window_attention_refusals(gpu):
    check_wattn_refusals(ag.C(), gpu)


@pytest.mark.parametrize("case", UNPATCH_CASES)
def test_unpatchify_bitwise(gpu, case):
    check_unpatchify(ag.C(), gpu, *case)


def test_swin_block_pair_parity_with_cpu_fp32(gpu):
    from mpi_pytorch_amd.models.swin import SwinBlock
    from mpi_pytorch_amd.parallel.arena import ParamArena
    torch.manual_seed(3)
    mk = lambda: torch.nn.Sequential(SwinBlock(64, 2, 7, 0), SwinBlock(64, 2, 7, 3))
    bc, bg = mk(), mk()
    for p in bc.parameters():  # away from the zero biases and unit scales of the initialisation
        if p.dim() == 1:
            torch.nn.init.normal_(p, 0.5, 0.5)
    bg.load_state_dict(bc.state_dict())
    bg = bg.to(gpu)
    x = torch.randn(2 * 14 * 14, 64).to(BF)
    res = []
    for blk, dev in ((bc, torch.device("cpu")), (bg, gpu)):
        ParamArena(blk, dev)
        xi = (x.float() if dev.type == "cpu" else x.to(dev)).requires_grad_()
        y = blk[1](blk[0](xi * 1, 14, 14), 14, 14)
        torch.manual_seed(4)
        y.backward(torch.randn(y.shape).to(BF).to(dev).to(y.dtype))
        res.append([y.detach(), xi.grad] + [q.grad for q in blk.parameters()])
    names = ["y", "dx"] + [n for n, _ in bc.named_parameters()]
    cos = {n: round(dg._cos(a, b), 4) for n, a, b in zip(names, *res)}
    assert min(cos.values()) >= 0.99, cos


def test_swin_training_step_bitwise(gpu, monkeypatch):
    from mpi_pytorch_amd.engine import build_training
    from mpi_pytorch_amd.models.swin import SwinTransformer
    from mpi_pytorch_amd import models
    from mpi_pytorch_amd.parallel import World
    monkeypatch.setitem(models.WINDOW_ARCH, "swin",
                        ("swin_reduced", lambda n: SwinTransformer(4, 64, (1, 1), (2, 4), 4, n), 32))
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(8, 32, 32, 8, generator=g) * (torch.arange(8) < 3)).to(gpu, BF)
    y = torch.randint(0, 10, (8,), generator=g).to(gpu)
    outs = []
    for _ in range(2):
        torch.manual_seed(0)
        model, _opt, step, _ = build_training("swin", 10, gpu, World(device=gpu), 1e-3)
        loss = step(x, y).clone()
        torch.cuda.synchronize()
        outs.append((loss.cpu(), model._mpa_arena.grad.cpu().clone(),
                     model._mpa_arena.master.cpu().clone()))
    assert bool(torch.isfinite(outs[0][0]).all()) and float(outs[0][1].abs().sum()) > 0
    assert all(torch.equal(a, b) for a, b in zip(*outs))
