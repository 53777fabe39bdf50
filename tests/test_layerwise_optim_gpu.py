"""Layer-wise optimizers on the device (csrc/kernels/optim.hip): the per-chunk norms over the
segment plan, the trust ratios, the LAMB / AdamW / LARS update kernels against the
``ops/ref.py`` twins and float64 per-parameter loops written here, and the optimizers under
non-finite skip, HIP-graph replay, two ranks and checkpoint resume.

The reference has none of this (``main.py:125`` there: ``torch.optim.Adam``); the oracles
are ``torch.optim.AdamW``, the existing ``adam_step_dev`` kernel and the papers' formulas in
float64."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from mpi_pytorch_amd.engine import build_training
from mpi_pytorch_amd.ops import ref
from mpi_pytorch_amd.parallel import World
from mpi_pytorch_amd.parallel.arena import ALIGN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the kernels take betas and eps as fp32: the float64 loops below get the same values (at
# t = 7 the fp32 rounding of 0.999 alone moves 1 - b2^8 by 1.3e-5)
B1, B2, EPS = (float(np.float32(x)) for x in (0.9, 0.999, 1e-8))
BOTH = ref.SEG_DECAY | ref.SEG_ADAPT
ZERO = 4  # the all-zero segment of the plan below, between two non-zero ones


def C():
    from mpi_pytorch_amd.ops import _ext
    return _ext.ext()


@pytest.fixture
def det(gpu):
    k = C()
    old = k.deterministic()
    k.set_deterministic(1)
    yield gpu
    k.set_deterministic(int(old))


def rel64(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


# -------------------------------------------------------------------------------- plan
class Plan:
    """Six segments that mix the flags: one slot; 17 slots; exactly one chunk; one chunk +
    one slot (a full and a one-slot chunk); one slot (all zero in the tests); two chunks
    less one slot.  The grids are not capped (one block per chunk), so no segment wraps."""

    def __init__(self, dev, flags=(BOTH, 0, BOTH, ref.SEG_DECAY, ref.SEG_ADAPT, BOTH)):
        CH = int(C().seg_chunk())
        assert CH == ref.seg_chunk() and CH % ALIGN == 0
        self.CH = CH
        self.lens = [ALIGN, ALIGN * 17, CH, CH + ALIGN, ALIGN, 2 * CH - ALIGN]
        self.flags = list(flags)
        rows, chunk_seg, off = [], [], 0
        for s, (ln, f) in enumerate(zip(self.lens, self.flags)):
            nch = -(-ln // CH)
            rows.append([off, ln, len(chunk_seg), nch, f])
            chunk_seg += [s] * nch
            off += ln
        assert [r[3] for r in rows] == [1, 1, 1, 2, 1, 2]
        self.rows, self.n, self.nseg, self.nchunks = rows, off, len(rows), len(chunk_seg)
        self.seg_cpu = torch.tensor(rows, dtype=torch.int64)
        self.chunk_cpu = torch.tensor(chunk_seg, dtype=torch.int32)
        self.seg, self.chunk_seg = self.seg_cpu.to(dev), self.chunk_cpu.to(dev)
        self.dev = dev

    def slices(self):
        return [slice(r[0], r[0] + r[1]) for r in self.rows]

    def on(self, s, bit):
        return bool(self.flags[s] & bit)

    def bufs(self, dev=None):
        dev = self.dev if dev is None else dev
        return (torch.zeros(2, self.nchunks, device=dev), torch.ones(self.nseg, device=dev),
                torch.zeros(self.nseg, 2, device=dev))

    def seg_sums(self, part):
        return [float(part[r[2]:r[2] + r[3]].double().sum()) for r in self.rows]


def _hyper(dev, lr=1e-2 / 3, gs=1.0, skip=0.0):
    h = torch.zeros(ref.HYPER_N, device=dev)
    h[ref.HYPER_LR], h[ref.HYPER_SCALE], h[ref.HYPER_SKIP] = lr, gs, skip
    return h


def _ints(plan, gen):
    """Small integers, sparse enough that every chunk's sum stays below 2^24 (exact in
    fp32); the last element of every non-zero segment is set (it is read)."""
    x = torch.randint(-3, 4, (plan.n,), device=plan.dev, generator=gen).float()
    x *= (torch.rand(plan.n, device=plan.dev, generator=gen) < 1 / 4)
    for s, sl in enumerate(plan.slices()):
        x[sl.stop - 1] = 0.0 if s == ZERO else 3.0
    x[plan.slices()[ZERO]] = 0.0
    return x


def _randn(plan, gen, scale=1.0):
    x = torch.randn(plan.n, device=plan.dev, generator=gen) * scale
    x[plan.slices()[ZERO]] = 0.0
    return x


# ------------------------------------------------------------------------ 1. exact norms
def test_norms_exact_and_reproducible(gpu):
    plan = Plan(gpu)
    k = C()
    gen = torch.Generator(device=gpu).manual_seed(11)
    h = _hyper(gpu)
    part, ratio, norms = plan.bufs()
    p, g = _ints(plan, gen), _ints(plan, gen)
    # seg_sqnorm, and lamb_norms' sum of p^2: integers, exact
    k.seg_sqnorm(p, plan.seg, plan.chunk_seg, h, False, part[0])
    k.seg_sqnorm(g, plan.seg, plan.chunk_seg, h, True, part[1])  # (scale 1.0)
    k.trust_ratio(plan.seg, plan.chunk_seg, part[0], part[1], h, ref.TRUST_LAMB, 0.0, 0.0, ratio,
                  norms)
    z = torch.zeros(plan.n, device=gpu)
    part2 = torch.zeros_like(part)
    k.lamb_norms(p, z, z, z, torch.zeros(1, device=gpu), h, plan.seg, plan.chunk_seg, part2[0],
                 part2[1], B1, B2, EPS, 0.0)
    for x, pt, col in ((p, part[0], 0), (g, part[1], 1), (p, part2[0], None)):
        assert float(pt.max()) < 2 ** 24
        got = plan.seg_sums(pt)
        for s, sl in enumerate(plan.slices()):
            exact = float((x[sl].double() ** 2).sum())
            assert got[s] == exact, (s, got[s], exact)
            assert (exact == 0.0) == (s == ZERO)
            if col is not None:  # sqrtf is correctly rounded: the norm of an exact sum
                assert float(norms[s, col]) == float(np.sqrt(np.float32(exact)))
    assert float(part2[1].abs().max()) == 0.0  # g = m = v = 0, wd = 0: u is exactly 0
    assert float(ratio[ZERO]) == 1.0 and float(norms[ZERO].abs().max()) == 0.0
    # random values: within the project's norm bound of float64, bitwise equal twice, in
    # every mode (fixed order, no atomics)
    p, g = _randn(plan, gen), _randn(plan, gen, 0.1)
    m, v = _randn(plan, gen, 0.1), _randn(plan, gen, 0.1).abs()
    st = torch.full((1,), 7.0, device=gpu)
    h = _hyper(gpu, gs=0.5)
    old = k.deterministic()
    runs = []
    try:
        for mode in (0, 0, 1):
            k.set_deterministic(mode)
            a, b = torch.zeros_like(part), torch.zeros_like(part)
            k.seg_sqnorm(p, plan.seg, plan.chunk_seg, h, False, a[0])
            k.seg_sqnorm(g, plan.seg, plan.chunk_seg, h, True, a[1])
            k.lamb_norms(p, g, m, v, st, h, plan.seg, plan.chunk_seg, b[0], b[1], B1, B2, EPS,
                         0.01)
            r, nv = torch.ones_like(ratio), torch.zeros_like(norms)
            k.trust_ratio(plan.seg, plan.chunk_seg, b[0], b[1], h, ref.TRUST_LAMB, 0.0, 0.01, r,
                          nv)
            runs.append((a, b, r, nv))
    finally:
        k.set_deterministic(int(old))
    for other in runs[1:]:
        for t, u in zip(runs[0], other):
            assert torch.equal(t, u)
    a, b, _r, nv = runs[0]
    u64 = _lamb64(plan, p, g, m, v, 7, 0.5, 0.01)[0]
    p2, g2 = p.double().cpu() ** 2, (g.double().cpu() * 0.5) ** 2
    for pt, sq in ((a[0], p2), (a[1], g2), (b[0], p2), (b[1], u64 ** 2)):
        got = plan.seg_sums(pt)
        for s, sl in enumerate(plan.slices()):
            want = float(sq[sl].sum())
            assert abs(got[s] - want) <= 1e-5 * want, (s, got[s], want)
    for s, sl in enumerate(plan.slices()):
        want = float(p[sl].double().norm())
        assert abs(float(nv[s, 0]) - want) <= 5e-6 * want


# ---------------------------------------------------------------- float64 textbook loops
def _lamb64(plan, p, g, m, v, t, gs, wd, lr=0.0):
    """(u, ratios, dp) of LAMB with bias correction, per parameter in float64; t = 0-based."""
    p, g, m, v = (x.double().cpu() for x in (p, g, m, v))
    u, dp, ratios = torch.zeros_like(p), torch.zeros_like(p), []
    for s, sl in enumerate(plan.slices()):
        gh = g[sl] * gs
        m2 = B1 * m[sl] + (1 - B1) * gh
        v2 = B2 * v[sl] + (1 - B2) * gh * gh
        us = (m2 / (1 - B1 ** (t + 1))) / ((v2 / (1 - B2 ** (t + 1))).sqrt() + EPS)
        if plan.on(s, ref.SEG_DECAY):
            us = us + wd * p[sl]
        pn, un = float(p[sl].norm()), float(us.norm())
        r = pn / un if plan.on(s, ref.SEG_ADAPT) and pn > 0 and un > 0 else 1.0
        u[sl], dp[sl] = us, -lr * r * us
        ratios.append(r)
    return u, ratios, dp


def _adamw64(plan, p, g, m, v, t, gs, wd, lr):
    p, g, m, v = (x.double().cpu() for x in (p, g, m, v))
    dp = torch.zeros_like(p)
    for s, sl in enumerate(plan.slices()):
        gh = g[sl] * gs
        m2 = B1 * m[sl] + (1 - B1) * gh
        v2 = B2 * v[sl] + (1 - B2) * gh * gh
        adam = (m2 / (1 - B1 ** (t + 1))) / ((v2 / (1 - B2 ** (t + 1))).sqrt() + EPS)
        wd_s = wd if plan.on(s, ref.SEG_DECAY) else 0.0
        dp[sl] = -lr * wd_s * p[sl] - lr * adam
    return dp


def _lars64(plan, p, g, buf, t, gs, wd, lr, coef, mom=0.9):
    p, g, buf = (x.double().cpu() for x in (p, g, buf))
    dp, ratios = torch.zeros_like(p), []
    for s, sl in enumerate(plan.slices()):
        gh = g[sl] * gs
        wd_s = wd if plan.on(s, ref.SEG_DECAY) else 0.0
        pn, gn = float(p[sl].norm()), float(gh.norm())
        r = 1.0
        if plan.on(s, ref.SEG_ADAPT) and pn > 0 and gn > 0:
            r = coef * pn / (gn + wd_s * pn + 1e-8)
        g2 = r * (gh + wd_s * p[sl])
        b2 = g2 if t == 0 else mom * buf[sl] + g2
        dp[sl] = -lr * b2
        ratios.append(r)
    return ratios, dp


# --------------------------------------------------------------------------- 2. ratios
def test_lamb_ratios(gpu):
    plan = Plan(gpu)
    k = C()
    gen = torch.Generator(device=gpu).manual_seed(21)
    p, g = _randn(plan, gen), _randn(plan, gen, 0.1)
    m, v = _randn(plan, gen, 0.1), _randn(plan, gen, 0.1).abs()
    st = torch.full((1,), 7.0, device=gpu)
    h = _hyper(gpu, gs=0.5)
    part, ratio, norms = plan.bufs()
    k.lamb_norms(p, g, m, v, st, h, plan.seg, plan.chunk_seg, part[0], part[1], B1, B2, EPS, 0.01)
    k.trust_ratio(plan.seg, plan.chunk_seg, part[0], part[1], h, ref.TRUST_LAMB, 0.0, 0.01,
                  ratio, norms)
    want = _lamb64(plan, p, g, m, v, 7, 0.5, 0.01)[1]
    got = ratio.tolist()
    for s in range(plan.nseg):
        if not plan.on(s, ref.SEG_ADAPT) or s == ZERO:
            assert got[s] == 1.0 and want[s] == 1.0
        else:  # two norms, each good to 5e-6
            assert got[s] != 1.0 and abs(got[s] - want[s]) <= 1e-5 * want[s], (s, got[s], want[s])
    # the oracle computes the same from the same inputs
    cp, cr, cn = plan.bufs("cpu")
    hc = h.cpu()
    ref.lamb_norms(p.cpu(), g.cpu(), m.cpu(), v.cpu(), st.cpu(), hc, plan.seg_cpu, plan.chunk_cpu,
                   cp[0], cp[1], B1, B2, EPS, 0.01)
    ref.trust_ratio(plan.seg_cpu, plan.chunk_cpu, cp[0], cp[1], hc, ref.TRUST_LAMB, 0.0, 0.01, cr,
                    cn)
    assert rel64(ratio, cr) <= 1e-5 and rel64(norms, cn) <= 5e-6


@pytest.mark.parametrize("gs", [1.0, 0.5])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_lars_ratios(gpu, gs, wd):
    plan = Plan(gpu)
    k = C()
    gen = torch.Generator(device=gpu).manual_seed(22)
    p, g = _randn(plan, gen), _randn(plan, gen, 0.1)
    h = _hyper(gpu, gs=gs)
    part, ratio, norms = plan.bufs()
    k.seg_sqnorm(p, plan.seg, plan.chunk_seg, h, False, part[0])
    k.seg_sqnorm(g, plan.seg, plan.chunk_seg, h, True, part[1])
    k.trust_ratio(plan.seg, plan.chunk_seg, part[0], part[1], h, ref.TRUST_LARS, 0.02, wd, ratio,
                  norms)
    want = _lars64(plan, p, g, torch.zeros_like(p), 0, gs, wd, 0.0, 0.02)[0]
    got = ratio.tolist()
    for s in range(plan.nseg):
        if not plan.on(s, ref.SEG_ADAPT) or s == ZERO:
            assert got[s] == 1.0 and want[s] == 1.0
        else:
            assert abs(got[s] - want[s]) <= 1e-5 * want[s], (s, got[s], want[s])
    gn = float((g[plan.slices()[0]].double() * gs).norm())
    assert abs(float(norms[0, 1]) - gn) <= 5e-6 * gn  # the norm of the SCALED gradient
    cp, cr, cn = plan.bufs("cpu")
    hc = h.cpu()
    ref.seg_sqnorm(p.cpu(), plan.seg_cpu, plan.chunk_cpu, hc, False, cp[0])
    ref.seg_sqnorm(g.cpu(), plan.seg_cpu, plan.chunk_cpu, hc, True, cp[1])
    ref.trust_ratio(plan.seg_cpu, plan.chunk_cpu, cp[0], cp[1], hc, ref.TRUST_LARS, 0.02, wd, cr,
                    cn)
    assert rel64(ratio, cr) <= 1e-5 and rel64(norms, cn) <= 5e-6


# ------------------------------------------------------- 3. updates against the oracle
def _state(plan, seed):
    gen = torch.Generator(device=plan.dev).manual_seed(seed)
    p, g = _randn(plan, gen), _randn(plan, gen, 0.1)
    m, v = _randn(plan, gen, 0.1), _randn(plan, gen, 0.1).abs()  # (v is never negative)
    return p, g, m, v


def _gpu_update(kind, plan, p, g, m, v, sh, st, h, wd, coef=0.02):
    k = C()
    part, ratio, norms = plan.bufs()
    if kind == "lamb":
        k.lamb_norms(p, g, m, v, st, h, plan.seg, plan.chunk_seg, part[0], part[1], B1, B2, EPS, wd)
        k.trust_ratio(plan.seg, plan.chunk_seg, part[0], part[1], h, ref.TRUST_LAMB, 0.0, wd,
                      ratio, norms)
    if kind in ("lamb", "adamw"):
        k.lamb_step_dev(p, g, m, v, sh, st, h, plan.seg, plan.chunk_seg, ratio, B1, B2, EPS, wd,
                        kind == "adamw")
    else:
        k.seg_sqnorm(p, plan.seg, plan.chunk_seg, h, False, part[0])
        k.seg_sqnorm(g, plan.seg, plan.chunk_seg, h, True, part[1])
        k.trust_ratio(plan.seg, plan.chunk_seg, part[0], part[1], h, ref.TRUST_LARS, coef, wd,
                      ratio, norms)
        k.lars_step_dev(p, g, m, sh, st, h, plan.seg, plan.chunk_seg, ratio, 0.9, 0.0, wd, False)
    return ratio


def _ref_update(kind, plan, p, g, m, v, sh, st, h, wd, coef=0.02):
    part, ratio, norms = plan.bufs("cpu")
    sg, cs = plan.seg_cpu, plan.chunk_cpu
    if kind == "lamb":
        ref.lamb_norms(p, g, m, v, st, h, sg, cs, part[0], part[1], B1, B2, EPS, wd)
        ref.trust_ratio(sg, cs, part[0], part[1], h, ref.TRUST_LAMB, 0.0, wd, ratio, norms)
    if kind in ("lamb", "adamw"):
        ref.lamb_step_dev(p, g, m, v, sh, st, h, sg, cs, ratio, B1, B2, EPS, wd, kind == "adamw")
    else:
        ref.seg_sqnorm(p, sg, cs, h, False, part[0])
        ref.seg_sqnorm(g, sg, cs, h, True, part[1])
        ref.trust_ratio(sg, cs, part[0], part[1], h, ref.TRUST_LARS, coef, wd, ratio, norms)
        ref.lars_step_dev(p, g, m, sh, st, h, sg, cs, ratio, 0.9, 0.0, wd, False)


@pytest.mark.parametrize("kind", ["lamb", "adamw", "lars"])
@pytest.mark.parametrize("shadow", [True, False])
def test_updates_match_oracle(gpu, kind, shadow):
    """Step indices 0 and 7 from non-zero state.  p and the bf16 shadow against the fp32
    twin (the bounds test_kernels_gpu.py uses for Adam / SGD); the update dp against the
    float64 textbook loops above, allowed 4x the error the fp32 twin itself shows against
    that loop on the same inputs (FMA contraction, another summation order).  That error is
    mostly the rounding of p + dp to fp32, relative to the largest |dp|: measured with these
    inputs at lr = 1e-2/3 for steps 0 / 7, 9.8e-7 / 5.8e-7 (lamb), 3.8e-6 / 5.2e-6 (adamw)
    and 4.3e-4 / 1.8e-4 (lars, whose trust_coef = 0.02 makes dp that much smaller); the
    kernels showed the same figures (adamw: 3.7e-6 / 3.1e-6)."""
    plan = Plan(gpu)
    wd, gs = 0.01, 1.0 / 3
    h = _hyper(gpu, gs=gs)
    lr, gs = float(h[ref.HYPER_LR]), float(h[ref.HYPER_SCALE])  # the fp32 values
    none = torch.empty(0, device=gpu)
    for t in (0, 7):
        p, g, m, v = _state(plan, 30 + t)
        sh = torch.zeros(plan.n, dtype=torch.bfloat16, device=gpu) if shadow else none
        st = torch.full((1,), float(t), device=gpu)
        cpu = [x.cpu().clone() for x in (p, g, m, v, sh, st, h)]
        p0, m0, v0 = p.clone(), m.clone(), v.clone()
        if kind == "lars":
            dp64 = _lars64(plan, p, g, m, t, gs, wd, lr, 0.02)[1]
        elif kind == "lamb":
            dp64 = _lamb64(plan, p, g, m, v, t, gs, wd, lr)[2]
        else:
            dp64 = _adamw64(plan, p, g, m, v, t, gs, wd, lr)
        _gpu_update(kind, plan, p, g, m, v, sh, st, h, wd)
        _ref_update(kind, plan, *cpu, wd)
        rp, _rg, rm, rv, rsh = cpu[:5]
        assert not torch.equal(p, p0)
        assert rel64(p, rp) < 1e-5
        assert rel64(m, rm) < 1e-5 and (kind == "lars" or rel64(v, rv) < 1e-5)
        if shadow:
            assert rel64(sh.float(), rp) < 1e-2
            assert torch.equal(sh, p.to(torch.bfloat16))
        ref_err = rel64(rp.double() - p0.double().cpu(), dp64)
        got_err = rel64(p.double() - p0.double(), dp64)
        print("%s t=%d: dp vs float64: fp32 twin %.3e, kernel %.3e" % (kind, t, ref_err, got_err))
        assert ref_err > 0 and got_err <= 4 * ref_err, (got_err, ref_err)
        z = plan.slices()[ZERO]  # p = g = m = v = 0 stays exactly 0
        assert not p[z].any() and not m[z].any() and (kind == "lars" or not v[z].any())
        if kind != "lars":  # moments: bitwise adam_step_dev's with wd = 0
            pa, ma, va = p0.clone(), m0.clone(), v0.clone()
            C().adam_step_dev(pa, g, ma, va, none, st, h, B1, B2, EPS, 0.0)
            assert torch.equal(m, ma) and torch.equal(v, va)


@pytest.mark.parametrize("t", [0, 7])
def test_adamw_matches_torch(gpu, t):
    """Every decay flag on: one torch.optim.AdamW step on the same tensors on the CPU."""
    plan = Plan(gpu, flags=(BOTH,) * 6)
    wd = 0.01
    h = _hyper(gpu, gs=1.0 / 3)
    lr, gs = float(h[ref.HYPER_LR]), float(h[ref.HYPER_SCALE])
    p, g, m, v = _state(plan, 40 + t)
    tp = torch.nn.Parameter(p.cpu().clone())
    tp.grad = g.cpu() * gs
    opt = torch.optim.AdamW([tp], lr=lr, betas=(B1, B2), eps=EPS, weight_decay=wd)
    opt.state[tp] = dict(step=torch.tensor(float(t)), exp_avg=m.cpu().clone(),
                         exp_avg_sq=v.cpu().clone())
    opt.step()
    st = torch.full((1,), float(t), device=gpu)
    _gpu_update("adamw", plan, p, g, m, v, torch.empty(0, device=gpu), st, h, wd)
    assert rel64(p, tp.detach()) < 1e-5
    assert rel64(m, opt.state[tp]["exp_avg"]) < 1e-5
    assert rel64(v, opt.state[tp]["exp_avg_sq"]) < 1e-5


# ----------------------------------------------------------------------- 4. neighbours
@pytest.mark.parametrize("kind", ["lamb", "adamw", "lars"])
def test_no_decay_segments_are_left_alone(gpu, kind):
    """g = 0 and zero state: a segment without the decay flag stays bitwise unchanged while
    its decaying neighbours move."""
    plan = Plan(gpu)
    gen = torch.Generator(device=gpu).manual_seed(50)
    p = torch.randn(plan.n, device=gpu, generator=gen)
    z = torch.zeros(plan.n, device=gpu)
    g, m, v = z.clone(), z.clone(), z.clone()
    sh = p.to(torch.bfloat16)
    p0, sh0 = p.clone(), sh.clone()
    st = torch.zeros(1, device=gpu)
    _gpu_update(kind, plan, p, g, m, v, sh, st, _hyper(gpu, lr=0.1), 0.1, coef=1.0)
    for s, sl in enumerate(plan.slices()):
        if plan.on(s, ref.SEG_DECAY):
            assert not torch.equal(p[sl], p0[sl]), s
            assert bool((p[sl].abs() <= p0[sl].abs()).all())  # decay shrinks
        else:
            assert torch.equal(p[sl], p0[sl]) and torch.equal(sh[sl], sh0[sl]), s


def _structural_zeros(arena):
    """True where the arena holds a stored element that no exported tensor has: alignment
    padding, the pixel-pair stem's 4th channel and column past the kernel, pad_out rows."""
    zero = torch.ones(arena.n_train, dtype=torch.bool)
    for p in arena.trainable:
        o, e = arena.slice_of(p)
        keep = torch.ones(p.shape)
        if getattr(p, "_mpa_export", None) is not None:
            keep = p._mpa_import(p._mpa_export(keep))
        zero[o:e] = keep.reshape(-1) == 0
    return zero


def test_stored_zeros_stay_zero_under_lamb(det):
    """ResNet-18 with 10 classes has all three kinds: a 7x7 stride-2 pixel-pair stem
    (Conv2d), a head stored with 32 rows (pad_out), and a bias slot with padding."""
    gpu = det
    torch.manual_seed(0)
    model, opt, step, _ = build_training("resnet18", 10, gpu, World(device=gpu), 1e-2, "lamb",
                                         weight_decay=0.05)
    a = model._mpa_arena
    zero = _structural_zeros(a)
    names = {a.names[id(p)]: int(zero[slice(*a.slice_of(p))].sum()) for p in a.trainable}
    assert names["conv1.weight"] > 0 and names["fc.weight"] == 22 * 512
    fcb = dict(model.named_parameters())["fc.bias"]
    o, e = a.slice_of(fcb)
    assert names["fc.bias"] == 22 and e - o == 32 and zero[e:o + ALIGN].all()  # + padding
    x, y = _batch(gpu, B=8, nc=10)
    for _ in range(3):
        step(x, y)
    torch.cuda.synchronize()
    n = a.n_train
    for t in (a.master[:n], a.shadow[:n], a.grad[:n], opt.exp_avg[:n], opt.exp_avg_sq[:n]):
        assert not t.cpu()[zero].any()
    assert float(opt.step_t) == 3.0
    r = opt.last_trust_ratios()
    assert r["bn1.weight"] == 1.0 and r["fc.bias"] == 1.0 and r["conv1.weight"] != 1.0
    # the stored norm is the exported norm
    pn = opt.last_param_norms()["fc.weight"]
    assert pn[0] > 0 and pn[1] > 0


# ------------------------------------------------------------------------------ 5. skip
def _small(gpu, kind, **kw):
    from mpi_pytorch_amd.optim import FusedAdamW, FusedLAMB, FusedLARS
    from mpi_pytorch_amd.parallel.arena import ParamArena
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(40, 70), torch.nn.Linear(70, 9)).to(gpu)
    arena = ParamArena(model, gpu)
    params = list(model.parameters())
    if kind == "lars":
        opt = FusedLARS(params, arena, lr=1e-2, momentum=0.9, weight_decay=0.01, trust_coef=0.02,
                        **kw)
    else:
        cls = FusedAdamW if kind == "adamw" else FusedLAMB
        opt = cls(params, arena, lr=1e-2, weight_decay=0.01, **kw)
    state = [opt.momentum_buffer] if kind == "lars" else [opt.exp_avg, opt.exp_avg_sq]
    return model, arena, params, opt, state


@pytest.mark.parametrize("kind", ["adamw", "lamb", "lars"])
def test_nonfinite_step_is_skipped(gpu, kind):
    model, arena, params, opt, state = _small(gpu, kind)
    opt.set_clip(1.0)
    for t in state:
        t.normal_().abs_()
    opt.seg_ratio.fill_(0.25)  # (a skipped step leaves the ratios alone too)
    before = [t.clone() for t in [arena.master, arena.shadow, opt.seg_ratio, opt.seg_part] + state]
    arena.zero_grad()
    for p in params:
        p.grad.fill_(0.5)
    params[1].grad.view(-1)[5] = float("inf")
    opt.step()
    for t, c in zip([arena.master, arena.shadow, opt.seg_ratio, opt.seg_part] + state, before):
        assert torch.equal(t, c)
    assert opt.nonfinite_steps() == 1 and float(opt.step_t) == 1.0  # the step still counts
    assert math.isinf(opt.last_grad_norm())
    arena.zero_grad()
    for p in params:
        p.grad.fill_(0.5)
    opt.step()
    assert not torch.equal(arena.master, before[0]) and not torch.equal(state[0], before[4])
    assert torch.equal(arena.shadow[:arena.n_train],
                       arena.master[:arena.n_train].to(torch.bfloat16))
    assert opt.nonfinite_steps() == 1 and float(opt.step_t) == 2.0
    if kind != "adamw":
        assert not torch.equal(opt.seg_ratio, before[2])


# ---------------------------------------------------------------------- 6. graph replay
SCHED = dict(kind="cosine", warmup_steps=2, total_steps=6, lr_min_ratio=0.0)


def _train(gpu, kind, max_norm, seed=0):
    torch.manual_seed(seed)
    return build_training("resnet18", 100, gpu, World(device=gpu), 1e-3 if kind == "lamb" else 0.1,
                          kind, weight_decay=0.01, schedule=SCHED if max_norm else None,
                          clip_grad_norm=max_norm, trust_coef=0.02)[:3]


def _batch(gpu, B=32, hw=64, nc=100, seed=1):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = (torch.randn(B, hw, hw, 8, generator=g) * (torch.arange(8) < 3)).to(gpu, torch.bfloat16)
    y = torch.randint(0, nc, (B,), generator=g).to(gpu)
    return x, y


@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_graph_replays_bitwise_equal_eager(det, kind):
    """ResNet-18, warm-up 2 + cosine over 6 steps, clipping active: 4 graph replays == 4
    eager steps bitwise, and the replayed trust ratios move from step to step."""
    gpu = det
    x, y = _batch(gpu)
    model, opt, step = _train(gpu, kind, 0.0)
    step(x, y)
    n0 = float(model._mpa_arena.grad.double().norm())
    del model, opt, step
    max_norm = 0.5 * n0
    model, opt, step = _train(gpu, kind, max_norm)
    ref_loss = torch.stack([step(x, y).clone() for _ in range(4)])
    torch.cuda.synchronize()
    ref_master = model._mpa_arena.master.clone()
    ref_ratios = opt.last_trust_ratios()
    assert opt.nonfinite_steps() == 0
    del model, opt, step
    model, opt, step = _train(gpu, kind, max_norm)
    assert step.capture(x, y, warmup=2)
    assert float(opt.step_t) == 0.0 and set(opt.last_trust_ratios().values()) == {1.0}
    got, ratios = [], []
    for i in range(4):
        got.append(step(x, y).clone())
        ratios.append(opt.last_trust_ratios())
        if i == 0:
            assert float(opt.hyper[ref.HYPER_COEF]) < 1.0  # clipping was active
    torch.cuda.synchronize()
    assert ratios[0] != ratios[1] and ratios[1] != ratios[3]
    assert ratios[3] == ref_ratios
    assert ratios[0]["bn1.weight"] == 1.0 and ratios[0]["conv1.weight"] != 1.0
    assert torch.equal(torch.stack(got), ref_loss)
    assert torch.equal(model._mpa_arena.master, ref_master)


# ---------------------------------------------------------------- 7. two ranks, one GPU
_WORKER = r'''
import os, sys, torch
sys.path.insert(0, os.environ["PYTHONPATH"])
from mpi_pytorch_amd.parallel import init_world, shutdown
from mpi_pytorch_amd.engine import build_training
from mpi_pytorch_amd.ops import _ext
_ext.ext().set_deterministic(1)
w = init_world("cuda")
torch.manual_seed(0)
model, opt, step, _ = build_training(
    "resnet18", 100, w.device, w, 1e-3, "lamb", weight_decay=0.01,
    schedule=dict(kind="cosine", warmup_steps=2, total_steps=6, lr_min_ratio=0.1),
    clip_grad_norm=0.05)
g = torch.Generator().manual_seed(5)
X = (torch.randn(32, 64, 64, 8, generator=g) * (torch.arange(8) < 3)).to(torch.bfloat16)
Y = torch.randint(0, 100, (32,), generator=g)
n = 32 // w.world_size
x = X[w.rank * n:(w.rank + 1) * n].to(w.device)
y = Y[w.rank * n:(w.rank + 1) * n].to(w.device)
ratios = []
for _ in range(4):
    step(x, y)
    ratios.append(opt.seg_ratio.cpu().clone())
torch.cuda.synchronize()
torch.save({"master": model._mpa_arena.master.cpu(), "ratios": torch.stack(ratios),
            "norms": opt.seg_norms.cpu(), "scale": opt.grad_scale}, sys.argv[1] + str(w.rank))
shutdown()
'''


def test_lamb_two_ranks_one_gpu(gpu, tmp_path):
    """Both ranks norm the same all-reduced arena with the same fixed-order kernels: bitwise
    equal ratios on every step, bitwise equal replicas after four."""
    script = tmp_path / "w.py"
    script.write_text(_WORKER)
    out = tmp_path / "dp.pt"
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    env.update(MASTER_ADDR="127.0.0.1", MPA_DIST_BACKEND="gloo", PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "mpi_pytorch_amd.launch", "-n", "2", "--timeout", "200",
           str(script), str(out)]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    r0, r1 = torch.load(str(out) + "0"), torch.load(str(out) + "1")
    assert r0["scale"] == 0.5
    assert torch.equal(r0["master"], r1["master"])
    assert torch.equal(r0["ratios"], r1["ratios"]) and torch.equal(r0["norms"], r1["norms"])
    assert not torch.equal(r0["ratios"][0], r0["ratios"][3])
    assert bool((r0["ratios"] > 0).all()) and bool(torch.isfinite(r0["ratios"]).all())


# -------------------------------------------------------------------------- 8. checkpoint
@pytest.mark.parametrize("kind", ["adamw", "lamb", "lars"])
def test_checkpoint_resume_is_bitwise(gpu, kind):
    def grads(params, i):
        gen = torch.Generator(device="cpu").manual_seed(100 + i)
        for p in params:
            p.grad.copy_(torch.randn(p.shape, generator=gen))

    def run(opt, arena, params, steps):
        for i in steps:
            arena.zero_grad()
            grads(params, i)
            opt.step()

    _m, arena, params, opt, state = _small(gpu, kind)
    opt.set_schedule("cosine", warmup_steps=1, total_steps=5)
    run(opt, arena, params, range(3))
    _m2, arena2, params2, opt2, _s = _small(gpu, kind)
    opt2.set_schedule("cosine", warmup_steps=1, total_steps=5)
    run(opt2, arena2, params2, range(2))
    sd = opt2.state_dict()
    # a fresh optimizer with other settings: the checkpoint's are restored
    _m3, arena3, params3, opt3, state3 = _small(gpu, kind, wd_exclude_1d=False)
    opt3.load_state_dict(sd)
    assert opt3.wd_exclude_1d and torch.equal(opt3.plan_seg, opt.plan_seg)
    arena3.master.copy_(arena2.master)
    arena3.sync_shadow()
    run(opt3, arena3, params3, [2])
    assert float(opt3.step_t) == 3.0
    assert torch.equal(arena3.master, arena.master) and torch.equal(arena3.shadow, arena.shadow)
    for a, b in zip(state3, state):
        assert torch.equal(a, b)
    assert opt3.last_trust_ratios() == opt.last_trust_ratios()
