"""Training recipe on the device (csrc/kernels/optim.hip): the fixed-order gradient norm,
the hyper record (LR schedule + clip coefficient + non-finite skip), the device-argument
optimizer kernels, and the whole step under HIP-graph replay and with two ranks.

The reference has no schedule and no clipping (``main.py:125,155`` there: Adam
at a constant LR); the oracles here are optim.py's formulas in Python float64 and the
existing host-argument kernels."""
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

# one full-grid sweep of adam_kernel / sgd_kernel: blocks_for()'s 4,096-block cap x 256
# threads x one float4 each
OPT_SWEEP = 4096 * 256 * 4


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


def lr_f64(base, k, kind, W, T, r=0.0, gamma=0.1, decay=1):
    if k < W:
        return base * (k + 1) / W
    if kind == "cosine":
        if k >= T:
            return base * r
        p = (k - W) / max(1, T - W)
        return base * (r + (1 - r) * 0.5 * (1 + math.cos(math.pi * p)))
    if kind == "step":
        return base * gamma ** (k // decay)
    return base


# ------------------------------------------------------------------------------- norm
def _sqnorm(g):
    k = C()
    ws = torch.zeros(k.grad_sqnorm_grid_cap(), device=g.device)
    out = torch.zeros(1, device=g.device)
    n = k.grad_sqnorm(g, ws)
    assert 0 < n <= ws.numel() and n % 8 == 0  # a multiple of the XCD count
    k.grad_sqnorm_sum(ws, n, out)
    return out


def _norm_sizes():
    # one arena slot; 17 slots (no multiple of a block's 8,192 elements); one full sweep of
    # the norm kernel's capped grid (cap x 256 threads x 8 float4 per thread) + one slot
    return [ALIGN, ALIGN * 17, int(C().grad_sqnorm_sweep()) + ALIGN]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_grad_sqnorm(gpu, which):
    n = _norm_sizes()[which]
    assert C().grad_sqnorm_sweep() == C().grad_sqnorm_grid_cap() * 256 * 8 * 4
    gen = torch.Generator(device=gpu).manual_seed(which)
    # small integers, sparse enough that every partial sum stays below 2^24: exact in fp32
    g = torch.randint(-3, 4, (n,), device=gpu, generator=gen).float()
    if n > 4096:
        g *= (torch.rand(n, device=gpu, generator=gen) < 1 / 16)
    g[-1] = 3.0  # (the very last element is read)
    exact = float((g.double() ** 2).sum())
    assert exact < 2 ** 24
    assert float(_sqnorm(g)) == exact
    # random values: fp32 accumulation (<= a few thousand addends per thread + a tree)
    g = torch.randn(n, device=gpu, generator=gen)
    want = float((g.double() ** 2).sum())
    old = C().deterministic()
    C().set_deterministic(0)  # reproducible in every mode, not only the deterministic one
    try:
        a, b = _sqnorm(g), _sqnorm(g)
    finally:
        C().set_deterministic(int(old))
    assert abs(float(a) - want) <= 1e-5 * want, (float(a), want)
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------ hyper
W_, T_, BASE = 5, 50, 3e-3


def _hyper(k, kind="constant", r=0.0, gamma=0.1, decay=0, sumsq=None, max_norm=0.0, gs=1.0,
           hyper=None):
    dev = torch.device("cuda", 0)
    step = torch.full((1,), float(k), device=dev)
    hyper = torch.zeros(ref.HYPER_N, device=dev) if hyper is None else hyper
    ws = torch.zeros(C().grad_sqnorm_grid_cap(), device=dev)
    nparts = 0
    if sumsq is not None:
        ws[0] = sumsq
        nparts = 8
    C().hyper_update(step, hyper, ws, nparts, ref.SCHEDULE_KINDS.index(kind), BASE, W_, T_, r,
                     gamma, decay, max_norm, gs)
    return hyper.cpu()


@pytest.mark.parametrize("kind,r", [("constant", 0.0), ("cosine", 0.0), ("cosine", 0.1),
                                    ("step", 0.0)])
def test_hyper_schedule(gpu, kind, r):
    for k in (0, W_ - 1, W_, (W_ + T_) // 2, T_ - 1, T_, T_ + 5):
        h = _hyper(k, kind, r=r, gamma=0.5, decay=10)
        want = lr_f64(BASE, k, kind, W_, T_, r, 0.5, 10)
        assert abs(float(h[ref.HYPER_LR]) - want) <= 1e-6 * BASE, (kind, k, float(h[0]), want)
        # no clipping: the scale is the plain grad scale, nothing is skipped
        assert float(h[ref.HYPER_SCALE]) == 1.0 and float(h[ref.HYPER_SKIP]) == 0.0


def test_hyper_clip(gpu):
    third = float(np.float32(1.0 / 3.0))
    # below max_norm: coef exactly 1, the effective scale bitwise the grad scale
    for gs in (1.0, 0.5, third):
        h = _hyper(3, sumsq=4.0, max_norm=2.0 * gs + 1e-3, gs=gs)
        assert float(h[ref.HYPER_COEF]) == 1.0
        assert float(h[ref.HYPER_SCALE]) == float(np.float32(gs))
        assert abs(float(h[ref.HYPER_NORM]) - 2.0 * gs) <= 1e-6
    # total == max_norm exactly still counts as "not above"
    h = _hyper(3, sumsq=4.0, max_norm=2.0, gs=1.0)
    assert float(h[ref.HYPER_COEF]) == 1.0 and float(h[ref.HYPER_SCALE]) == 1.0
    # above: torch's coefficient
    for gs in (1.0, 0.5):
        sumsq = float(np.float32(1234.5678))
        h = _hyper(3, sumsq=sumsq, max_norm=0.7, gs=gs)
        total = gs * math.sqrt(sumsq)
        coef = min(1.0, 0.7 / (total + 1e-6))
        assert abs(float(h[ref.HYPER_COEF]) - coef) <= 1e-6 * coef
        assert abs(float(h[ref.HYPER_SCALE]) - gs * coef) <= 1e-6 * gs * coef
        assert abs(float(h[ref.HYPER_NORM]) - total) <= 1e-6 * total
        assert float(h[ref.HYPER_SKIP]) == 0.0 and float(h[ref.HYPER_NONFINITE]) == 0.0
    # inf / NaN sum of squares: skip flag, counter + 1 (it accumulates in the record)
    hy = None
    for i, bad in enumerate((float("inf"), float("nan"))):
        hy = _hyper(3, sumsq=bad, max_norm=0.7, hyper=None if hy is None else hy.cuda())
        assert float(hy[ref.HYPER_SKIP]) == 1.0 and float(hy[ref.HYPER_NONFINITE]) == i + 1


# ------------------------------------------------- device-argument optimizer kernels
def _opt_inputs(gpu, n, seed):
    gen = torch.Generator(device=gpu).manual_seed(seed)
    p = torch.randn(n, device=gpu, generator=gen)
    g = torch.randn(n, device=gpu, generator=gen) * 0.1
    return p, g


def _hyper_with(gpu, lr, gs):
    h = torch.zeros(ref.HYPER_N, device=gpu)
    h[ref.HYPER_LR] = lr
    h[ref.HYPER_SCALE] = gs
    return h, float(h[ref.HYPER_LR]), float(h[ref.HYPER_SCALE])  # the fp32 values


@pytest.mark.parametrize("n", [ALIGN, OPT_SWEEP + ALIGN])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("shadow", [True, False])
def test_adam_step_dev_bitwise(gpu, n, wd, shadow):
    p, g = _opt_inputs(gpu, n, 1)
    h, lr, gs = _hyper_with(gpu, 1e-2 / 3, 1.0 / 3)
    none = torch.empty(0, device=gpu)
    a = [p.clone(), torch.zeros(n, device=gpu), torch.zeros(n, device=gpu),
         torch.zeros(n, dtype=torch.bfloat16, device=gpu) if shadow else none]
    b = [t.clone() for t in a]
    for t in (0.0, 7.0):  # the first and a later step
        st = torch.full((1,), t, device=gpu)
        C().adam_step(a[0], g, a[1], a[2], a[3], st, lr, 0.9, 0.999, 1e-8, wd, gs)
        C().adam_step_dev(b[0], g, b[1], b[2], b[3], st, h, 0.9, 0.999, 1e-8, wd)
        for u, v in zip(a, b):
            assert torch.equal(u, v)
    assert not torch.equal(a[0], p)


@pytest.mark.parametrize("n", [ALIGN, OPT_SWEEP + ALIGN])
@pytest.mark.parametrize("wd,shadow", [(0.0, True), (0.01, False)])
@pytest.mark.parametrize("nesterov", [False, True])
def test_sgd_step_dev_bitwise(gpu, n, wd, shadow, nesterov):
    p, g = _opt_inputs(gpu, n, 2)
    h, lr, gs = _hyper_with(gpu, 0.1 / 3, 1.0 / 3)
    none = torch.empty(0, device=gpu)
    a = [p.clone(), torch.zeros(n, device=gpu),
         torch.zeros(n, dtype=torch.bfloat16, device=gpu) if shadow else none]
    b = [t.clone() for t in a]
    for t in (0.0, 4.0):  # the first step seeds the momentum buffer
        st = torch.full((1,), t, device=gpu)
        C().sgd_step(a[0], g, a[1], a[2], st, lr, 0.9, 0.0, wd, nesterov, gs)
        C().sgd_step_dev(b[0], g, b[1], b[2], st, h, 0.9, 0.0, wd, nesterov)
        for u, v in zip(a, b):
            assert torch.equal(u, v)
    assert not torch.equal(a[0], p)


# -------------------------------------------------------------------------------- skip
def _padding_mask(arena):
    pad = torch.ones(arena.n_train, dtype=torch.bool)
    for p in arena.trainable:
        o, e = arena.slice_of(p)
        pad[o:e] = False
    return pad


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_nonfinite_step_is_skipped(gpu, kind):
    from mpi_pytorch_amd.optim import FusedAdam, FusedSGD
    from mpi_pytorch_amd.parallel.arena import ParamArena
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(40, 70), torch.nn.Linear(70, 9)).to(gpu)
    arena = ParamArena(model, gpu)
    params = list(model.parameters())
    opt = FusedAdam(params, arena, lr=1e-2) if kind == "adam" else \
        FusedSGD(params, arena, lr=1e-2, momentum=0.9)
    opt.set_clip(1.0)
    state = [opt.exp_avg, opt.exp_avg_sq] if kind == "adam" else [opt.momentum_buffer]
    for t in state:
        t.normal_().abs_()  # (non-zero state; Adam's second moment is never negative)
    before = [t.clone() for t in [arena.master, arena.shadow] + state]
    arena.zero_grad()
    for p in params:
        p.grad.fill_(0.5)
    params[1].grad.view(-1)[5] = float("inf")
    opt.step()
    for t, c in zip([arena.master, arena.shadow] + state, before):
        assert torch.equal(t, c)
    assert opt.nonfinite_steps() == 1 and float(opt.step_t) == 1.0  # the step still counts
    assert math.isinf(opt.last_grad_norm())
    arena.zero_grad()
    for p in params:
        p.grad.fill_(0.5)
    opt.step()
    assert not torch.equal(arena.master, before[0]) and not torch.equal(state[0], before[2])
    assert torch.equal(arena.shadow[:arena.n_train],
                       arena.master[:arena.n_train].to(torch.bfloat16))
    assert opt.nonfinite_steps() == 1 and float(opt.step_t) == 2.0
    # the norm runs over the padded arena: its padding is zero and stays zero
    pad = _padding_mask(arena)
    assert pad.any() and not arena.grad[:arena.n_train].cpu()[pad].any()
    want = float(arena.grad[:arena.n_train].double().norm())
    assert abs(opt.last_grad_norm() - want) <= 1e-5 * want


# -------------------------------------------------------------------------- end to end
SCHED = dict(kind="cosine", warmup_steps=3, total_steps=8, lr_min_ratio=0.0)


def _train(gpu, max_norm, seed=0):
    torch.manual_seed(seed)
    return build_training("resnet18", 100, gpu, World(device=gpu), 1e-3,
                          schedule=SCHED if max_norm else None,
                          clip_grad_norm=max_norm)[:3]


def _batch(gpu, B=32, hw=64, nc=100, seed=1):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = (torch.randn(B, hw, hw, 8, generator=g) * (torch.arange(8) < 3)).to(gpu, torch.bfloat16)
    y = torch.randint(0, nc, (B,), generator=g).to(gpu)
    return x, y


def test_recipe_graph_replays_bitwise_equal_eager(det):
    """ResNet-18, warm-up 3 + cosine over 8 steps, clipping active: 6 graph replays == 6
    eager steps bitwise, and the replayed learning rate moves with the device step counter
    (a host-float LR would be frozen into the graph)."""
    gpu = det
    x, y = _batch(gpu)
    # the first step's gradient norm, measured on the plain path; clip to half of it
    model, opt, step = _train(gpu, 0.0)
    step(x, y)
    n0 = float(model._mpa_arena.grad.double().norm())
    del model, opt, step
    max_norm = 0.5 * n0
    # eager
    model, opt, step = _train(gpu, max_norm)
    assert opt.recipe_on
    ref_loss = torch.stack([step(x, y).clone() for _ in range(6)])
    torch.cuda.synchronize()
    a = model._mpa_arena
    ref_master = a.master.clone()
    want = opt.grad_scale * float(a.grad[:a.n_train].double().norm())
    assert abs(opt.last_grad_norm() - want) <= 1e-5 * want, (opt.last_grad_norm(), want)
    assert float(opt.hyper[ref.HYPER_COEF]) < 1.0 or want <= max_norm
    # padding stays zero after a step (this model's parameters happen to fill their slots;
    # test_nonfinite_step_is_skipped asserts the same on an arena that has padding)
    assert not a.grad[:a.n_train].cpu()[_padding_mask(a)].any()
    assert opt.nonfinite_steps() == 0
    del model, opt, step
    # graph
    model, opt, step = _train(gpu, max_norm)
    assert step.capture(x, y, warmup=2)
    assert float(opt.step_t) == 0.0  # capture's warm-up steps were rolled back
    got, lrs, coefs = [], {}, []
    for i in range(6):
        got.append(step(x, y).clone())
        if i in (0, 4):
            lrs[i] = opt.current_lr()
        if i == 0:
            coefs.append(float(opt.hyper[ref.HYPER_COEF]))
            assert abs(opt.last_grad_norm() - n0) <= 1e-5 * n0  # the first step's norm
    torch.cuda.synchronize()
    assert coefs[0] < 1.0  # clipping was active
    assert lrs[0] != lrs[4]
    for i in (0, 4):
        want = lr_f64(1e-3, i, "cosine", 3, 8)
        assert abs(lrs[i] - want) <= 1e-6 * 1e-3, (i, lrs[i], want)
    assert torch.equal(torch.stack(got), ref_loss)
    assert torch.equal(model._mpa_arena.master, ref_master)


# ---------------------------------------------------------------- two ranks on one GPU
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
    "resnet18", 100, w.device, w, 1e-2, "sgd",
    schedule=dict(kind="cosine", warmup_steps=2, total_steps=6, lr_min_ratio=0.1),
    clip_grad_norm=0.05)
g = torch.Generator().manual_seed(5)
X = (torch.randn(32, 64, 64, 8, generator=g) * (torch.arange(8) < 3)).to(torch.bfloat16)
Y = torch.randint(0, 100, (32,), generator=g)
n = 32 // w.world_size
x = X[w.rank * n:(w.rank + 1) * n].to(w.device)
y = Y[w.rank * n:(w.rank + 1) * n].to(w.device)
norms = []
for _ in range(3):
    step(x, y)
    norms.append(opt.last_grad_norm())
torch.cuda.synchronize()
torch.save({"master": model._mpa_arena.master.cpu(), "norms": norms, "lr": opt.current_lr(),
            "coef": float(opt.hyper[3]), "scale": opt.grad_scale}, sys.argv[1] + str(w.rank))
shutdown()
'''


def test_recipe_two_ranks_one_gpu(gpu, tmp_path):
    """Both ranks take the norm of the same all-reduced arena with the same fixed-order
    kernel: equal norms, equal clip coefficient, bitwise equal replicas."""
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
    assert r0["norms"] == r1["norms"] and r0["lr"] == r1["lr"] and r0["coef"] == r1["coef"]
    assert r0["coef"] < 1.0 and all(n > 0 for n in r0["norms"])
    assert abs(r0["lr"] - lr_f64(1e-2, 2, "cosine", 2, 6, 0.1)) <= 1e-6 * 1e-2
