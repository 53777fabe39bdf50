"""Weight EMA on the flat arena: the two kernels against their fp32 oracle (bitwise), the
update inside the training step (eager and graph replay), ``swapped_in()``, checkpoint
resume and two data-parallel ranks.

The kernel checks take the implementation as an argument: ``tests/test_ema_cpu.py`` runs
them with ``ops/ref.py`` as that implementation, so a GPU failure is the kernel's.

A zero's sign: ``ema + w * (p - ema)`` with ``p == ema == -0`` is ``-0 + +0 = +0`` in IEEE
arithmetic, so the fixed point is bitwise for every value except ``-0``, which becomes
``+0`` (kernel and oracle agree on it; the fixed-point check asserts both)."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from mpi_pytorch_amd.checkpoint import build_state, load_checkpoint, _to_cpu
from mpi_pytorch_amd.engine import build_training
from mpi_pytorch_amd.ops import ref
from mpi_pytorch_amd.parallel import World

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 777.25
GUARD = 64  # sentinel elements on each side of a window (keeps it 16-B aligned)
# 64: one wave; 1088: a partial block; 4096 blocks x 256 threads x 4 elements + 192: one
# element group past the full grid, so the grid-stride loop takes a second trip (for 48
# threads); twice that + 192: a third
FULL_GRID = 4096 * 256 * 4
SIZES = (64, 1088, FULL_GRID + 192, 2 * FULL_GRID + 192)


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


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def specials(n, seed, neg_zero=True):
    """N(0, 1) values with +0, -0, denormals of both signs and +-1e30 sprinkled in."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g)
    x[0::7] = 0.0
    if neg_zero:
        x[1::7] = -0.0
    x[2::11] = 1e-40
    x[3::11] = -3e-39
    x[4::13] = 1e30
    x[5::13] = -1e30
    return x


def window(vals, dev):
    """``vals`` as a window of a larger sentinel-filled buffer on ``dev``."""
    n = vals.numel()
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    win = buf[GUARD:GUARD + n]
    win.copy_(vals)
    return buf, win


def guards_untouched(buf, n):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())


# ------------------------------------------------------------------- 1. ema_update
def check_ema_update(k, dev, n, t, warmup, decay=0.9998):
    p = specials(n, 1)
    e0 = specials(n, 2).roll(3)  # (so zeros / denormals / 1e30 meet other kinds in p)
    pd = p.to(dev)
    buf, win = window(e0, dev)
    step = torch.tensor([float(t)], device=dev)
    k.ema_update(win, pd, step, decay, warmup)
    want = e0.clone()
    ref.ema_update(want, p, step.cpu(), decay, warmup)
    assert same_bits(win, want)
    assert guards_untouched(buf, n)
    assert same_bits(pd, p)
    assert not same_bits(win, e0)


@pytest.mark.parametrize("warmup", [True, False])
@pytest.mark.parametrize("t", [1, 9, 10000])
@pytest.mark.parametrize("n", SIZES)
def test_ema_update_matches_oracle_bitwise(gpu, n, t, warmup):
    check_ema_update(C(), gpu, n, t, warmup)


def check_fixed_point(k, dev, n=1088):
    """ema == p stays bitwise p (and -0 becomes +0, see the module docstring)."""
    for t in (0, 1, 9, 10000, 10 ** 6):
        for warmup in (True, False):
            p = specials(n, 3, neg_zero=False)
            e = p.clone().to(dev)
            k.ema_update(e, p.to(dev), torch.tensor([float(t)], device=dev), 0.9998, warmup)
            assert same_bits(e, p), (t, warmup)
            z = torch.full((64,), -0.0)
            e = z.clone().to(dev)
            k.ema_update(e, z.to(dev), torch.tensor([float(t)], device=dev), 0.9998, warmup)
            assert same_bits(e, torch.zeros(64))


def test_fixed_point(gpu):
    check_fixed_point(C(), gpu)


def expected_weight(t, decay, warmup=True):
    f = np.float32
    d = f(decay)
    if warmup:
        d = min(d, (f(1) + f(t)) / (f(10) + f(t)))
    return f(1) - d


def check_weight_readback(k, dev, decay=0.9):
    """p = 1, ema = 0: the result is w itself."""
    for t in (0, 1, 8, 9, 89, 10 ** 6):
        e = torch.zeros(64, device=dev)
        k.ema_update(e, torch.ones(64, device=dev), torch.tensor([float(t)], device=dev), decay,
                     True)
        w = expected_weight(t, decay)
        assert same_bits(e, torch.full((64,), float(w))), t
        if (1 + t) / (10 + t) >= decay:  # past the warm-up: the decay itself
            assert same_bits(e, torch.full((64,), float(np.float32(1) - np.float32(decay)))), t
        else:
            assert float(w) > 1 - decay


def test_weight_readback(gpu):
    check_weight_readback(C(), gpu)


def check_closed_form(k, dev, decay=0.99, steps=200):
    """p constant c, ema_0 = 0, no warm-up: |ema_k - c (1 - d^k)| <= 4 k 2^-24 |c| (three
    roundings per step; 1 - d is exact in fp32 for d in [0.5, 1))."""
    c = torch.tensor([1.0, -1.0, 3.7, -0.3, 1e-3, 12345.678, 1e20, -7e-20] * 8)
    e = torch.zeros(64, device=dev)
    cd = c.to(dev)
    step = torch.zeros(1, device=dev)
    for _ in range(steps):
        k.ema_update(e, cd, step, decay, False)
    d = float(np.float32(decay))
    want = c.double() * (1.0 - d ** steps)
    err = (e.double().cpu() - want).abs()
    bound = 4 * steps * 2.0 ** -24 * c.double().abs()
    assert bool((err <= bound).all()), (err / bound).max()


def test_closed_form(gpu):
    check_closed_form(C(), gpu)


# -------------------------------------------------------------- 2. ema_update_multi
MULTI_LENGTHS = (1, 3, 64, 65, 1000, 2051)


class _Buffers(torch.nn.Module):
    """A parameter, float buffers of MULTI_LENGTHS (the 65-element one a slice that starts
    at an odd element of a larger tensor) and an int64 buffer."""

    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(40, 70)
        g = torch.Generator().manual_seed(7)
        self.big = torch.randn(200, generator=g)  # (not a buffer: b3 is a view into it)
        for i, ln in enumerate(MULTI_LENGTHS):
            self.register_buffer("b%d" % i, torch.randn(ln, generator=g))
        self.register_buffer("count", torch.tensor([5, 6, 7], dtype=torch.int64))

    def place(self, dev):
        self.to(dev)
        self.big = self.big.to(dev)
        self.b3 = self.big[3:3 + 65]
        return self


def check_ema_multi(k, dev):
    from mpi_pytorch_amd.ema import ModelEMA
    from mpi_pytorch_amd.optim import FusedAdam
    from mpi_pytorch_amd.parallel.arena import ParamArena
    model = _Buffers().place(dev)
    assert model.b3.data_ptr() % 16 != 0 and model.b3.data_ptr() == model.big.data_ptr() + 12
    model._mpa_arena = ParamArena(model, dev)
    opt = FusedAdam(list(model.parameters()), model._mpa_arena)
    ema = ModelEMA(model, opt, 0.9, True)
    rows = ema.table_host.tolist()
    assert [r[2] for r in rows] == list(MULTI_LENGTHS)  # the int64 buffer has no row
    assert [r[0] for r in rows] == [b.data_ptr() for b in ema.buffers]
    assert all(r[1] % 4 == 0 for r in rows)
    assert torch.equal(ema.table.cpu(), ema.table_host)
    total = ema.ema_buf.numel()
    e0 = specials(total, 11)
    buf, ebuf = window(e0, dev)
    big0 = model.big.clone()
    srcs0 = [b.clone() for b in ema.buffers]
    want = e0.clone()
    for t in (2.0, 10000.0):  # the second call: another t, the same table
        step = torch.tensor([t], device=dev)
        k.ema_update_multi(ebuf, ema.table, ema.table_host, ema.buffers, step, 0.9, True)
        ref.ema_update_multi(want, ema.table_host, ema.table_host,
                             [b.cpu() for b in ema.buffers], step.cpu(), 0.9, True)
        assert same_bits(ebuf, want), t  # (slots and the padding between them)
    assert guards_untouched(buf, total)
    covered = torch.zeros(total, dtype=torch.bool)
    for _a, off, ln in rows:
        covered[off:off + ln] = True
    assert same_bits(ebuf.cpu()[~covered], e0[~covered]) and int((~covered).sum()) > 0
    assert not same_bits(ebuf.cpu()[covered], e0[covered])
    assert same_bits(model.big, big0)
    assert all(same_bits(a, b) for a, b in zip(ema.buffers, srcs0))
    assert model.count.tolist() == [5, 6, 7]


def test_ema_update_multi_matches_oracle_bitwise(gpu):
    check_ema_multi(C(), gpu)


def test_ema_update_multi_rejects_a_moved_source(gpu):
    """The binding checks the sources against the table's host twin."""
    k = C()
    src = torch.randn(65, device=gpu)
    ebuf = torch.zeros(128, device=gpu)
    th = torch.tensor([[src.data_ptr(), 0, 65]], dtype=torch.int64)
    step = torch.ones(1, device=gpu)
    k.ema_update_multi(ebuf, th.to(gpu), th, [src], step, 0.9, True)
    with pytest.raises(RuntimeError, match="does not describe"):
        k.ema_update_multi(ebuf, th.to(gpu), th, [src.clone()], step, 0.9, True)
    far = torch.tensor([[src.data_ptr(), 100, 65]], dtype=torch.int64)
    with pytest.raises(RuntimeError, match="outside ema_buf"):
        k.ema_update_multi(ebuf, far.to(gpu), far, [src], step, 0.9, True)


# ------------------------------------------------------------- 3. inside the training step
# decay 0.25: (1 + t) / (10 + t) is below it at t = 1, equal at t = 2 and above it at t = 3,
# so three steps take both branches of the warm-up
DECAY = 0.25


def _train(gpu, ema_decay, seed=0, **kw):
    torch.manual_seed(seed)
    return build_training("resnet18", 10, gpu, World(device=gpu), 1e-3, ema_decay=ema_decay,
                          **kw)[:3]


def _batch(gpu, B=8, hw=32, nc=10, seed=1):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = (torch.randn(B, hw, hw, 8, generator=g) * (torch.arange(8) < 3)).to(gpu, torch.bfloat16)
    y = torch.randint(0, nc, (B,), generator=g).to(gpu)
    return x, y


def _state(model, opt, step):
    a = model._mpa_arena
    out = {"master": a.master.clone(), "m": opt.exp_avg.clone(), "v": opt.exp_avg_sq.clone(),
           "bufs": [b.clone() for b in model.buffers()]}
    if step.ema is not None:
        out["ema"], out["ema_buf"] = step.ema.ema.clone(), step.ema.ema_buf.clone()
    return out


_EAGER = {}


def _eager(gpu, steps):
    """``steps`` eager steps with the EMA on, once per session: losses, final state and the
    host replay's inputs (master / buffer snapshots after each step)."""
    if steps not in _EAGER:
        x, y = _batch(gpu)
        model, opt, step = _train(gpu, DECAY)
        e = step.ema
        n = e.arena.n_train
        start = (e.ema.cpu().clone(), e.ema_buf.cpu().clone())
        losses, snaps = [], []
        for _ in range(steps):
            losses.append(step(x, y).clone())
            snaps.append((e.arena.master[:n].cpu().clone(), [b.cpu().clone() for b in e.buffers]))
        torch.cuda.synchronize()
        _EAGER[steps] = dict(loss=torch.stack(losses), state=_state(model, opt, step), snaps=snaps,
                             start=start, table=e.table_host.clone(), n=n)
    return _EAGER[steps]


def _assert_state_equal(a, b, keys=None):
    for k in keys or a:
        if k == "bufs":
            assert all(torch.equal(u, v) for u, v in zip(a[k], b[k])), k
        else:
            assert torch.equal(a[k], b[k]), k


def test_ema_does_not_perturb_training_and_equals_host_replay(det):
    gpu = det
    r = _eager(gpu, 3)
    x, y = _batch(gpu)
    model, opt, step = _train(gpu, 0.0)
    assert step.ema is None
    loss = torch.stack([step(x, y).clone() for _ in range(3)])
    torch.cuda.synchronize()
    assert torch.equal(loss, r["loss"])
    _assert_state_equal(_state(model, opt, step), r["state"], ("master", "m", "v", "bufs"))
    # host replay of the oracle over the snapshots
    n = r["n"]
    ema, ema_buf = r["start"][0].clone(), r["start"][1].clone()
    for i, (master, bufs) in enumerate(r["snaps"]):
        t = torch.tensor([float(i + 1)])
        ref.ema_update(ema[:n], master, t, DECAY, True)
        ref.ema_update_multi(ema_buf, r["table"], r["table"], bufs, t, DECAY, True)
    assert same_bits(r["state"]["ema"], ema)
    assert same_bits(r["state"]["ema_buf"], ema_buf)
    assert not same_bits(ema[:n], r["snaps"][-1][0])  # an average, not the last iterate


def test_graph_replays_bitwise_equal_eager(det):
    gpu = det
    r = _eager(gpu, 3)
    x, y = _batch(gpu)
    model, opt, step = _train(gpu, DECAY)
    before = _state(model, opt, step)
    assert step.capture(x, y, warmup=2)
    torch.cuda.synchronize()
    assert float(opt.step_t) == 0.0
    _assert_state_equal(_state(model, opt, step), before)  # the warm-up steps are rolled back
    loss = torch.stack([step(x, y).clone() for _ in range(3)])
    torch.cuda.synchronize()
    assert torch.equal(loss, r["loss"])
    _assert_state_equal(_state(model, opt, step), r["state"])


# ------------------------------------------------------------------------ 4. swapped_in
def test_swapped_in_shows_the_averaged_model_and_restores_the_live_one(det):
    gpu = det
    x, y = _batch(gpu)
    model, opt, step = _train(gpu, DECAY)
    for _ in range(2):
        step(x, y)
    ema, a = step.ema, model._mpa_arena

    def live():
        return [a.master.clone(), a.shadow.clone(), a.shadow_t.clone()] + \
            [b.clone() for b in model.buffers()]

    before = live()
    sd = ema.state_dict()
    assert all(torch.equal(u, v) for u, v in zip(live(), before))
    model.eval()
    with torch.no_grad():
        out_live = model(x).float().clone()
        with ema.swapped_in() as m:
            assert m is model
            out_in = model(x).float().clone()
            assert torch.equal(a.master[:a.n_train], ema.ema[:a.n_train])
            inside = {k: v.clone() for k, v in model.state_dict().items()}
    assert all(torch.equal(u, v) for u, v in zip(live(), before))
    assert not torch.equal(out_in, out_live)
    assert set(inside) == set(sd) and all(torch.equal(inside[k], sd[k]) for k in sd)
    assert tuple(sd["conv1.weight"].shape) == (64, 3, 7, 7)  # torchvision's OIHW
    # a fresh model (other initial weights) loaded from the EMA's state dict
    fresh, _o, _s = _train(gpu, 0.0, seed=5)
    fresh.load_state_dict(sd)
    fresh._mpa_arena.sync_shadow()
    fresh.eval()
    with torch.no_grad():
        out_fresh = fresh(x).float()
    assert torch.equal(out_in, out_fresh)
    # the body raises: restored all the same
    with pytest.raises(KeyError, match="boom"):
        with ema.swapped_in():
            assert not torch.equal(a.master, before[0])
            raise KeyError("boom")
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(live(), before))


# ------------------------------------------------------------------------ 5. checkpoint
def test_checkpoint_resume_is_bitwise(det):
    """Two steps, save, rebuild, load, two more == four uninterrupted steps, for the weights
    and for the EMA (the file goes through torch.save / weights_only loading in memory)."""
    gpu = det
    x, y = _batch(gpu)
    r = _eager(gpu, 4)
    model, opt, step = _train(gpu, DECAY)
    for _ in range(2):
        step(x, y)
    f = io.BytesIO()
    state = build_state(0, model, opt, 0.0, step.ema)
    assert set(state) == {"epoch", "state_dict", "optimizer", "loss", "ema_state_dict", "ema"}
    assert state["ema"] == {"decay": DECAY, "warmup": True}
    torch.save(_to_cpu(state), f)
    del model, opt, step, state
    model, opt, step = _train(gpu, DECAY, seed=9)  # other initial weights
    f.seek(0)
    load_checkpoint(f, model, opt, ema=step.ema)
    assert float(opt.step_t) == 2.0
    for _ in range(2):
        step(x, y)
    torch.cuda.synchronize()
    _assert_state_equal(_state(model, opt, step), r["state"])


# ---------------------------------------------------------------- 6. two ranks, one GPU
_WORKER = r'''
import os, sys, torch
sys.path.insert(0, os.environ["PYTHONPATH"])
from mpi_pytorch_amd.parallel import init_world, shutdown
from mpi_pytorch_amd.engine import build_training
from mpi_pytorch_amd.ops import _ext
_ext.ext().set_deterministic(1)
w = init_world("cuda")
torch.manual_seed(w.rank)  # (different initial weights: sync_params makes them rank 0's)
model, opt, step, _ = build_training("resnet18", 10, w.device, w, 1e-3, ema_decay=0.25)
g = torch.Generator().manual_seed(5)
X = (torch.randn(16, 32, 32, 8, generator=g) * (torch.arange(8) < 3)).to(torch.bfloat16)
Y = torch.randint(0, 10, (16,), generator=g)
n = 16 // w.world_size
x = X[w.rank * n:(w.rank + 1) * n].to(w.device)
y = Y[w.rank * n:(w.rank + 1) * n].to(w.device)
for _ in range(3):
    step(x, y)
torch.cuda.synchronize()
a = model._mpa_arena
torch.save({"master": a.master[:a.n_train].cpu(), "ema": step.ema.ema[:a.n_train].cpu()},
           sys.argv[1] + str(w.rank))
shutdown()
'''


def test_ema_two_ranks_one_gpu(gpu, tmp_path):
    """Every rank keeps its own average and nothing is communicated: identical weights give
    bitwise identical parameter averages."""
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
    assert torch.equal(r0["master"], r1["master"])
    assert same_bits(r0["ema"], r1["ema"])
    assert not torch.equal(r0["ema"], r0["master"])
