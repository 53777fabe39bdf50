"""Training recipe (per-step LR schedule + global-norm gradient clipping) on the CPU path:
the fp32 oracles of ``ops/ref.py`` behind ``FusedAdam`` / ``FusedSGD``, checked against
``torch.optim`` + ``clip_grad_norm_`` + ``LambdaLR``; the checkpoint format; the config
fields; the training driver's metrics; two gloo ranks.

The reference trains with a constant ``LR`` and no gradient control
(``main.py:125,155`` there); the recipe is off by default and these tests cover
what it adds."""
import json
import math
import os
import socket
import tempfile

import pytest
import torch
import torch.multiprocessing as mp
import torch.nn as nn

from mpi_pytorch_amd.config import Config
from mpi_pytorch_amd.optim import FusedAdam, FusedSGD
from mpi_pytorch_amd.parallel.arena import ParamArena

BASE, W, T, R, MAX_NORM, GS = 1e-2, 3, 10, 0.1, 0.5, 0.5


def lr_f64(base, k, kind="cosine", W=W, T=T, r=R, gamma=0.1, decay=0):
    """The schedule of optim.py in Python float64; k = 0-based index of the update."""
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


def _tiny(seed=0):
    torch.manual_seed(seed)
    # (sizes that are no multiple of the arena's 64-element slots: padding in between)
    return nn.Sequential(nn.Linear(7, 33), nn.Tanh(), nn.Linear(33, 5))


def _grads(model, steps, seed=3):
    """Per-step gradients, the same for the engine and for torch: their norm (times GS)
    is above MAX_NORM on some steps and below it on others."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for s in range(steps):
        scale = 1.0 if s % 2 == 0 else 0.01
        out.append([torch.randn(p.shape, generator=g) * scale for p in model.parameters()])
    return out


def _make(kind, model, recipe):
    arena = ParamArena(model, torch.device("cpu"))
    params = list(model.parameters())
    if kind == "adam":
        opt = FusedAdam(params, arena, lr=BASE, weight_decay=0.01)
    else:
        opt = FusedSGD(params, arena, lr=BASE, momentum=0.9, weight_decay=0.01)
    opt.grad_scale = GS
    if recipe:
        opt.set_schedule("cosine", warmup_steps=W, total_steps=T, lr_min_ratio=R)
        opt.set_clip(MAX_NORM)
    return arena, opt


def _run_engine(kind, recipe, steps=10, stop=None):
    model = _tiny()
    arena, opt = _make(kind, model, recipe)
    lrs = []
    for gs in _grads(model, steps)[:stop]:
        arena.zero_grad()
        for p, g in zip(model.parameters(), gs):
            p.grad.copy_(g)
        opt.step()
        lrs.append(opt.current_lr())
    return model, arena, opt, lrs


def _run_torch(kind, recipe, steps=10):
    model = _tiny()
    params = list(model.parameters())
    if kind == "adam":
        opt = torch.optim.Adam(params, lr=BASE, weight_decay=0.01)
    else:
        opt = torch.optim.SGD(params, lr=BASE, momentum=0.9, weight_decay=0.01)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda k: lr_f64(BASE, k) / BASE) if recipe \
        else None
    clipped = 0
    for gs in _grads(model, steps):
        for p, g in zip(params, gs):
            p.grad = g.clone() * GS  # the averaged gradient
        if recipe:
            clipped += float(torch.nn.utils.clip_grad_norm_(params, MAX_NORM)) > MAX_NORM
        opt.step()
        if sched is not None:
            sched.step()
    return params, clipped


def _max_diff(model, params):
    return max(float((p.detach() - q.detach()).abs().max())
               for p, q in zip(model.parameters(), params))


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_recipe_matches_torch(kind):
    """10 steps with warm-up + cosine + clipping vs torch's optimizer, clip_grad_norm_ and
    LambdaLR on the same gradients.  Allowed: 4x the difference the EXISTING path (no
    schedule, no clip) shows against plain torch in the same setting, floor 1e-7."""
    model, _a, _o, _ = _run_engine(kind, recipe=False)
    params, _ = _run_torch(kind, recipe=False)
    base_diff = _max_diff(model, params)
    model, arena, opt, lrs = _run_engine(kind, recipe=True)
    params, clipped = _run_torch(kind, recipe=True)
    diff = _max_diff(model, params)
    print("%s: existing path vs torch %.3e, recipe vs torch %.3e" % (kind, base_diff, diff))
    assert 0 < clipped < 10  # both branches of the clip were taken
    assert diff <= max(4 * base_diff, 1e-7), (diff, base_diff)
    for k, lr in enumerate(lrs):
        assert abs(lr - lr_f64(BASE, k)) <= 1e-6 * BASE, (k, lr)
    assert opt.nonfinite_steps() == 0
    # the last step's norm: torch's total_norm of the averaged gradient
    want = GS * float(arena.grad.double().norm())
    assert abs(opt.last_grad_norm() - want) <= 1e-5 * want


def test_recipe_off_is_the_existing_path():
    model, arena, opt, lrs = _run_engine("adam", recipe=False, steps=2)
    assert not opt.recipe_on and opt.hyper is None and lrs == [BASE, BASE]
    with pytest.raises(RuntimeError):
        opt.last_grad_norm()
    with pytest.raises(ValueError):
        opt.set_schedule("linear")
    with pytest.raises(ValueError):
        opt.set_schedule("step", decay_steps=0)
    with pytest.raises(ValueError):
        opt.set_clip(-1.0)


def test_nonfinite_step_is_skipped_cpu():
    model = _tiny()
    arena, opt = _make("adam", model, recipe=True)
    before = arena.master.clone()
    arena.zero_grad()
    next(model.parameters()).grad.view(-1)[3] = float("inf")
    opt.step()
    assert torch.equal(arena.master, before) and float(opt.exp_avg.abs().sum()) == 0
    assert opt.nonfinite_steps() == 1 and float(opt.step_t) == 1.0  # the step still counts
    arena.zero_grad()
    for p in model.parameters():
        p.grad.fill_(0.01)
    opt.step()
    assert not torch.equal(arena.master, before) and opt.nonfinite_steps() == 1
    assert abs(opt.current_lr() - lr_f64(BASE, 1)) <= 1e-6 * BASE


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_checkpoint_with_recipe(kind, tmp_path):
    model, arena, opt, lrs = _run_engine(kind, recipe=True, stop=4)
    sd = opt.state_dict()
    g = sd["param_groups"][0]
    assert g["initial_lr"] == BASE and g["mpa_step"] == 4.0
    assert abs(g["lr"] - lr_f64(BASE, 3)) <= 1e-6 * BASE  # the last scheduled value
    assert g["mpa_schedule"]["kind"] == "cosine" and g["mpa_clip_grad_norm"] == MAX_NORM
    # torch.load(weights_only=True) accepts it, and torch's own optimizers load it
    path = str(tmp_path / "opt.pt")
    torch.save({"optimizer": sd}, path)
    sd = torch.load(path, weights_only=True)["optimizer"]
    params = [nn.Parameter(p.detach().clone()) for p in model.parameters()]
    if kind == "adam":
        torch.optim.Adam(params, lr=BASE).load_state_dict(sd)
    else:
        torch.optim.SGD(params, lr=BASE, momentum=0.9).load_state_dict(sd)
    # a fresh optimizer resumes the schedule: its 5th update uses the uninterrupted run's LR
    _m, _a, _o, full = _run_engine(kind, recipe=True, stop=5)
    model2 = _tiny()
    arena2, opt2 = _make(kind, model2, recipe=False)
    opt2.load_state_dict(sd)
    assert opt2.recipe_on and float(opt2.step_t) == 4.0 and opt2.lr == BASE
    arena2.master.copy_(arena.master)
    arena2.zero_grad()
    for p, gr in zip(model2.parameters(), _grads(model2, 5)[4]):
        p.grad.copy_(gr)
    opt2.step()
    assert opt2.current_lr() == full[4]
    assert abs(full[4] - lr_f64(BASE, 4)) <= 1e-6 * BASE
    m_full = _run_engine(kind, recipe=True, stop=5)[1].master
    assert torch.equal(arena2.master, m_full)


def test_sgd_checkpoint_remembers_its_step():
    model, arena, opt, _ = _run_engine("sgd", recipe=False, stop=3)
    model2 = _tiny()
    _a2, opt2 = _make("sgd", model2, recipe=False)
    opt2.load_state_dict(opt.state_dict())
    assert float(opt2.step_t) == 3.0


def test_config_fields(monkeypatch):
    c = Config()
    assert (c.lr_schedule, c.warmup_steps, c.lr_min_ratio, c.lr_gamma, c.lr_decay_steps,
            c.clip_grad_norm) == ("constant", 0, 0.0, 0.1, 0, 0.0) and not c.recipe_on
    c = Config.from_args(["--lr-schedule", "cosine", "--warmup_steps", "5", "--lr-min-ratio",
                          "0.05", "--clip-grad-norm", "1.5"])
    assert (c.lr_schedule, c.warmup_steps, c.lr_min_ratio, c.clip_grad_norm) == \
        ("cosine", 5, 0.05, 1.5) and c.recipe_on
    monkeypatch.setenv("MPA_LR_SCHEDULE", "step")
    monkeypatch.setenv("MPA_lr_decay_steps", "30")
    monkeypatch.setenv("MPA_LR_GAMMA", "0.5")
    c = Config.from_env()
    assert (c.lr_schedule, c.lr_decay_steps, c.lr_gamma) == ("step", 30, 0.5)
    monkeypatch.delenv("MPA_lr_decay_steps")
    with pytest.raises(ValueError):
        Config.from_env()  # step without lr_decay_steps
    monkeypatch.delenv("MPA_LR_SCHEDULE")
    for bad in (dict(lr_schedule="linear"), dict(warmup_steps=-1), dict(lr_min_ratio=1.5),
                dict(clip_grad_norm=-1.0), dict(lr_schedule="step", lr_decay_steps=0),
                dict(lr_schedule="step", lr_decay_steps=5, lr_gamma=0.0)):
        with pytest.raises(ValueError):
            Config(**bad)


def _reset_world():
    import mpi_pytorch_amd.parallel.dist as D
    D._WORLD = None


def test_training_driver_metrics(tmp_path):
    """2 epochs x 2 steps, warm-up 1 + cosine over the run's 4 steps + clipping: the
    metrics record carries lr / grad_norm / nonfinite_steps, lr following the schedule at
    the epoch boundaries; a default run's record has none of them."""
    from mpi_pytorch_amd.engine.trainer import run_training
    kw = dict(synthetic_images=32, image_size=32, NUM_EPOCHS=2, BATCH_SIZE=16, NUM_CLASSES=10,
              VALIDATE=False, device="cpu", watchdog_s=0)
    _reset_world()
    run_training(Config(CHECKPOINT_DIR=str(tmp_path) + "/a/", log_file=str(tmp_path / "a.log"),
                        metrics_jsonl=str(tmp_path / "a.jsonl"), lr_schedule="cosine",
                        warmup_steps=1, lr_min_ratio=0.1, clip_grad_norm=0.05, **kw))
    recs = [json.loads(l) for l in (tmp_path / "a.jsonl").read_text().splitlines()]
    assert len(recs) == 2
    for e, rec in enumerate(recs):
        k = 2 * e + 1  # the epoch's last update
        want = lr_f64(4e-4, k, W=1, T=4, r=0.1)
        assert abs(rec["lr"] - want) <= 1e-6 * 4e-4, (e, rec["lr"], want)
        assert rec["grad_norm"] > 0 and rec["nonfinite_steps"] == 0
    assert "_Epoch: 1 | Train Loss: " in (tmp_path / "a.log").read_text()
    _reset_world()
    run_training(Config(CHECKPOINT_DIR=str(tmp_path) + "/b/", log_file=str(tmp_path / "b.log"),
                        metrics_jsonl=str(tmp_path / "b.jsonl"), **kw))
    for line in (tmp_path / "b.jsonl").read_text().splitlines():
        assert not {"lr", "grad_norm", "nonfinite_steps"} & set(json.loads(line))
    _reset_world()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    from mpi_pytorch_amd.parallel import init_world, sync_params, shutdown
    from mpi_pytorch_amd.engine import build_model, loss_fn
    from mpi_pytorch_amd.optim import build_optimizer
    import mpi_pytorch_amd.parallel.dist as D
    D._WORLD = None
    w = init_world("cpu")
    torch.manual_seed(100 + rank)
    m, _ = build_model("alexnet", 10, False, torch.device("cpu"), w, bucket_mb=8.0, overlap=True)
    for mod in m.modules():
        if type(mod).__name__ == "Dropout":
            mod.p = 0.0
    sync_params(m)
    opt = build_optimizer("adam", m, 1e-3)
    opt.grad_scale = 1.0 / world
    opt.set_schedule("cosine", warmup_steps=2, total_steps=6, lr_min_ratio=0.1)
    opt.set_clip(0.05)
    g = torch.Generator().manual_seed(7)
    X = torch.randn(8, 95, 95, 3, generator=g)
    Y = torch.randint(0, 10, (8,), generator=g)
    per = 8 // world
    xs, ys = X[rank * per:(rank + 1) * per], Y[rank * per:(rank + 1) * per]
    norms = []
    for _ in range(3):
        m._mpa_arena.zero_grad()
        loss_fn(m(xs), ys).backward()
        m._mpa_bucketer.finish()
        opt.step()
        norms.append(opt.last_grad_norm())
    torch.save({"final": m._mpa_arena.master.clone(), "norms": norms, "lr": opt.current_lr(),
                "coef": float(opt.hyper[3])}, os.path.join(out_dir, "r%d.pt" % rank))
    shutdown()


def test_recipe_two_ranks_gloo():
    """With the recipe on, every rank computes the same norm from the all-reduced arena, so
    the replicas stay bitwise identical."""
    with tempfile.TemporaryDirectory() as d:
        mp.start_processes(_worker, args=(2, _free_port(), d), nprocs=2, join=True,
                           start_method="spawn")
        r0, r1 = (torch.load(os.path.join(d, "r%d.pt" % r)) for r in range(2))
    assert torch.equal(r0["final"], r1["final"])
    assert r0["norms"] == r1["norms"] and r0["lr"] == r1["lr"]
    assert r0["coef"] < 1.0  # the clip was active
    assert abs(r0["lr"] - lr_f64(1e-3, 2, W=2, T=6, r=0.1)) <= 1e-6 * 1e-3
