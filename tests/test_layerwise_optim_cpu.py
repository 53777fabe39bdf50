"""Layer-wise optimizers (AdamW, LAMB, LARS) on the CPU path: the config fields, the segment
and chunk plan over the arena, the ``ops/ref.py`` twins behind ``FusedAdamW`` / ``FusedLAMB``
/ ``FusedLARS`` against ``torch.optim.AdamW`` and float64 per-parameter loops written here,
the checkpoint format, and the training driver.

The reference trains with ``torch.optim.Adam`` only (``main.py:125`` there): these
optimizers are an addition, and ``adam`` / ``sgd`` keep their kernels and semantics."""
import json
import math

import pytest
import torch
import torch.nn as nn

from mpi_pytorch_amd.config import Config
from mpi_pytorch_amd.ops import ref
from mpi_pytorch_amd.optim import (FusedAdam, FusedAdamW, FusedLAMB, FusedLARS,
                                   build_optimizer, build_segment_plan)
from mpi_pytorch_amd.parallel.arena import ALIGN, ParamArena, _align

LR, WD, GS, COEF = 1e-2, 0.05, 0.5, 0.02
B1, B2, EPS, MOM = 0.9, 0.999, 1e-8, 0.9


# ------------------------------------------------------------------------------ config
def test_config_fields(monkeypatch):
    c = Config()
    assert (c.optimizer, c.trust_coef, c.wd_exclude_1d) == ("adam", 0.001, True)
    for name in ("adam", "sgd", "adamw", "lamb", "lars"):
        assert Config(optimizer=name).optimizer == name
    for bad in ("lamb2", "AdamW", "", "rmsprop"):
        with pytest.raises(ValueError, match="adam\\|sgd\\|adamw\\|lamb\\|lars"):
            Config(optimizer=bad)
    with pytest.raises(ValueError):
        Config(trust_coef=0.0)
    c = Config.from_args(["--optimizer", "lars", "--trust-coef", "0.02", "--wd_exclude_1d", "0"])
    assert (c.optimizer, c.trust_coef, c.wd_exclude_1d) == ("lars", 0.02, False)
    monkeypatch.setenv("MPA_OPTIMIZER", "lamb")
    monkeypatch.setenv("MPA_TRUST_COEF", "0.5")
    monkeypatch.setenv("MPA_wd_exclude_1d", "false")
    c = Config.from_env()
    assert (c.optimizer, c.trust_coef, c.wd_exclude_1d) == ("lamb", 0.5, False)


# -------------------------------------------------------------------------------- plan
@pytest.mark.parametrize("name", ["resnet18", "inception"])
def test_plan_properties(name):
    from mpi_pytorch_amd.engine import build_training
    from mpi_pytorch_amd.parallel import World
    model, opt, _s, _ = build_training(name, 10, torch.device("cpu"), World(), 1e-3, "lamb")
    a = model._mpa_arena
    CH = ref.seg_chunk()
    assert opt.plan_seg.dtype == torch.int64 and opt.plan_chunk_seg.dtype == torch.int32
    seg, chunk_seg = opt.plan_seg.tolist(), opt.plan_chunk_seg.tolist()
    assert len(seg) == len(a.trainable)  # grouped parameters stay one segment each
    if name == "inception":
        assert callable(getattr(model, "_mpa_param_groups", None))
    off = nchunks = 0
    for s, (p, (o, ln, first, nch, flags)) in enumerate(zip(a.trainable, seg)):
        assert o == off == a.offsets[id(p)] and o % ALIGN == 0 and ln == _align(p.numel())
        assert first == nchunks and nch == -(-ln // CH) and nch >= 1
        assert chunk_seg[first:first + nch] == [s] * nch  # consecutive, never another segment
        one_d = p.ndim <= 1
        assert flags == (0 if one_d else ref.SEG_DECAY | ref.SEG_ADAPT), (a.names[id(p)], flags)
        off += ln
        nchunks += nch
    assert off == a.n_train and nchunks == len(chunk_seg)
    assert any(f == 0 for *_x, f in seg) and any(f != 0 for *_x, f in seg)
    # every flag on without the exclusion; a smaller chunk only cuts finer
    seg_all, _ = build_segment_plan(a, wd_exclude_1d=False)
    assert all(f == ref.SEG_DECAY | ref.SEG_ADAPT for f in seg_all[:, ref.SEG_FLAGS].tolist())
    seg64, cs64 = build_segment_plan(a, chunk=ALIGN)
    assert cs64.numel() == a.n_train // ALIGN
    assert int(seg64[:, ref.SEG_NCHUNK].sum()) == cs64.numel()


# ------------------------------------------------------- the oracle vs independent code
def _tiny(seed=0):
    torch.manual_seed(seed)
    # (sizes that are no multiple of the arena's 64-element slots: padding in between)
    return nn.Sequential(nn.Linear(7, 33), nn.Tanh(), nn.Linear(33, 5))


def _grads(model, steps, seed=3, mul=1.0):
    g = torch.Generator().manual_seed(seed)
    return [[torch.randn(p.shape, generator=g) * mul for p in model.parameters()]
            for _ in range(steps)]


def _make(kind, model, exclude=True, wd=WD):
    arena = ParamArena(model, torch.device("cpu"))
    params = list(model.parameters())
    if kind == "adam":
        opt = FusedAdam(params, arena, lr=LR, weight_decay=wd)
    elif kind == "adamw":
        opt = FusedAdamW(params, arena, lr=LR, weight_decay=wd, wd_exclude_1d=exclude)
    elif kind == "lamb":
        opt = FusedLAMB(params, arena, lr=LR, weight_decay=wd, wd_exclude_1d=exclude)
    else:
        opt = FusedLARS(params, arena, lr=LR, momentum=MOM, weight_decay=wd, trust_coef=COEF,
                        wd_exclude_1d=exclude)
    opt.grad_scale = GS
    return arena, opt


def _run_engine(kind, steps=5, exclude=True, mul=1.0, model=None, opt_arena=None, start=0):
    model = _tiny() if model is None else model
    arena, opt = _make(kind, model, exclude) if opt_arena is None else opt_arena
    for gs in _grads(model, steps, mul=mul)[start:]:
        arena.zero_grad()
        for p, g in zip(model.parameters(), gs):
            p.grad.copy_(g)
        opt.step()
    return model, arena, opt


def _max_diff(model, params):
    return max(float((p.detach().double() - q.detach().double()).abs().max())
               for p, q in zip(model.parameters(), params))


def _run_torch(cls, groups, steps=5):
    model = _tiny()
    params = list(model.parameters())
    opt = cls(groups(params), lr=LR)
    for gs in _grads(model, steps):
        for p, g in zip(params, gs):
            p.grad = g.clone() * GS
        opt.step()
    return params


@pytest.mark.parametrize("exclude", [False, True])
def test_adamw_matches_torch(exclude):
    """Five steps against torch.optim.AdamW on the same gradients: one group with
    ``wd_exclude_1d=False``, two groups (decay / no decay on 1-D) with True.  Allowed: 4x
    the difference the existing FusedAdam shows against torch.optim.Adam in the same
    setting, floor 1e-7 (test_recipe_cpu.py's bound for Adam)."""
    base = _max_diff(_run_engine("adam")[0], _run_torch(
        torch.optim.Adam, lambda ps: [dict(params=ps, weight_decay=WD)]))

    def groups(ps):
        if not exclude:
            return [dict(params=ps, weight_decay=WD)]
        return [dict(params=[p for p in ps if p.ndim > 1], weight_decay=WD),
                dict(params=[p for p in ps if p.ndim <= 1], weight_decay=0.0)]
    model, _a, opt = _run_engine("adamw", exclude=exclude)
    diff = _max_diff(model, _run_torch(torch.optim.AdamW, groups))
    print("adamw exclude=%s: FusedAdam vs torch.Adam %.3e, FusedAdamW vs torch.AdamW %.3e"
          % (exclude, base, diff))
    assert diff <= max(4 * base, 1e-7), (diff, base)
    assert set(opt.last_trust_ratios().values()) == {1.0}
    # and the decay is really decoupled: coupled Adam with the same numbers differs
    assert _max_diff(model, list(_run_engine("adam")[0].parameters())) > 1e-5


def _textbook(kind, steps=5, exclude=True, mul=1.0):
    """LAMB / LARS per parameter in float64, straight from the papers' formulas."""
    model = _tiny()
    ps = [p.detach().double().clone() for p in model.parameters()]
    st = [dict(m=torch.zeros_like(p), v=torch.zeros_like(p), buf=None) for p in ps]
    ratios = []
    for t, gs in enumerate(_grads(model, steps, mul=mul), 1):
        ratios = []
        for p, s, g in zip(ps, st, gs):
            g = g.double() * GS
            on = not (exclude and p.ndim <= 1)
            wd = WD if on else 0.0
            if kind == "lamb":
                s["m"] = B1 * s["m"] + (1 - B1) * g
                s["v"] = B2 * s["v"] + (1 - B2) * g * g
                u = (s["m"] / (1 - B1 ** t)) / ((s["v"] / (1 - B2 ** t)).sqrt() + EPS) + wd * p
                pn, un = float(p.norm()), float(u.norm())
                r = pn / un if on and pn > 0 and un > 0 else 1.0
                p -= LR * r * u
            else:
                pn, gn = float(p.norm()), float(g.norm())
                r = COEF * pn / (gn + wd * pn + 1e-8) if on and pn > 0 and gn > 0 else 1.0
                g = r * (g + wd * p)
                s["buf"] = g.clone() if s["buf"] is None else MOM * s["buf"] + g
                p -= LR * s["buf"]
            ratios.append(r)
    return ps, ratios


@pytest.mark.parametrize("kind", ["lamb", "lars"])
@pytest.mark.parametrize("exclude", [True, False])
def test_lamb_lars_match_float64_loop(kind, exclude):
    """Five steps of the fp32 CPU path against the float64 loop above.  Bound: parameters
    are O(1), every step adds a few fp32 roundings (2^-24 = 6e-8 each, relative) to each
    element and to the ratio; 5 steps x ~8 roundings x 6e-8 = 2.4e-6 absolute at |p| <= 1."""
    model, arena, opt = _run_engine(kind, exclude=exclude)
    want, ratios = _textbook(kind, exclude=exclude)
    diff = _max_diff(model, want)
    print("%s exclude=%s: fp32 path vs float64 loop %.3e" % (kind, exclude, diff))
    assert diff <= 2.4e-6, diff
    got = opt.last_trust_ratios()
    names = [arena.names[id(p)] for p in model.parameters()]
    for n, r in zip(names, ratios):
        assert abs(got[n] - r) <= 1e-5 * r, (n, got[n], r)
    if exclude:
        assert got["0.bias"] == 1.0 and got["2.bias"] == 1.0 and got["0.weight"] != 1.0
    # arena padding is zero in weights and state and stays zero
    pad = torch.ones(arena.n_train, dtype=torch.bool)
    for p in arena.trainable:
        o, e = arena.slice_of(p)
        pad[o:e] = False
    assert pad.any() and not arena.master[:arena.n_train][pad].any()


def test_lamb_first_step_is_gradient_scale_invariant():
    """The trust ratio normalises the update: with all gradients x10 LAMB's first step moves
    every parameter the same way (Adam's first direction is g / (|g| + eps), itself scale
    free up to eps = 1e-8 against |g| ~ 1: a 1e-8 relative change of a 1e-2 step)."""
    a = _run_engine("lamb", steps=1)[0]
    b = _run_engine("lamb", steps=1, mul=10.0)[0]
    start = _tiny()
    moved = _max_diff(a, list(start.parameters()))
    diff = _max_diff(a, list(b.parameters()))
    print("lamb first step: moved %.3e, x10 gradients change it by %.3e" % (moved, diff))
    assert moved > 1e-3 and diff <= 4e-7  # a few fp32 roundings of O(1) parameters


# ------------------------------------------------------------------------------- state
@pytest.mark.parametrize("kind", ["adamw", "lamb", "lars"])
def test_state_dict_round_trip(kind, tmp_path):
    model, arena, opt = _run_engine(kind, steps=2)
    opt.trust_coef = 0.25
    sd = opt.state_dict()
    g = sd["param_groups"][0]
    assert g["mpa_trust_coef"] == 0.25 and g["mpa_wd_exclude_1d"] is True
    assert g["mpa_step"] == 2.0 and g["weight_decay"] == WD
    path = str(tmp_path / "opt.pt")
    torch.save({"optimizer": sd}, path)
    sd = torch.load(path, weights_only=True)["optimizer"]  # plain Python values only
    params = [nn.Parameter(p.detach().clone()) for p in model.parameters()]
    if kind == "lars":
        assert set(sd["state"][0]) == {"momentum_buffer"}
        torch.optim.SGD(params, lr=LR, momentum=MOM).load_state_dict(sd)
    else:
        assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
        assert g["decoupled_weight_decay"] is True
        t = torch.optim.AdamW(params, lr=LR)
        t.load_state_dict(sd)
        assert t.param_groups[0]["weight_decay"] == WD
    # a fresh optimizer (other settings) takes over the saved ones and continues bitwise
    model2 = _tiny()
    arena2, opt2 = _make(kind, model2, exclude=False)
    opt2.load_state_dict(sd)
    assert opt2.trust_coef == 0.25 and opt2.wd_exclude_1d is True
    assert torch.equal(opt2.plan_seg, opt.plan_seg) and float(opt2.step_t) == 2.0
    arena2.master.copy_(arena.master)
    _run_engine(kind, steps=3, model=model2, opt_arena=(arena2, opt2), start=2)
    full_model, full_arena, full_opt = _run_engine(kind, steps=2)
    full_opt.trust_coef = 0.25
    _run_engine(kind, steps=3, model=full_model, opt_arena=(full_arena, full_opt), start=2)
    assert torch.equal(arena2.master, full_arena.master)


def test_build_optimizer_names():
    model = _tiny()
    model._mpa_arena = ParamArena(model, torch.device("cpu"))
    for name, cls in (("adamw", FusedAdamW), ("lamb", FusedLAMB), ("lars", FusedLARS)):
        opt = build_optimizer(name, model, 1e-3, 0.9, 0.01, 0.5, False)
        assert type(opt) is cls and opt.kind == name
        assert opt.trust_coef == 0.5 and opt.wd_exclude_1d is False
    with pytest.raises(ValueError):
        build_optimizer("rmsprop", model, 1e-3)


def _reset_world():
    import mpi_pytorch_amd.parallel.dist as D
    D._WORLD = None


def test_training_driver_lamb(tmp_path):
    """One debug epoch with ``--optimizer lamb``, then a resumed second one: the log keeps
    its lines, the metrics record gains the trust-ratio summary, and a default run's record
    does not."""
    from mpi_pytorch_amd.engine.trainer import run_training
    kw = dict(synthetic_images=32, image_size=32, BATCH_SIZE=16, NUM_CLASSES=10, VALIDATE=False,
              device="cpu", watchdog_s=0, CHECKPOINT_DIR=str(tmp_path) + "/c/",
              MODELS_DIR=str(tmp_path) + "/m/", log_file=str(tmp_path / "a.log"),
              metrics_jsonl=str(tmp_path / "a.jsonl"))
    lamb = Config.from_args(["--optimizer", "lamb", "--weight-decay", "0.01"], NUM_EPOCHS=1, **kw)
    assert lamb.optimizer == "lamb"
    _reset_world()
    run_training(lamb)
    _reset_world()
    run_training(Config(optimizer="lamb", weight_decay=0.01, NUM_EPOCHS=2, FROM_CHECKPOINT=True,
                        **kw))
    recs = [json.loads(l) for l in (tmp_path / "a.jsonl").read_text().splitlines()]
    assert [r["epoch"] for r in recs] == [0, 1]
    for r in recs:
        t = r["trust_ratio"]
        assert 0 < t["min"] <= t["median"] <= t["max"] and math.isfinite(t["max"])
        assert t["min"] != t["max"] and math.isfinite(r["train_loss"])
    text = (tmp_path / "a.log").read_text()
    for line in ("_Optimizer Created", "_Loading Checkpoint", "_Checkpoint loaded",
                 "_Entering training Loop", "_Epoch: 0 | Train Loss: ", "_Epoch: 1 | Train Loss: ",
                 "_Checkpoint saved"):
        assert line in text, line
    _reset_world()
    kw.update(metrics_jsonl=str(tmp_path / "b.jsonl"), log_file=str(tmp_path / "b.log"),
              CHECKPOINT_DIR=str(tmp_path) + "/d/")
    run_training(Config(NUM_EPOCHS=1, **kw))
    for line in (tmp_path / "b.jsonl").read_text().splitlines():
        assert "trust_ratio" not in json.loads(line)
    _reset_world()
