"""Weight EMA without a GPU: the oracle alone meets every check ``test_ema_gpu.py`` applies
to the kernels, ``ModelEMA`` on the CPU path against ``torch.optim.swa_utils.AveragedModel``,
config, checkpoint keys, resume from a checkpoint without an average, the driver's log and
metrics, and ``eval_ema`` in the evaluation pipeline's ``load_predictor``."""
import json
import logging
import os
import shutil

import pytest
import torch

import test_ema_gpu as eg
from mpi_pytorch_amd.checkpoint import (build_state, load_checkpoint, read_checkpoint,
                                        save_checkpoint)
from mpi_pytorch_amd.config import Config
from mpi_pytorch_amd.engine import build_training
from mpi_pytorch_amd.ops import ref
from mpi_pytorch_amd.parallel import World

CPU = torch.device("cpu")


def _reset_world():
    import mpi_pytorch_amd.parallel.dist as D
    D._WORLD = None


# --------------------------------------------------- the oracle meets the kernels' checks
@pytest.mark.parametrize("warmup", [True, False])
@pytest.mark.parametrize("t", [1, 9, 10000])
def test_oracle_meets_ema_update_checks(t, warmup):
    for n in eg.SIZES[:2]:
        eg.check_ema_update(ref, CPU, n, t, warmup)


def test_oracle_meets_the_small_checks():
    eg.check_ema_update(ref, CPU, eg.SIZES[2], 9, True)
    eg.check_fixed_point(ref, CPU)
    eg.check_weight_readback(ref, CPU)
    eg.check_closed_form(ref, CPU)
    eg.check_ema_multi(ref, CPU)


def test_oracle_rejects_a_bad_decay_or_table():
    e, p, t = torch.zeros(64), torch.ones(64), torch.zeros(1)
    for d in (1.0, -0.1):
        with pytest.raises(ValueError):
            ref.ema_update(e, p, t, d, True)
    th = torch.tensor([[0, 0, 65]], dtype=torch.int64)
    with pytest.raises(ValueError):
        ref.ema_update_multi(e, th, th, [torch.ones(65)], t, 0.5, True)  # outside ema_buf


# ------------------------------------------------------------------------------- config
def test_config_validation_and_default_off():
    c = Config()
    assert (c.ema_decay, c.ema_warmup, c.eval_ema) == (0.0, True, False)
    for bad in (1.0, -0.01, 1.5):
        with pytest.raises(ValueError, match="ema_decay"):
            Config(ema_decay=bad)
    assert Config(ema_decay=0.9998).ema_decay == 0.9998
    c = Config.from_args(["--ema_decay", "0.99", "--ema_warmup", "false", "--eval_ema", "true"])
    assert (c.ema_decay, c.ema_warmup, c.eval_ema) == (0.99, False, True)
    model, opt, step, _ = build_training("resnet18", 10, CPU, World(), 1e-3)
    assert step.ema is None
    assert set(build_state(0, model, opt, 0.0)) == {"epoch", "state_dict", "optimizer", "loss"}
    with pytest.raises(ValueError, match="ema_decay"):
        build_training("resnet18", 10, CPU, World(), 1e-3, ema_decay=1.0)


# ----------------------------------------------------------------- against AveragedModel
def test_model_ema_matches_averaged_model():
    """20 updates, no warm-up, N(0, 4) weights and float buffers redrawn before each one:
    per element |ModelEMA - AveragedModel| <= 2 k 2^-23 max(|p|, |ema|), the maximum taken
    over the k updates' weights and averages: update j rounds three times (torch's lerp may
    fuse one), each time by at most 2^-24 of an intermediate no larger than
    2 max(|p_j|, |ema_j|), and later updates only shrink that error (by d each).  With only
    the last update's |p| and |ema| as the scale the bound is not a bound: where both
    happen to be near 0 the error of the earlier, larger values remains, and the unfused
    oracle itself is 4.2 times over it at the worst element of this data."""
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    from mpi_pytorch_amd.ema import ModelEMA
    from mpi_pytorch_amd.optim import FusedAdam
    from mpi_pytorch_amd.parallel.arena import ParamArena
    d, k = 0.9, 20

    def make():
        torch.manual_seed(3)
        return torch.nn.Sequential(torch.nn.Linear(40, 70), torch.nn.BatchNorm1d(70),
                                   torch.nn.Linear(70, 9))

    twin, model = make(), make()
    arena = ParamArena(model, CPU)
    model._mpa_arena = arena
    opt = FusedAdam(list(model.parameters()), arena)
    ema = ModelEMA(model, opt, d, warmup=False)
    avg = AveragedModel(twin, multi_avg_fn=get_ema_multi_avg_fn(d), use_buffers=True)
    avg.update_parameters(twin)  # (the first call copies: both start from the weights)
    assert len(ema.buffers) == 2  # running_mean, running_var; not num_batches_tracked
    g = torch.Generator().manual_seed(4)
    scale = {name: torch.zeros_like(v, dtype=torch.float64)
             for name, v in twin.state_dict().items() if v.is_floating_point()}
    with torch.no_grad():
        for _ in range(k):
            for a, b in zip(list(twin.parameters()) + list(twin.buffers()),
                            list(model.parameters()) + list(model.buffers())):
                if a.is_floating_point():
                    a.copy_(torch.randn(a.shape, generator=g) * 2.0)
                    b.copy_(a)
            opt.step_t += 1.0
            ema.update()
            avg.update_parameters(twin)
            for src in (twin.state_dict(), avg.module.state_dict()):
                for name in scale:
                    scale[name] = torch.maximum(scale[name], src[name].double().abs())
    sd = ema.state_dict()
    want = avg.module.state_dict()
    live = twin.state_dict()
    assert set(sd) == set(want)
    worst = 0.0
    for name, w in want.items():
        if not w.is_floating_point():
            continue
        got = sd[name].double()
        bound = 2 * k * 2.0 ** -23 * scale[name]
        err = (got - w.double()).abs()
        worst = max(worst, float((err / bound).max()))
        assert bool((err <= bound).all()), (name, worst)
        assert not torch.equal(sd[name], live[name])
    print("worst |err| / bound: %.3f" % worst)


# ---------------------------------------------------- state dict: torchvision's names
def test_ema_state_dict_has_the_models_names_and_shapes():
    """torchvision is loaded with strict=True where it is installed; without it the names
    and shapes are compared against ``model.state_dict()`` (torchvision's, by the model
    zoo's own tests)."""
    model, opt, step, _ = build_training("resnet18", 10, CPU, World(), 1e-3, ema_decay=0.9)
    step(torch.randn(4, 32, 32, 3), torch.randint(0, 10, (4,)))
    sd = step.ema.state_dict()
    try:
        import torchvision
    except ImportError:
        torchvision = None
    if torchvision is not None:
        torchvision.models.resnet18(num_classes=10).load_state_dict(sd, strict=True)
    live = model.state_dict()
    assert list(sd) == list(live)
    assert all(sd[k].shape == live[k].shape and sd[k].dtype == live[k].dtype for k in sd)
    assert tuple(sd["conv1.weight"].shape) == (64, 3, 7, 7)
    assert not torch.equal(sd["fc.weight"], live["fc.weight"])
    # the reverse: the average becomes the dict's weights, the live model stays
    before = model._mpa_arena.master.clone()
    batches = [m._batches_host for m in model.modules() if hasattr(m, "_batches_host")]
    want = (step.ema.ema.clone(), step.ema.ema_buf.clone())
    step.ema.reset()
    assert not torch.equal(step.ema.ema, want[0])
    step.ema.load_state_dict(sd)
    assert torch.equal(step.ema.ema, want[0]) and torch.equal(step.ema.ema_buf, want[1])
    assert torch.equal(model._mpa_arena.master, before)
    assert batches == [m._batches_host for m in model.modules() if hasattr(m, "_batches_host")]


# ------------------------------------------------------------- resume: an old checkpoint
class _Lines(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def test_checkpoint_without_an_average_starts_from_the_loaded_weights(tmp_path):
    from mpi_pytorch_amd.utils.logging import get_logger
    x, y = torch.randn(4, 32, 32, 3), torch.randint(0, 10, (4,))
    model, opt, step, _ = build_training("resnet18", 10, CPU, World(), 1e-3)
    step(x, y)
    path = save_checkpoint(build_state(0, model, opt, 0.0), 0, "resnet18", str(tmp_path))
    model2, opt2, step2, _ = build_training("resnet18", 10, CPU, World(), 1e-3, ema_decay=0.9)
    step2(x, y)
    n = model2._mpa_arena.n_train
    h = _Lines()
    log = get_logger()
    log.addHandler(h)
    old = log.level
    log.setLevel(logging.INFO)
    try:
        load_checkpoint(path, model2, opt2, ema=step2.ema)
    finally:
        log.removeHandler(h)
        log.setLevel(old)
    assert len([ln for ln in h.lines if "no ema_state_dict" in ln]) == 1
    assert torch.equal(step2.ema.ema[:n], model._mpa_arena.master[:n])
    for (slot, b), live in zip(step2.ema._slots(), [b for b in model.buffers()
                                                     if b.is_floating_point()]):
        assert torch.equal(slot, live.reshape(-1))
    # and one with an average restores it
    path = save_checkpoint(build_state(0, model2, opt2, 0.0, step2.ema), 0, "resnet18",
                           str(tmp_path))
    step2(x, y)
    want = read_checkpoint(path)["ema_state_dict"]
    model3, opt3, step3, _ = build_training("resnet18", 10, CPU, World(), 1e-3, ema_decay=0.9)
    h.lines.clear()
    log.addHandler(h)
    try:
        load_checkpoint(path, model3, opt3, ema=step3.ema)
    finally:
        log.removeHandler(h)
    assert not h.lines
    got = step3.ema.state_dict()
    assert all(torch.equal(got[k], want[k]) for k in want)


# --------------------------------------------- the driver: log, metrics, checkpoint, eval
@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """A default run (one epoch), then a resumed run with the EMA on from its checkpoint."""
    from mpi_pytorch_amd.engine.trainer import run_training
    d = tmp_path_factory.mktemp("ema_runs")
    common = dict(synthetic_images=16, image_size=32, BATCH_SIZE=8, NUM_CLASSES=10,
                  CHECKPOINT_DIR=str(d) + "/ck/", device="cpu")
    _reset_world()
    run_training(Config(NUM_EPOCHS=1, log_file=str(d / "a.log"),
                        metrics_jsonl=str(d / "a.jsonl"), **common))
    ck = os.path.join(str(d), "ck", "checkpoint_resnet18.pt")
    old = str(d / "old.pt")
    shutil.copy(ck, old)
    _reset_world()
    out = run_training(Config(NUM_EPOCHS=2, FROM_CHECKPOINT=True, ema_decay=0.9, eval_topk=3,
                              log_file=str(d / "b.log"), metrics_jsonl=str(d / "b.jsonl"),
                              **common))
    _reset_world()
    return dict(dir=d, old=old, new=ck, out=out, common=common)


def test_default_run_is_unchanged(runs):
    assert set(read_checkpoint(runs["old"])) == {"epoch", "state_dict", "optimizer", "loss"}
    text = (runs["dir"] / "a.log").read_text()
    assert "EMA" not in text and "ema" not in text
    rec = json.loads((runs["dir"] / "a.jsonl").read_text().splitlines()[-1])
    assert "acc" in rec and not [k for k in rec if "ema" in k]


def test_run_with_ema_logs_validates_and_checkpoints(runs):
    lines = (runs["dir"] / "b.log").read_text().splitlines()
    assert len([ln for ln in lines if "no ema_state_dict" in ln]) == 1
    tail = [ln.split(":", 2)[2] for ln in lines if "_Epoch: 1 |" in ln]
    assert [ln.split("|")[1].strip().split(":")[0] for ln in tail] == \
        ["Train Loss", "Acc", "Top-3 Acc", "EMA Acc", "EMA Top-3 Acc"]
    rec = runs["out"]["history"][-1]
    assert rec["epoch"] == 1
    for key in ("acc", "acc_top3", "acc_ema", "acc_ema_top3"):
        assert 0.0 <= rec[key] <= 1.0
    assert tail[3] == "_Epoch: 1 | EMA Acc: {}".format(rec["acc_ema"])
    saved = json.loads((runs["dir"] / "b.jsonl").read_text().splitlines()[-1])
    assert saved["acc_ema"] == rec["acc_ema"] and saved["acc_ema_top3"] == rec["acc_ema_top3"]
    ck = read_checkpoint(runs["new"])  # (weights_only=True: plain Python types)
    assert set(ck) == {"epoch", "state_dict", "optimizer", "loss", "ema_state_dict", "ema"}
    assert ck["ema"] == {"decay": 0.9, "warmup": True}
    assert list(ck["ema_state_dict"]) == list(ck["state_dict"])
    assert not torch.equal(ck["ema_state_dict"]["fc.weight"], ck["state_dict"]["fc.weight"])


def test_load_predictor_eval_ema(runs):
    from mpi_pytorch_amd.engine.eval_pipeline import load_predictor
    ck = read_checkpoint(runs["new"])
    cfg = Config(NUM_CLASSES=10, device="cpu")
    live = load_predictor(cfg, CPU, runs["new"]).state_dict()
    cfg_ema = Config(NUM_CLASSES=10, device="cpu", eval_ema=True)
    avg = load_predictor(cfg_ema, CPU, runs["new"]).state_dict()
    for k in ("conv1.weight", "fc.weight", "bn1.running_mean"):
        assert torch.equal(live[k], ck["state_dict"][k])
        assert torch.equal(avg[k], ck["ema_state_dict"][k])
    with pytest.raises(KeyError, match="has no ema_state_dict"):
        load_predictor(cfg_ema, CPU, runs["old"])
    with pytest.raises(FileNotFoundError, match="eval_ema"):
        load_predictor(cfg_ema, CPU, str(runs["dir"] / "missing.pt"))
