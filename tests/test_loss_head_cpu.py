"""The loss head on the CPU: the checks of ``test_loss_head_gpu.py`` run with the oracle as
the implementation (every bound there is met by ``ops/ref.py`` alone), the oracle itself
against ``F.cross_entropy(label_smoothing=...)`` and ``torch.topk``, and the plumbing from
``Config`` through the training driver and the evaluation pipeline."""
import json
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_loss_head_gpu as lh
from mpi_pytorch_amd.config import Config
from mpi_pytorch_amd.ops import ref

CPU = torch.device("cpu")


def _reset_world():
    import mpi_pytorch_amd.parallel.dist as D
    D._WORLD = None


# ------------------------------------------------- the GPU file's checks, on the oracle
@pytest.mark.parametrize("shape", lh.SHAPES)
def test_oracle_meets_smoothed_ce_checks(shape):
    for eps in lh.EPS:
        lh.check_smoothed_random(ref, CPU, *shape, eps)
        lh.check_smoothed_flat(ref, CPU, *shape, eps)
    lh.check_smoothed_bitwise(ref, CPU, *shape)


def test_oracle_meets_weighted_and_autograd_checks():
    for shape in ((300, 33, 64), (7, 1000, 1024), (7, 1004, 1004)):
        lh.check_smoothed_weighted(ref, CPU, *shape)
    lh.check_autograd(CPU)


@pytest.mark.parametrize("shape", lh.SHAPES)
def test_oracle_meets_topk_checks(shape):
    lh.check_topk_vs_ref(ref, CPU, *shape)
    lh.check_topk_vs_argmax(ref, CPU, *shape)
    lh.check_topk_tie_free(ref, CPU, *shape)


def test_oracle_meets_topk_rule_checks():
    lh.check_topk_tie_rule(ref, CPU)
    lh.check_topk_nan_and_accumulate(ref, CPU)
    with pytest.raises(ValueError):
        ref.topk_correct(torch.zeros(2, 8), torch.zeros(2, dtype=torch.int64), 0,
                         torch.zeros(1, dtype=torch.int64))


def test_flat_check_sees_a_dropped_term():
    """The closed forms fail an implementation without the logit-sum term, and one without
    the eps/NC term of the gradient (the max-norm gradient bound alone sees neither at
    64,500 classes)."""
    class NoSum:
        ce_bwd = staticmethod(ref.ce_bwd)

        @staticmethod
        def ce_fwd(logits, labels, smoothing=0.0):
            lf = logits.float()
            lse = torch.logsumexp(lf, 1)
            picked = lf.gather(1, labels.view(-1, 1)).squeeze(1)
            return (lse - (1 - smoothing) * picked).mean().reshape(1), lse

    class NoUniform:
        ce_fwd = staticmethod(ref.ce_fwd)

        @staticmethod
        def ce_bwd(logits, labels, lse, go, weight=1.0, smoothing=0.0):
            B = logits.shape[0]
            p = torch.exp(logits.float() - lse[:, None])
            p[torch.arange(B), labels] -= 1.0 - smoothing
            return (p * (go.reshape(()) * weight / B)).to(logits.dtype)

    for shape in ((5, 33, 64), (4, 64500, 64512)):
        for impl in (NoSum, NoUniform):
            with pytest.raises(AssertionError):
                lh.check_smoothed_flat(impl, CPU, *shape, 0.1)


# --------------------------------------------------------------- the oracle vs torch
@pytest.mark.parametrize("NC", [33, 1000, 64500])
@pytest.mark.parametrize("eps", [0.0, 0.1, 1.0])
def test_oracle_matches_torch_cross_entropy(NC, eps):
    torch.manual_seed(80)
    B = 6
    logits = (torch.randn(B, NC) * 3 + 2).to(torch.bfloat16)
    labels = torch.randint(0, NC, (B,))
    x = logits.float().requires_grad_(True)
    want = F.cross_entropy(x, labels, label_smoothing=eps)
    want.backward()
    loss, lse = ref.ce_fwd(logits, labels, eps)
    want = float(want.detach())
    assert abs(float(loss) - want) <= 1e-5 * abs(want)
    d = ref.ce_bwd(logits.float(), labels, lse, torch.ones(1), 1.0, eps)
    assert lh.rel(d, x.grad) < 1e-4


@pytest.mark.parametrize("NC", [33, 1000])
def test_oracle_topk_matches_torch_topk(NC):
    torch.manual_seed(81)
    vals = lh.distinct_rows(16, NC, CPU)
    labels = torch.randint(0, NC, (16,))
    for k in (1, 5, NC):
        cnt = torch.zeros(1, dtype=torch.int64)
        ref.topk_correct(vals, labels, k, cnt)
        assert int(cnt) == int((vals.float().topk(k, 1).indices == labels[:, None]).any(1).sum())


# ------------------------------------------------------------------------- plumbing
def test_config_validates_and_overrides(monkeypatch):
    c = Config()
    assert c.label_smoothing == 0.0 and c.eval_topk == 0
    for bad in (-0.01, 1.01):
        with pytest.raises(ValueError):
            Config(label_smoothing=bad)
    with pytest.raises(ValueError):
        Config(eval_topk=-1)
    assert Config(label_smoothing=1.0, eval_topk=1).eval_topk == 1
    c = Config.from_args(["--label_smoothing", "0.1", "--eval-topk", "5"])
    assert c.label_smoothing == 0.1 and c.eval_topk == 5
    monkeypatch.setenv("MPA_LABEL_SMOOTHING", "0.2")
    monkeypatch.setenv("MPA_EVAL_TOPK", "3")
    c = Config.from_args([])
    assert c.label_smoothing == 0.2 and c.eval_topk == 3


def test_step_loss_is_torch_smoothed_cross_entropy():
    from mpi_pytorch_amd.engine import build_training
    from mpi_pytorch_amd.parallel import World
    torch.manual_seed(0)
    model, opt, step, _ = build_training("resnet18", 50, CPU, World(), 1e-3,
                                         label_smoothing=0.1)
    assert step.label_smoothing == 0.1
    seen = []
    model.register_forward_hook(lambda m, i, o: seen.append(o.detach().clone()))
    x, y = torch.randn(6, 32, 32, 3), torch.randint(0, 50, (6,))
    loss = float(step(x, y))
    want = float(F.cross_entropy(seen[0].float(), y, label_smoothing=0.1))
    plain = float(F.cross_entropy(seen[0].float(), y))
    assert abs(loss - want) <= 1e-5 * abs(want) and abs(want - plain) > 1e-4


def _shape_of(line):
    return re.sub(r"[-+]?\d+(\.\d+)?(e[-+]?\d+)?", "#", line)


def test_training_driver_logs_topk_and_keeps_every_other_line(tmp_path):
    from mpi_pytorch_amd.engine.trainer import run_training
    texts = {}
    for name, extra in (("plain", {}), ("head", dict(label_smoothing=0.1, eval_topk=5))):
        _reset_world()
        d = tmp_path / name
        d.mkdir()
        cfg = Config(synthetic_images=32, image_size=32, NUM_EPOCHS=1, BATCH_SIZE=16,
                     NUM_CLASSES=50, CHECKPOINT_DIR=str(d) + "/ck/", device="cpu",
                     log_file=str(d / "training.log"), metrics_jsonl=str(d / "m.jsonl"), **extra)
        run_training(cfg)
        texts[name] = (d / "training.log").read_text().splitlines()
    rec = json.loads((tmp_path / "head" / "m.jsonl").read_text().splitlines()[0])
    plain_rec = json.loads((tmp_path / "plain" / "m.jsonl").read_text().splitlines()[0])
    assert "acc_top5" in rec and "acc_top5" not in plain_rec
    assert 0.0 <= rec["acc"] <= rec["acc_top5"] <= 1.0
    lines = texts["head"]
    at = [i for i, s in enumerate(lines) if "_Epoch: 0 | Top-5 Acc: " in s]
    assert len(at) == 1 and "_Epoch: 0 | Acc: " in lines[at[0] - 1]
    assert float(lines[at[0]].rsplit(" ", 1)[1]) == rec["acc_top5"]
    assert not any("Top-" in s for s in texts["plain"])
    rest = lines[:at[0]] + lines[at[0] + 1:]
    assert [_shape_of(s) for s in rest] == [_shape_of(s) for s in texts["plain"]]


def test_eval_pipeline_counts_topk(tmp_path):
    from mpi_pytorch_amd.engine import build_training
    from mpi_pytorch_amd.engine.eval_pipeline import StreamPipeline, _batches, run_pipeline
    from mpi_pytorch_amd.data.manifest import SyntheticImages
    from mpi_pytorch_amd.models import input_spec
    from mpi_pytorch_amd.ops import functional as Fn
    from mpi_pytorch_amd.data.loader import IMAGENET_MEAN, IMAGENET_STD
    from mpi_pytorch_amd.parallel import World
    model, _opt, _step, _ = build_training("resnet18", 12, CPU, World(), 1e-3)
    model.eval()
    src = SyntheticImages((40, 40))
    names = ["img/%d.jpg" % i for i in range(30)]
    labels = list(np.random.default_rng(0).integers(0, 12, size=30))
    # plain per-batch counts with the oracle
    spec = input_spec(model, (32, 32))
    top1 = torch.zeros(1, dtype=torch.int64)
    top5 = torch.zeros(1, dtype=torch.int64)
    with torch.no_grad():
        for imgs, lab in _batches(names, labels, 8, src):
            x = Fn.preprocess(torch.from_numpy(imgs), (32, 32), IMAGENET_MEAN, IMAGENET_STD, 1,
                              spec["cpad"], out_dtype=torch.float32, pad=spec["pad"])
            out = model(x)
            ref.argmax_correct(out, lab, top1)
            ref.topk_correct(out, lab, 5, top5)
    pipe = StreamPipeline(model, CPU, (32, 32), lanes=2, assign="roundrobin", topk=5)
    counts = pipe.run(_batches(names, labels, 8, src))
    assert sum(counts) == int(top1)
    assert sum(pipe.topk_correct()) == int(top5) >= int(top1)
    # off by default, and for topk = 1
    for k in (0, 1):
        assert StreamPipeline(model, CPU, (32, 32), topk=k).topk_correct() == []
    # the driver logs the line after "Accuracy is"
    _reset_world()
    log = tmp_path / "evaluation.log"
    cfg = Config(synthetic_images=24, image_size=32, NUM_CLASSES=12, eval_batch=8, eval_topk=5,
                 CHECKPOINT_DIR=str(tmp_path) + "/ck/", device="cpu", log_file=str(log))
    acc = run_pipeline(cfg)
    lines = log.read_text().splitlines()
    at = [i for i, s in enumerate(lines) if "Top-5 accuracy is " in s]
    assert len(at) == 1 and "Accuracy is " in lines[at[0] - 1]
    assert float(lines[at[0]].rsplit(" ", 1)[1]) >= acc
