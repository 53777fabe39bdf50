"""The long-tail head on the CPU: the checks of ``test_longtail_gpu.py`` run with the oracle as
the implementation (every bound there is met by ``ops/ref.py`` alone), the oracle itself
against ``F.cross_entropy(x.float() + bias, ...)``, the class prior and the macro scores
against loops written here, and the plumbing from ``Config`` through the training driver,
the evaluation pipeline and two gloo ranks."""
import json
import math
import os
import re
import socket
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

import test_longtail_gpu as lt
from mpi_pytorch_amd.config import Config
from mpi_pytorch_amd.ops import ref

CPU = torch.device("cpu")


def _reset_world():
    import mpi_pytorch_amd.parallel.dist as D
    D._WORLD = None


# ------------------------------------------------- the GPU file's checks, on the oracle
@pytest.mark.parametrize("shape", lt.SHAPES)
def test_oracle_meets_adjusted_ce_checks(shape):
    for eps in lt.EPS:
        for mixed in (False, True):
            lt.check_adjusted_random(ref, CPU, *shape, eps, mixed)
    lt.check_constant_bias(ref, CPU, *shape)
    lt.check_null_and_zero_bias(ref, CPU, *shape)
    lt.check_flat_logits(ref, CPU, *shape)


def test_oracle_meets_weighted_and_autograd_checks():
    for shape in ((300, 33, 64), (7, 1000, 1024), (7, 1004, 1004)):
        lt.check_adjusted_weighted(ref, CPU, *shape)
    lt.check_autograd(CPU)


@pytest.mark.parametrize("shape", lt.SHAPES)
def test_oracle_meets_argmax_stats_checks(shape):
    lt.check_stats_vs_ref(ref, CPU, *shape)


def test_oracle_meets_argmax_stats_rule_checks():
    lt.check_stats_contention(ref, CPU)
    lt.check_stats_rules(ref, CPU)
    lt.check_stats_window(ref, CPU)
    lt.check_macro_scores(CPU)


def test_checks_see_a_misapplied_bias():
    """An implementation that drops the bias, applies it to the label only, or to the LSE
    only, or that reads the bias's NaN tail, fails."""
    class Dropped:
        @staticmethod
        def ce_fwd(logits, labels, eps=0.0, y2=None, lam=None, bias=None):
            return ref.ce_fwd(logits, labels, eps, y2, lam)

        @staticmethod
        def ce_bwd(logits, labels, lse, go, w=1.0, eps=0.0, y2=None, lam=None, bias=None):
            return ref.ce_bwd(logits, labels, lse, go, w, eps, y2, lam)

    class LabelOnly(Dropped):
        @staticmethod
        def ce_fwd(logits, labels, eps=0.0, y2=None, lam=None, bias=None):
            loss, lse = ref.ce_fwd(logits, labels, eps, y2, lam)
            return loss - bias[labels].mean(), lse

    class LseOnly(Dropped):
        @staticmethod
        def ce_fwd(logits, labels, eps=0.0, y2=None, lam=None, bias=None):
            _, lse = ref.ce_fwd(logits, labels, eps, y2, lam, bias)
            picked = logits.float().gather(1, labels.view(-1, 1)).squeeze(1)
            return (lse - picked).mean().reshape(1), lse

        ce_bwd = staticmethod(ref.ce_bwd)

    class ReadsTail:
        @staticmethod
        def ce_fwd(logits, labels, eps=0.0, y2=None, lam=None, bias=None):
            loss, lse = ref.ce_fwd(logits, labels, eps, y2, lam, bias)
            return loss + 0.0 * bias.sum(), lse

        ce_bwd = staticmethod(ref.ce_bwd)

    for impl in (Dropped, LabelOnly, LseOnly):
        with pytest.raises(AssertionError):
            lt.check_flat_logits(impl, CPU, 5, 33, 64)
    for impl in (Dropped, ReadsTail):
        with pytest.raises(AssertionError):
            lt.check_adjusted_random(impl, CPU, 5, 33, 64, 0.0, False)


# --------------------------------------------------------------- the oracle vs torch
@pytest.mark.parametrize("NC", [33, 1000, 64500])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("mixed", [False, True])
def test_oracle_matches_torch_cross_entropy_of_adjusted_logits(NC, eps, mixed):
    g = lt.gen(80)
    B = 6
    logits = (torch.randn(B, NC, generator=g) * 3 + 2).to(torch.bfloat16)
    y = torch.randint(0, NC, (B,), generator=g)
    bias = lt.zipf_log_prior(NC, g).float()
    x = logits.float().requires_grad_(True)
    mix = ()
    if mixed:  # probability targets
        y2 = torch.randint(0, NC, (B,), generator=g)
        lam = torch.rand(B, generator=g)
        tgt = torch.zeros(B, NC)
        tgt[torch.arange(B), y] += lam
        tgt[torch.arange(B), y2] += 1.0 - lam
        mix = (y2, lam)
        want = F.cross_entropy(x + bias, tgt, label_smoothing=eps)
    else:
        want = F.cross_entropy(x + bias, y, label_smoothing=eps)
    want.backward()
    loss, lse = ref.ce_fwd(logits, y, eps, *lt.mix_args(mix), bias)
    want = float(want.detach())
    assert abs(float(loss) - want) <= 1e-5 * abs(want)
    assert lt.rel(lse, torch.logsumexp(logits.float() + bias, 1)) < 1e-6
    d = ref.ce_bwd(logits.float(), y, lse, torch.ones(1), 1.0, eps, *lt.mix_args(mix), bias)
    assert lt.rel(d, x.grad) < 1e-4


# ------------------------------------------------------------------- prior and scores
def test_class_log_prior_matches_a_float64_loop():
    from mpi_pytorch_amd.data.longtail import class_log_prior, logit_bias
    labels = [0, 0, 0, 3, 3, 1, 5, 5, 5, 5]
    NC = 7  # classes 2, 4 and 6 have no image
    got = class_log_prior(labels, NC)
    assert got.dtype == torch.float32 and got.shape == (NC,)
    for c in range(NC):
        n = sum(1 for v in labels if v == c)
        want = math.log((n + 1.0) / (len(labels) + NC))
        assert float(got[c]) == float(np.float32(want)), c
    assert bool(torch.isfinite(got).all()) and float(got[2]) == float(got[4]) < float(got[1])
    # numpy labels, any order: the same vector bitwise
    perm = np.random.default_rng(0).permutation(len(labels))
    assert torch.equal(class_log_prior(np.asarray(labels)[perm], NC), got)
    b = logit_bias(labels, NC, 0.5)
    assert b.dtype == torch.float32 and b.is_contiguous() and torch.equal(b, got * 0.5)
    with pytest.raises(ValueError):
        logit_bias(labels, NC, -1.0)
    with pytest.raises(ValueError):
        class_log_prior(labels, 0)


def test_macro_scores_rejects_other_shapes():
    from mpi_pytorch_amd.metrics import macro_scores
    with pytest.raises(ValueError):
        macro_scores(torch.zeros(2, 5, dtype=torch.int64))


# ------------------------------------------------------------------------- plumbing
def test_config_validates_and_overrides(monkeypatch):
    c = Config()
    assert c.logit_adjust_tau == 0.0 and c.eval_macro is False
    for bad in (-0.01, float("nan")):
        with pytest.raises(ValueError):
            Config(logit_adjust_tau=bad)
    c = Config.from_args(["--logit_adjust_tau", "1.5", "--eval_macro", "true"])
    assert c.logit_adjust_tau == 1.5 and c.eval_macro is True
    c = Config.from_args(["--logit-adjust-tau", "0.5", "--eval-macro", "1"])
    assert c.logit_adjust_tau == 0.5 and c.eval_macro is True
    monkeypatch.setenv("MPA_LOGIT_ADJUST_TAU", "2")
    monkeypatch.setenv("MPA_EVAL_MACRO", "true")
    c = Config.from_args([])
    assert c.logit_adjust_tau == 2.0 and c.eval_macro is True


def test_step_loss_is_torch_cross_entropy_of_adjusted_logits():
    from mpi_pytorch_amd.engine import build_training
    from mpi_pytorch_amd.parallel import World
    bias = lt.step_bias()
    losses = {}
    for name, kw in (("adj", dict(logit_bias=bias)), ("none", dict(logit_bias=None)),
                     ("plain", {})):
        torch.manual_seed(0)
        model, opt, step, _ = build_training("resnet18", lt.NCLS, CPU, World(), 1e-3,
                                             label_smoothing=0.1, **kw)
        seen = []
        model.register_forward_hook(lambda m, i, o: seen.append(o.detach().clone()))
        g = lt.gen(1)
        x, y = torch.randn(6, 32, 32, 3, generator=g), torch.randint(0, lt.NCLS, (6,), generator=g)
        losses[name] = (step(x, y).clone(), model._mpa_arena.master.clone())
        if name == "adj":
            assert torch.equal(step.logit_bias, bias)
            want = float(F.cross_entropy(seen[0].float() + bias, y, label_smoothing=0.1))
            plain = float(F.cross_entropy(seen[0].float(), y, label_smoothing=0.1))
            assert abs(float(losses[name][0]) - want) <= 1e-5 * abs(want)
            assert abs(want - plain) > 1e-3
        else:
            assert step.logit_bias is None
    assert all(torch.equal(a, b) for a, b in zip(losses["none"], losses["plain"]))
    assert not torch.equal(losses["adj"][1], losses["plain"][1])
    with pytest.raises(ValueError):
        build_training("resnet18", lt.NCLS, CPU, World(), 1e-3, logit_bias=bias[:-1])


def _shape_of(line):
    return re.sub(r"[-+]?\d+(\.\d+)?(e[-+]?\d+)?", "#", line)


def test_training_driver_logs_macro_scores_after_the_unchanged_lines(tmp_path, monkeypatch):
    import mpi_pytorch_amd.engine.trainer as T
    built = []
    real = T.build_training
    monkeypatch.setattr(T, "build_training",
                        lambda *a, **kw: built.append(kw.get("logit_bias")) or real(*a, **kw))
    texts = {}
    runs = (("plain", {}),
            ("tail", dict(logit_adjust_tau=1.0, eval_macro=True, ema_decay=0.9, eval_topk=5)),
            ("ema", dict(ema_decay=0.9, eval_topk=5)))
    for name, extra in runs:
        _reset_world()
        d = tmp_path / name
        d.mkdir()
        cfg = Config(synthetic_images=32, image_size=32, NUM_EPOCHS=1, BATCH_SIZE=16,
                     NUM_CLASSES=50, CHECKPOINT_DIR=str(d) + "/ck/", device="cpu",
                     log_file=str(d / "training.log"), metrics_jsonl=str(d / "m.jsonl"), **extra)
        T.run_training(cfg)
        texts[name] = (d / "training.log").read_text().splitlines()
    # tau = 0 builds the step without a bias: the call path it always had
    assert built[0] is None and built[2] is None
    assert built[1].dtype == torch.float32 and built[1].shape == (50,)
    rec = json.loads((tmp_path / "tail" / "m.jsonl").read_text().splitlines()[0])
    other = json.loads((tmp_path / "ema" / "m.jsonl").read_text().splitlines()[0])
    new_keys = {"macro_f1", "balanced_acc", "macro_f1_ema", "balanced_acc_ema"}
    assert new_keys <= set(rec) and not new_keys & set(other)
    assert set(rec) - new_keys == set(other)
    for k in new_keys:
        assert 0.0 <= rec[k] <= 1.0
    lines = texts["tail"]
    at = [i for i, s in enumerate(lines) if "Macro-F1: " in s]
    assert len(at) == 2
    assert "_Epoch: 0 | Macro-F1: " in lines[at[0]] and " | Balanced Acc: " in lines[at[0]]
    assert "_Epoch: 0 | Top-5 Acc: " in lines[at[0] - 1]
    assert "_Epoch: 0 | EMA Macro-F1: " in lines[at[1]] and "| EMA Balanced Acc: " in lines[at[1]]
    assert "_Epoch: 0 | EMA Top-5 Acc: " in lines[at[1] - 1] and at[1] == len(lines) - 1
    assert float(lines[at[0]].rsplit(" ", 1)[1]) == rec["balanced_acc"]
    assert float(lines[at[1]].rsplit(" ", 1)[1]) == rec["balanced_acc_ema"]
    adj = [i for i, s in enumerate(lines) if "_Logit adjustment: tau 1.0" in s]
    assert len(adj) == 1
    rest = [s for i, s in enumerate(lines) if i not in at + adj]
    assert [_shape_of(s) for s in rest] == [_shape_of(s) for s in texts["ema"]]
    assert not any("Macro" in s or "Logit adjustment" in s for s in texts["plain"] + texts["ema"])


def _tiny_eval_model():
    from mpi_pytorch_amd.engine import build_training
    from mpi_pytorch_amd.parallel import World
    torch.manual_seed(0)
    model, _opt, _step, _ = build_training("resnet18", 12, CPU, World(), 1e-3)
    model.eval()
    return model


def _plain_stats(model, names, labels):
    """Plain batched evaluation with the oracle: (top-1 count, stats)."""
    from mpi_pytorch_amd.engine.eval_pipeline import _batches
    from mpi_pytorch_amd.data.manifest import SyntheticImages
    from mpi_pytorch_amd.models import input_spec
    from mpi_pytorch_amd.ops import functional as Fn
    from mpi_pytorch_amd.data.loader import IMAGENET_MEAN, IMAGENET_STD
    spec = input_spec(model, (32, 32))
    top1 = torch.zeros(1, dtype=torch.int64)
    plain = torch.zeros(1, dtype=torch.int64)
    stats = torch.zeros(3, 12, dtype=torch.int64)
    with torch.no_grad():
        for imgs, lab in _batches(names, labels, 8, SyntheticImages((40, 40))):
            x = Fn.preprocess(torch.from_numpy(imgs), (32, 32), IMAGENET_MEAN, IMAGENET_STD, 1,
                              spec["cpad"], out_dtype=torch.float32, pad=spec["pad"])
            out = model(x)
            ref.argmax_stats(out, lab, top1, stats)
            ref.argmax_correct(out, lab, plain)
    assert int(top1) == int(plain)
    return int(top1), stats


def test_eval_pipeline_collects_class_stats(tmp_path):
    from mpi_pytorch_amd.engine.eval_pipeline import StreamPipeline, _batches, run_pipeline
    from mpi_pytorch_amd.data.manifest import SyntheticImages
    from mpi_pytorch_amd.metrics import macro_scores
    model = _tiny_eval_model()
    src = SyntheticImages((40, 40))
    names = ["img/%d.jpg" % i for i in range(30)]
    labels = list(np.random.default_rng(0).integers(0, 12, size=30))
    top1, stats = _plain_stats(model, names, labels)
    assert int(stats[0].sum()) == 30 == int(stats[1].sum()) and int(stats[2].sum()) == top1
    pipe = StreamPipeline(model, CPU, (32, 32), lanes=2, assign="roundrobin", macro=True)
    counts = pipe.run(_batches(names, labels, 8, src))
    assert sum(counts) == top1
    assert all(s is not None for s in pipe.stats) and torch.equal(pipe.class_stats(), stats)
    off = StreamPipeline(model, CPU, (32, 32))
    assert off.run(_batches(names, labels, 8, src)) == [top1] and off.class_stats() is None
    # the driver logs the two lines after the accuracy lines
    _reset_world()
    log = tmp_path / "evaluation.log"
    cfg = Config(synthetic_images=24, image_size=32, NUM_CLASSES=12, eval_batch=8, eval_topk=5,
                 eval_macro=True, CHECKPOINT_DIR=str(tmp_path) + "/ck/", device="cpu",
                 log_file=str(log))
    run_pipeline(cfg)
    lines = log.read_text().splitlines()
    at = [i for i, s in enumerate(lines) if "Macro-F1 is " in s]
    assert len(at) == 1 and "Top-5 accuracy is " in lines[at[0] - 1]
    assert "Accuracy is " in lines[at[0] - 2] and "Balanced accuracy is " in lines[at[0] + 1]
    for i in (at[0], at[0] + 1):
        assert 0.0 <= float(lines[i].rsplit(" ", 1)[1]) <= 1.0
    _reset_world()
    log2 = tmp_path / "evaluation2.log"
    run_pipeline(Config(synthetic_images=24, image_size=32, NUM_CLASSES=12, eval_batch=8,
                        eval_topk=5, CHECKPOINT_DIR=str(tmp_path) + "/ck/", device="cpu",
                        log_file=str(log2)))
    plain_lines = log2.read_text().splitlines()
    rest = lines[:at[0]] + lines[at[0] + 2:]
    assert [_shape_of(s) for s in rest] == [_shape_of(s) for s in plain_lines]
    assert isinstance(macro_scores(stats)["macro_f1"], float)


# ------------------------------------------------------------------------ two gloo ranks
N_EVAL = 30


def _manifest_labels():
    return np.random.default_rng(5).integers(0, 12, size=200) ** 2 // 11  # (skewed)


def _eval_set():
    names = ["img/%d.jpg" % i for i in range(N_EVAL)]
    return names, list(np.random.default_rng(0).integers(0, 12, size=N_EVAL))


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
    from mpi_pytorch_amd.parallel import init_world, shutdown
    from mpi_pytorch_amd.engine.trainer import shared_logit_bias
    from mpi_pytorch_amd.engine.eval_pipeline import (StreamPipeline, _batches,
                                                      global_class_stats)
    from mpi_pytorch_amd.data.manifest import SyntheticImages
    import mpi_pytorch_amd.parallel.dist as D
    D._WORLD = None
    init_world("cpu")
    cfg = Config(NUM_CLASSES=12, logit_adjust_tau=1.5, device="cpu")
    # only rank 0 holds the manifest
    bias = shared_logit_bias(cfg, _manifest_labels() if rank == 0 else None, rank)
    assert shared_logit_bias(Config(NUM_CLASSES=12, device="cpu"), None, rank) is None
    model = _tiny_eval_model()
    names, labels = _eval_set()
    mine = slice(rank, None, world)
    pipe = StreamPipeline(model, CPU, (32, 32), lanes=2, assign="roundrobin", macro=True)
    counts = pipe.run(_batches(names[mine], labels[mine], 8, SyntheticImages((40, 40))))
    stats = global_class_stats(pipe, 12)
    torch.save({"bias": bias, "stats": stats, "count": sum(counts)},
               os.path.join(out_dir, "r%d.pt" % rank))
    shutdown()


def test_two_ranks_share_the_bias_and_sum_their_class_stats():
    from mpi_pytorch_amd.data.longtail import logit_bias
    with tempfile.TemporaryDirectory() as d:
        mp.start_processes(_worker, args=(2, _free_port(), d), nprocs=2, join=True,
                           start_method="spawn")
        r0, r1 = (torch.load(os.path.join(d, "r%d.pt" % r)) for r in range(2))
    assert r0["bias"].dtype == torch.float32 and torch.equal(r0["bias"], r1["bias"])
    assert torch.equal(r0["bias"], logit_bias(_manifest_labels(), 12, 1.5))
    names, labels = _eval_set()
    top1, stats = _plain_stats(_tiny_eval_model(), names, labels)
    assert torch.equal(r0["stats"], stats) and torch.equal(r1["stats"], stats)
    assert r0["count"] + r1["count"] == top1 == int(stats[2].sum())
