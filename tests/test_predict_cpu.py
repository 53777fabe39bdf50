"""Top-k predictions on the CPU: the kernel checks of ``test_predict_gpu.py`` run with the
oracle as the implementation (every bound there is met by ``ops/ref.py`` alone), the oracle
against float64, the pipeline's prediction arrays on the CPU path, and the driver: the
predictions file, unlabelled manifests, two gloo ranks and ``Config``."""
import csv
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import test_predict_gpu as pg
from test_loss_head_gpu import SHAPES, padded
from mpi_pytorch_amd.config import Config
from mpi_pytorch_amd.ops import ref

CPU = torch.device("cpu")


def _reset_world():
    import mpi_pytorch_amd.parallel.dist as D
    D._WORLD = None


# ------------------------------------------------- the GPU file's checks, on the oracle
@pytest.mark.parametrize("shape", SHAPES)
def test_oracle_meets_topk_predict_checks(shape):
    for k in pg.KS:
        pg.check_vs_oracle(ref, CPU, *shape, k)
        pg.check_vs_counting(ref, CPU, *shape, k)
    pg.check_tie_free(ref, CPU, *shape)


def test_oracle_meets_topk_predict_rule_checks():
    pg.check_tie_rule(ref, CPU)
    pg.check_nan_inf_short(ref, CPU)
    pg.check_nan_inf_short(ref, CPU, 41, 7)
    pg.check_windows(ref, CPU)
    pg.check_rows_independent(ref, CPU, 300, 33, 64)
    pg.check_rows_independent(ref, CPU, 4, 64500, 64512)
    pg.check_refusals(ref, CPU, ValueError)


@pytest.mark.parametrize("shape", [(5, 33, 64), (7, 1000, 1024), (4, 64500, 64512)])
def test_oracle_log_probabilities_match_float64(shape):
    B, NC, ld = shape
    torch.manual_seed(70)
    logits = padded(torch.randn(B, NC) * 3, ld)
    idx, prob = pg.predict(ref, logits, 16)
    x = logits.double()
    want = x.gather(1, idx.long()) - torch.logsumexp(x, 1, keepdim=True)
    err = ((prob.double().log() - want).abs() / want.abs().clamp_min(1.0)).max()
    assert float(err) <= 1e-5  # (three orders under the kernel's bound)


def test_checks_see_a_wrong_tie_order_and_a_pad_read():
    """The checks fail an implementation that breaks ties towards the higher index, and one
    that ranks the pad columns."""
    class HighIndexFirst:
        @staticmethod
        def topk_predict(logits, k, idx, prob):
            flipped = torch.flip(logits.float(), [1])
            ref.topk_predict(flipped, k, idx, prob)
            idx.copy_(torch.where(idx >= 0, logits.shape[1] - 1 - idx, idx))

    class ReadsThePad:
        @staticmethod
        def topk_predict(logits, k, idx, prob):
            B, NC = logits.shape
            ld = logits.stride(0)
            ref.topk_predict(logits.as_strided((B, ld), (ld, 1), logits.storage_offset()), k,
                             idx, prob)

    with pytest.raises(AssertionError):
        pg.check_tie_rule(HighIndexFirst, CPU)
    with pytest.raises(AssertionError):
        pg.check_vs_oracle(HighIndexFirst, CPU, 4, 64500, 64512, 16)
    with pytest.raises(AssertionError):
        pg.check_vs_oracle(ReadsThePad, CPU, 5, 33, 64, 5)


def test_predict_topk_op_on_the_cpu():
    from mpi_pytorch_amd.ops import functional as Fn
    torch.manual_seed(78)
    logits = torch.randn(7, 50)
    idx, prob = Fn.predict_topk(logits, 3)
    assert idx.dtype == torch.int32 and prob.dtype == torch.float32 and idx.shape == (7, 3)
    assert torch.equal(idx.long(), logits.topk(3, 1).indices)
    assert torch.allclose(prob, torch.softmax(logits, 1).gather(1, idx.long()), rtol=1e-5)
    with pytest.raises(ValueError):
        Fn.predict_topk(logits, 0)


# ------------------------------------------------------------------------- the pipeline
NCLS = 12


def _tiny_eval_model():
    from mpi_pytorch_amd.engine import build_training
    from mpi_pytorch_amd.parallel import World
    torch.manual_seed(0)
    model, _opt, _step, _ = build_training("resnet18", NCLS, CPU, World(), 1e-3)
    model.eval()
    return model


def test_cpu_pipeline_predictions_equal_plain_predict():
    from mpi_pytorch_amd.engine.eval_pipeline import (StreamPipeline, _batches, plain_eval,
                                                      plain_predict)
    from mpi_pytorch_amd.data.manifest import SyntheticImages
    model = _tiny_eval_model()
    src = SyntheticImages((40, 40))
    names = ["img/%d.jpg" % i for i in range(30)]
    labels = list(np.random.default_rng(0).integers(0, NCLS, size=30))
    want_i, want_p = plain_predict(model, names, 8, src, CPU, (32, 32), 5)
    assert want_i.shape == want_p.shape == (30, 5) and want_i.dtype == np.int32
    pipe = StreamPipeline(model, CPU, (32, 32), lanes=2, assign="random", predict_k=5)
    counts = pipe.run(_batches(names, labels, 8, src), rows=30)
    idx, prob = pipe.predictions()
    assert np.array_equal(idx, want_i) and np.array_equal(prob, want_p)
    assert sum(counts) == plain_eval(model, names, labels, 8, src, CPU, (32, 32))
    assert int((idx[:, 0] == np.asarray(labels)).sum()) == sum(counts)
    assert (np.diff(prob, axis=1) <= 0).all() and 0 < float(prob.sum(1).max()) <= 1 + 1e-3
    # off by default: nothing allocated, the same counts
    off = StreamPipeline(model, CPU, (32, 32), lanes=2, assign="random")
    assert off.run(_batches(names, labels, 8, src)) == counts
    assert off.predictions() is None and off.pred_idx is None
    with pytest.raises(ValueError):  # the arrays cannot be sized without the row count
        pipe.run(_batches(names, labels, 8, src))
    for bad in (-1, 17):
        with pytest.raises(ValueError):
            StreamPipeline(model, CPU, (32, 32), predict_k=bad)


# --------------------------------------------------------------------------- the driver
def _cfg(tmp_path, **kw):
    """A driver configuration whose checkpoint directory holds one seeded model (without a
    checkpoint every run would predict with fresh random weights)."""
    from mpi_pytorch_amd.checkpoint import save_checkpoint
    from mpi_pytorch_amd.models import initialize_model
    ckdir = str(tmp_path) + "/ck/"
    if not os.path.exists(ckdir):
        torch.manual_seed(3)
        model, _ = initialize_model("resnet18", NCLS, False, False)
        save_checkpoint({"epoch": 0, "state_dict": model.state_dict()}, 0, "resnet18", ckdir)
    kw.setdefault("synthetic_images", 32)
    return Config(image_size=32, NUM_CLASSES=NCLS, eval_batch=8, device="cpu",
                  CHECKPOINT_DIR=ckdir, **kw)


def _read(path):
    with open(path, newline="") as fh:
        rows = list(csv.reader(fh))
    return rows[0], rows[1:]


@pytest.mark.parametrize("k", [1, 3])
def test_driver_writes_the_predictions_file(tmp_path, k):
    from mpi_pytorch_amd.engine.eval_pipeline import load_predictor, plain_predict, run_pipeline
    from mpi_pytorch_amd.data.manifest import SyntheticImages, synthetic_manifest
    _reset_world()
    out = tmp_path / "sub" / "pred.csv"  # (the directory is made)
    log = tmp_path / "evaluation.log"
    cfg = _cfg(tmp_path, predictions_csv=str(out), predict_topk=k, log_file=str(log))
    acc = run_pipeline(cfg)
    assert os.listdir(out.parent) == ["pred.csv"]  # no temporary file left behind
    plain_file = tmp_path / "plain_open.txt"
    plain_file.write_text("x")  # the mode of a file made by open(), not the temp file's 0600
    assert os.stat(out).st_mode & 0o777 == os.stat(plain_file).st_mode & 0o777
    header, rows = _read(out)
    want_header = ["Id", "Predicted", "Probability"]
    for j in range(2, k + 1):
        want_header += ["Predicted_%d" % j, "Probability_%d" % j]
    assert header == want_header
    df = synthetic_manifest(32, NCLS, cfg.seed)
    assert [r[0] for r in rows] == [str(v) for v in df["file_name"].values]
    idx, prob = plain_predict(load_predictor(cfg, CPU), list(df["file_name"].values), 8,
                              SyntheticImages((32, 32)), CPU, (32, 32), k)
    for j in range(k):
        assert [int(r[1 + 2 * j]) for r in rows] == idx[:, j].tolist()
        # %.9g: the float32 comes back bit for bit
        assert np.array_equal(np.array([r[2 + 2 * j] for r in rows], dtype=np.float64)
                              .astype(np.float32), prob[:, j])
    hits = sum(int(r[1]) == int(c) for r, c in zip(rows, df["category_id"].values))
    assert hits / 32 == acc
    lines = log.read_text().splitlines()
    at = [i for i, s in enumerate(lines) if "Predictions written to " in s]
    acc_at = [i for i, s in enumerate(lines) if "Accuracy is " in s]
    assert len(at) == 1 and len(acc_at) == 1 and at[0] > acc_at[0]
    assert lines[at[0]].endswith("Predictions written to {} (32 rows, top-{})".format(out, k))
    # without the flag: no file, the same lines but that one
    _reset_world()
    log2 = tmp_path / "evaluation2.log"
    assert run_pipeline(_cfg(tmp_path, predict_topk=k, log_file=str(log2))) == acc
    plain = log2.read_text().splitlines()
    assert len(plain) == len(lines) - 1 and not any("Predictions" in s for s in plain)


def test_driver_runs_an_unlabelled_manifest(tmp_path):
    from mpi_pytorch_amd.engine.eval_pipeline import run_pipeline
    from mpi_pytorch_amd.data.manifest import synthetic_manifest
    df = synthetic_manifest(32, NCLS, 0)
    # labelled, through a manifest file: the reference run
    _reset_world()
    full = tmp_path / "labelled.csv"
    df.to_csv(full, index=False)
    want = tmp_path / "want.csv"
    acc = run_pipeline(_cfg(tmp_path, synthetic_images=0, TEST_CSV=str(full), eval_topk=5,
                            eval_macro=True, predictions_csv=str(want),
                            log_file=str(tmp_path / "a.log")))
    assert 0.0 <= acc <= 1.0
    # the same manifest without its labels
    _reset_world()
    bare = tmp_path / "unlabelled.csv"
    df.drop(columns=["category_id"]).to_csv(bare, index=False)
    out = tmp_path / "pred.csv"
    log = tmp_path / "b.log"
    got = run_pipeline(_cfg(tmp_path, synthetic_images=0, TEST_CSV=str(bare), eval_topk=5,
                            eval_macro=True, predictions_csv=str(out), log_file=str(log)))
    assert math.isnan(got)
    assert out.read_bytes() == want.read_bytes()
    lines = log.read_text().splitlines()
    assert sum("No labels in {}: accuracy not computed".format(bare) in s for s in lines) == 1
    assert not any("ccuracy is " in s or "Macro-F1" in s for s in lines)
    assert any("Predictions written to " in s for s in lines)


def test_predictions_file_uses_the_id_column(tmp_path):
    from mpi_pytorch_amd.engine.eval_pipeline import run_pipeline
    from mpi_pytorch_amd.data.manifest import synthetic_manifest
    _reset_world()
    df = synthetic_manifest(16, NCLS, 0)
    if "id" in df.columns:
        df = df.drop(columns=["id"])
    df.insert(0, "id", np.arange(16) * 3 + 100)
    src = tmp_path / "ids.csv"
    df.to_csv(src, index=False)
    out = tmp_path / "pred.csv"
    run_pipeline(_cfg(tmp_path, synthetic_images=0, TEST_CSV=str(src), predictions_csv=str(out),
                      log_file=str(tmp_path / "e.log")))
    assert [r[0] for r in _read(out)[1]] == [str(100 + 3 * i) for i in range(16)]


# ------------------------------------------------------------------------ two gloo ranks
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
    from mpi_pytorch_amd.parallel import shutdown
    from mpi_pytorch_amd.engine.eval_pipeline import run_pipeline
    import mpi_pytorch_amd.parallel.dist as D
    D._WORLD = None
    acc = run_pipeline(Config(image_size=32, NUM_CLASSES=NCLS, eval_batch=8, device="cpu",
                              synthetic_images=32, CHECKPOINT_DIR=out_dir + "/ck/",
                              predictions_csv=out_dir + "/two.csv", predict_topk=3,
                              log_file=out_dir + "/two.log"))
    if rank == 0:
        with open(out_dir + "/acc.txt", "w") as fh:
            fh.write(repr(acc))
    shutdown()


def test_two_ranks_write_the_single_rank_file(tmp_path):
    """32 images, batch 8: both ranks' batches are the single-rank run's batches, so the file
    is the single-rank file byte for byte."""
    from mpi_pytorch_amd.engine.eval_pipeline import run_pipeline
    cfg = _cfg(tmp_path, predictions_csv=str(tmp_path / "one.csv"), predict_topk=3,
               log_file=str(tmp_path / "one.log"))  # (writes the checkpoint the ranks load)
    mp.start_processes(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True,
                       start_method="spawn")
    _reset_world()
    one = tmp_path / "one.csv"
    threads = torch.get_num_threads()
    torch.set_num_threads(1)  # as the ranks run: the forward's sums in the same order
    try:
        acc = run_pipeline(cfg)
    finally:
        torch.set_num_threads(threads)
    assert (tmp_path / "two.csv").read_bytes() == one.read_bytes()
    assert len(one.read_text().splitlines()) == 33
    assert abs(float((tmp_path / "acc.txt").read_text()) - acc) < 1e-12
    assert sorted(p for p in os.listdir(tmp_path) if p.endswith(".csv")) == ["one.csv", "two.csv"]


# ------------------------------------------------------------------------------ config
def test_config_defaults_overrides_and_refusals(monkeypatch):
    c = Config()
    assert c.predictions_csv == "" and c.predict_topk == 1
    for bad in (0, 17, -3):
        with pytest.raises(ValueError):
            Config(predict_topk=bad)
    assert Config(predict_topk=16).predict_topk == 16
    c = Config.from_args(["--predictions_csv", "out.csv", "--predict-topk", "5"])
    assert c.predictions_csv == "out.csv" and c.predict_topk == 5
    monkeypatch.setenv("MPA_PREDICTIONS_CSV", "env.csv")
    monkeypatch.setenv("MPA_PREDICT_TOPK", "3")
    c = Config.from_args([])
    assert c.predictions_csv == "env.csv" and c.predict_topk == 3
    assert Config.from_args(["--predict_topk", "7"]).predict_topk == 7  # flags beat the env
    monkeypatch.setenv("MPA_PREDICT_TOPK", "0")
    with pytest.raises(ValueError):
        Config.from_args([])
