"""Mixup / CutMix on the CPU: the checks of ``test_mix_gpu.py`` run with the oracle as the
implementation (every bound there is met by ``ops/ref.py`` alone), the oracle against
``F.cross_entropy`` with class-probability targets, the sampler (``data/augment.py::
sample_mix``), and the plumbing from ``Config`` through the loader, the step and the driver."""
import json
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_loss_head_gpu as lh
import test_mix_gpu as mg
from mpi_pytorch_amd.config import Config
from mpi_pytorch_amd.data.augment import _mix_draws, label_weights, sample_ids, sample_mix
from mpi_pytorch_amd.ops import functional as Fn
from mpi_pytorch_amd.ops import ref

CPU = torch.device("cpu")


def _reset_world():
    import mpi_pytorch_amd.parallel.dist as D
    D._WORLD = None


# ------------------------------------------------- the GPU file's checks, on the oracle
# (On the CPU ``pre`` asks the oracle for bf16 output, so P is rounded to bf16 before the
# blend and the identity is exact here too.)
@pytest.mark.parametrize("case", mg.CASES[::4], ids=str)
def test_oracle_meets_blend_checks(case):
    mg.check_blend(CPU, case)


def test_oracle_meets_inert_oracle_and_rejection_checks():
    mg.check_inert(CPU, mg.CASES[0])
    mg.check_against_oracle(CPU, mg.CASES[5])
    mg.check_rejections(CPU)


@pytest.mark.parametrize("shape", lh.SHAPES)
def test_oracle_meets_mixed_ce_checks(shape):
    for eps in mg.CE_EPS:
        mg.check_ce_random(ref, CPU, *shape, eps)
        mg.check_ce_flat(ref, CPU, *shape, eps)
    mg.check_ce_bitwise(ref, CPU, *shape)


def test_oracle_meets_mixed_weighted_and_autograd_checks():
    for shape in ((300, 33, 64), (7, 1000, 1024), (7, 1004, 1004)):
        mg.check_ce_weighted(ref, CPU, *shape)
    mg.check_ce_autograd(CPU)


def test_flat_check_sees_a_dropped_second_label():
    """The closed forms fail an implementation that ignores labels2 in the backward."""
    class OneLabel:
        ce_fwd = staticmethod(ref.ce_fwd)

        @staticmethod
        def ce_bwd(logits, labels, lse, go, weight, eps, labels2, lam):
            return ref.ce_bwd(logits, labels, lse, go, weight, eps)

    with pytest.raises(AssertionError):
        mg.check_ce_flat(OneLabel, CPU, 4, 64500, 64512, 0.1)


# ------------------------------------------------------------------- the oracle vs torch
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_oracle_is_torch_cross_entropy_with_probability_targets(eps):
    torch.manual_seed(3)
    Bn, NC = 9, 37
    x = (torch.randn(Bn, NC) * 3 + 2).requires_grad_(True)
    y, y2, lam = mg.mixed_labels(Bn, NC, CPU)
    tgt = lam[:, None] * F.one_hot(y, NC) + (1 - lam[:, None]) * F.one_hot(y2, NC)
    want = F.cross_entropy(x, tgt, label_smoothing=eps)
    want.backward()
    loss, lse = ref.ce_fwd(x.detach(), y, eps, y2, lam)
    assert abs(float(loss) - float(want)) <= 1e-5 * abs(float(want))
    d = ref.ce_bwd(x.detach(), y, lse, torch.ones(1), 1.0, eps, y2, lam)
    assert lh.rel(d, x.grad) < 1e-4


# ----------------------------------------------------------------------------- sampler
HW = (32, 48)


def test_sampler_is_a_function_of_its_arguments():
    ids = np.arange(64, dtype=np.uint32) * 7 + 3
    a = sample_mix(ids, 2, 5, HW, 0.2, 1.0)
    b = sample_mix(ids, 2, 5, HW, 0.2, 1.0)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    assert a[0].dtype == np.int32 and a[0].shape == (64, 5)
    assert a[1].dtype == np.float32 and a[1].shape == (64,)
    for other in (sample_mix(ids, 3, 5, HW, 0.2, 1.0), sample_mix(ids, 2, 6, HW, 0.2, 1.0),
                  sample_mix(ids[::-1], 2, 5, HW, 0.2, 1.0)):
        assert not (np.array_equal(other[0], a[0]) and np.array_equal(other[1], a[1]))
    assert np.array_equal(a[0][:, 0], (np.arange(64) + 1) % 64)      # the next sample


def test_sampler_rows_are_valid_and_label_weights_exact():
    ids = np.arange(512, dtype=np.uint32)
    OH, OW = HW
    mix, lam = sample_mix(ids, 0, 1, HW, 0.4, 1.0)
    p, y0, x0, h, w = (mix[:, i].astype(np.int64) for i in range(5))
    assert (h >= 0).all() and (w >= 0).all() and (y0 >= 0).all() and (x0 >= 0).all()
    assert (y0 + h <= OH).all() and (x0 + w <= OW).all()
    assert np.isfinite(lam).all() and (lam >= 0).all() and (lam <= 1).all()
    cut = (h > 0) & (w > 0)
    assert 100 < cut.sum() < 400                                      # both methods occur
    assert (lam[cut] == 1.0).all()                                    # the rectangle mixes
    assert ((h == 0) == (w == 0)).all()                               # empty means (.., 0, 0)
    lw = label_weights(mix, lam, HW)
    assert lw.dtype == np.float32
    assert np.array_equal(lw[cut], (1.0 - (h * w)[cut] / float(OH * OW)).astype(np.float32))
    assert np.array_equal(lw[~cut], lam[~cut])
    assert len(np.unique(lam[~cut])) > 50                             # Mixup rows: Beta draws
    # the rows pass the host check of the op they feed
    Fn._check_mix(mix, lam, 512, HW, 0)
    # prob = 0: all-identity rows
    mix0, lam0 = sample_mix(ids, 0, 1, HW, 0.4, 1.0, prob=0.0)
    assert not mix0[:, 1:].any() and (lam0 == 1.0).all()
    assert (label_weights(mix0, lam0, HW) == 1.0).all()
    # one method on: only that one
    mixm, lamm = sample_mix(ids, 0, 1, HW, 0.4, 0.0)
    assert not mixm[:, 1:].any() and (lamm < 1.0).sum() > 400
    mixc, lamc = sample_mix(ids, 0, 1, HW, 0.0, 1.0)
    assert (lamc == 1.0).all() and (mixc[:, 3] > 0).sum() > 400
    for bad in (dict(mixup_alpha=-1.0, cutmix_alpha=1.0), dict(mixup_alpha=0.2, cutmix_alpha=-0.1)):
        with pytest.raises(ValueError):
            sample_mix(ids, 0, 1, HW, **bad)
    with pytest.raises(ValueError):
        sample_mix(ids, 0, 1, HW, 0.2, 1.0, prob=1.5)


def test_sampler_distributions():
    """cutmix_alpha = 1 draws l0 uniformly: over 4,096 samples the share below 0.25 lies within
    four binomial standard deviations, 4 * sqrt(0.25 * 0.75 / 4096) = 0.027, of 0.25; with
    both methods on and switch_prob 0.5 the CutMix share lies within 4 * sqrt(0.25 / 4096) =
    0.032 of 0.5."""
    ids = np.arange(4096, dtype=np.uint32)
    mixed, cut, l0, _uy, _ux = _mix_draws(ids, 0, 11, 0.0, 1.0, 1.0, 0.5)
    assert mixed.all() and cut.all()
    assert abs(float((l0 < 0.25).mean()) - 0.25) <= 0.027
    mixed, cut, _b, _uy, _ux = _mix_draws(ids, 0, 11, 0.2, 1.0, 1.0, 0.5)
    assert mixed.all()
    assert abs(float(cut.mean()) - 0.5) <= 0.032
    # the rectangle follows l0: sides int(OH * r), int(OW * r) before clipping
    mix, _lam = sample_mix(ids, 0, 11, (64, 64), 0.0, 1.0)
    _m, _c, l0, _uy, _ux = _mix_draws(ids, 0, 11, 0.0, 1.0, 1.0, 0.5)
    side = (64 * np.sqrt(1.0 - l0)).astype(np.int64)
    assert (mix[:, 3] <= side).all() and (mix[:, 4] <= side).all()
    inner = (mix[:, 1] > 0) & (mix[:, 2] > 0) & (mix[:, 1] + mix[:, 3] < 64) & \
        (mix[:, 2] + mix[:, 4] < 64)                                   # not clipped
    assert inner.sum() > 500
    assert np.array_equal(mix[inner, 3], (side // 2 * 2)[inner])


# ------------------------------------------------------------------------------ config
def test_config_mix_fields(monkeypatch):
    c = Config()
    assert (c.mixup_alpha, c.cutmix_alpha, c.mix_prob, c.mix_switch_prob) == (0.0, 0.0, 1.0, 0.5)
    assert c.mix_spec is None
    for kw in (dict(mixup_alpha=-0.1), dict(cutmix_alpha=-1.0), dict(mix_prob=1.5),
               dict(mix_prob=-0.1), dict(mix_switch_prob=2.0), dict(mixup_alpha=float("nan"))):
        with pytest.raises(ValueError):
            Config(**kw)
    c = Config.from_args(["--mixup_alpha", "0.2", "--cutmix-alpha", "1.0", "--mix-prob", "0.8",
                          "--seed", "3"])
    assert c.mix_spec == dict(mixup_alpha=0.2, cutmix_alpha=1.0, prob=0.8, switch_prob=0.5, seed=3)
    assert Config(cutmix_alpha=1.0).mix_spec["mixup_alpha"] == 0.0
    monkeypatch.setenv("MPA_MIXUP_ALPHA", "0.4")
    monkeypatch.setenv("MPA_MIX_SWITCH_PROB", "0.25")
    c = Config.from_args([])
    assert c.mixup_alpha == 0.4 and c.mix_switch_prob == 0.25 and c.mix_spec is not None
    assert Config.from_args(["--mixup_alpha", "0"]).mix_spec is None    # flags beat the environment


# ------------------------------------------------------------------------------ loader
def _loader(names, labels, mix, augment=None, batch=6):
    from mpi_pytorch_amd.data.manifest import SyntheticImages
    from mpi_pytorch_amd.engine.trainer import ManifestBatches
    return ManifestBatches(names, labels, batch, (16, 24), CPU, SyntheticImages((40, 36)), False,
                           0, cpad=4, pad=(3, 3, 3, 3), augment=augment, mix=mix)


@pytest.mark.parametrize("augment", [None, dict(kind="rrc", scale_min=0.08, seed=4)])
def test_loader_yields_mixed_labels_and_the_oracles_batch(augment):
    from mpi_pytorch_amd.engine import MixedLabels
    from mpi_pytorch_amd.data.loader import IMAGENET_MEAN, IMAGENET_STD
    names = ["img/%d.jpg" % i for i in range(15)]
    labels = list(np.random.default_rng(0).integers(0, 9, size=15))
    spec = Config(mixup_alpha=0.3, cutmix_alpha=1.0, seed=4).mix_spec
    ld = _loader(names, labels, spec, augment)
    plain = list(_loader(names, labels, None, augment).epoch(2))
    got = list(ld.epoch(2))
    assert len(got) == 3 and got[-1][0].shape[0] == 3               # a short last batch too
    ids = sample_ids(names)
    for i, ((x, y), (xp, yp)) in enumerate(zip(got, plain)):
        idx = np.arange(i * 6, min(15, i * 6 + 6))
        assert isinstance(y, MixedLabels) and torch.is_tensor(yp) and not isinstance(yp, tuple)
        mix, lam = sample_mix(ids[idx], 2, 4, (16, 24), 0.3, 1.0)
        assert torch.equal(y.labels, yp) and y.labels.dtype == torch.int64
        assert torch.equal(y.labels2, yp[torch.from_numpy(mix[:, 0].astype(np.int64))])
        assert torch.equal(y.lam, torch.from_numpy(label_weights(mix, lam, (16, 24))))
        assert y.lam.dtype == torch.float32
        imgs = torch.from_numpy(ld.source.load([names[j] for j in idx]))
        want = ref.preprocess(imgs, 16, 24, IMAGENET_MEAN, IMAGENET_STD, 0, 4, torch.float32,
                              (3, 3, 3, 3), boxes=ld._boxes(idx, 2, (40, 36)), mix=mix, lam=lam)
        assert x.dtype == torch.float32 and torch.equal(x, want)
        assert not torch.equal(x, xp)
    # mix=None: what the loader yields without the feature
    for (xp, yp), idx in zip(plain, (np.arange(0, 6), np.arange(6, 12), np.arange(12, 15))):
        imgs = torch.from_numpy(ld.source.load([names[j] for j in idx]))
        want = ref.preprocess(imgs, 16, 24, IMAGENET_MEAN, IMAGENET_STD, 0, 4, torch.float32,
                              (3, 3, 3, 3), boxes=ld._boxes(idx, 2, (40, 36)))
        assert torch.equal(xp, want) and torch.equal(yp, torch.tensor(labels)[idx])
    with pytest.raises(ValueError):
        from mpi_pytorch_amd.data.manifest import SyntheticImages
        from mpi_pytorch_amd.engine.trainer import ManifestBatches
        ManifestBatches(names, labels, 6, (16, 24), CPU, SyntheticImages((40, 36)), False, 0,
                        mode=1, mix=spec)


# -------------------------------------------------------------------------------- step
def test_step_gradient_is_the_lam_weighted_sum_of_two_cross_entropies():
    from mpi_pytorch_amd.engine import MixedLabels, build_training
    from mpi_pytorch_amd.parallel import World
    torch.manual_seed(0)
    model, opt, step, _ = build_training("resnet18", 10, CPU, World(), 1e-3, label_smoothing=0.1)
    x = torch.randn(4, 32, 32, 3)
    y, y2 = torch.randint(0, 10, (4,)), torch.randint(0, 10, (4,))
    lam = torch.tensor([0.3, 1.0, 0.0, 0.65])
    # the same loss written out with plain torch, on the same parameters
    model._mpa_arena.zero_grad()
    out = model(x)
    ce = lambda t: F.cross_entropy(out.float(), t, reduction="none", label_smoothing=0.1)
    want_loss = (lam * ce(y) + (1.0 - lam) * ce(y2)).mean()
    want_loss.backward()
    want = model._mpa_arena.grad.clone()
    assert float(want.abs().sum()) > 0
    seen = []
    real = opt.step
    opt.step = lambda: seen.append(model._mpa_arena.grad.clone())   # gradients only
    loss = step(x, MixedLabels(y, y2, lam))
    opt.step = real
    assert abs(float(loss) - float(want_loss)) <= 1e-5 * abs(float(want_loss))
    # rtol 1e-5 elementwise, with an absolute floor of the same 1e-5 relative to the largest
    # gradient: both sides are fp32 sums over the batch and the feature maps whose terms
    # cancel, so an element's rounding error scales with the terms, not with the element
    atol = 1e-5 * float(want.abs().max())
    assert torch.allclose(seen[0], want, rtol=1e-5, atol=atol)
    plain = []
    opt.step = lambda: plain.append(model._mpa_arena.grad.clone())
    step(x, y)
    opt.step = real
    assert not torch.allclose(plain[0], want, rtol=1e-3, atol=100 * atol)   # (and the labels matter)


# ------------------------------------------------------------------------------ driver
def _shape_of(line):
    return re.sub(r"[-+]?\d+(\.\d+)?(e[-+]?\d+)?", "#", line)


def test_training_driver_mixes_logs_the_configuration_and_keeps_every_other_line(tmp_path):
    from mpi_pytorch_amd.engine.trainer import run_training
    texts, hist = {}, {}
    extra = dict(mixup_alpha=0.2, cutmix_alpha=1.0, augment="rrc", label_smoothing=0.1)
    for name, kw in (("plain", {}), ("mixed", extra)):
        _reset_world()
        d = tmp_path / name
        d.mkdir()
        cfg = Config(synthetic_images=32, image_size=32, NUM_EPOCHS=1, BATCH_SIZE=16,
                     NUM_CLASSES=50, CHECKPOINT_DIR=str(d) + "/ck/", device="cpu", max_steps=2,
                     log_file=str(d / "training.log"), metrics_jsonl=str(d / "m.jsonl"), **kw)
        hist[name] = run_training(cfg)["history"]
        texts[name] = (d / "training.log").read_text().splitlines()
    _reset_world()
    assert all(np.isfinite(r["train_loss"]) for r in hist["mixed"])
    rec = json.loads((tmp_path / "mixed" / "m.jsonl").read_text().splitlines()[0])
    assert rec["config"] == dict(mixup_alpha=0.2, cutmix_alpha=1.0, mix_prob=1.0,
                                 mix_switch_prob=0.5)
    plain_rec = json.loads((tmp_path / "plain" / "m.jsonl").read_text().splitlines()[0])
    assert "config" not in plain_rec
    lines = texts["mixed"]
    at = [i for i, s in enumerate(lines) if "_Sample mixing: " in s]
    assert len(at) == 1 and "_Entering training Loop" in lines[at[0] - 1]
    assert lines[at[0]].endswith("_Sample mixing: mixup_alpha 0.2 | cutmix_alpha 1.0 | prob 1.0 "
                                 "| switch_prob 0.5")
    assert not any("mixing" in s for s in texts["plain"])
    rest = lines[:at[0]] + lines[at[0] + 1:]
    assert [_shape_of(s) for s in rest] == [_shape_of(s) for s in texts["plain"]]
