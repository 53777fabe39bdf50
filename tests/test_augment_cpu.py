"""Random-resized-crop + flip augmentation, host side: the oracle (``ref.preprocess`` with
``boxes``), the parameter sampler (``data/augment.py``), its determinism, the wiring through
``ManifestBatches`` and the ``Config`` fields."""
import numpy as np
import pytest
import torch

from mpi_pytorch_amd.config import Config
from mpi_pytorch_amd.data.augment import fallback_box, sample_boxes, sample_ids
from mpi_pytorch_amd.data.manifest import SyntheticImages
from mpi_pytorch_amd.ops import functional as Fn
from mpi_pytorch_amd.ops import ref

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
RATIO = (3.0 / 4.0, 4.0 / 3.0)
N = 4096


# ------------------------------------------------------------------------------ oracle
@pytest.mark.parametrize("cpad,pad", [(3, None), (4, (3, 2, 1, 0))])
def test_oracle_boxes_are_slice_resize_flip(cpad, pad):
    g = torch.Generator().manual_seed(5)
    img = torch.randint(0, 256, (6, 20, 31, 3), generator=g, dtype=torch.uint8)
    boxes = np.array([[4, 7, 1, 1, 0],        # 1x1
                      [0, 0, 20, 31, 1],      # the full image, mirrored
                      [11, 19, 9, 12, 1],     # touching the bottom-right corner
                      [11, 19, 9, 12, 0],
                      [0, 3, 5, 28, 1],
                      [3, 0, 17, 2, 0]])
    out = ref.preprocess(img, 16, 13, MEAN, STD, 0, cpad, torch.float32, pad, boxes=boxes)
    for b, (y0, x0, h, w, flip) in enumerate(boxes.tolist()):
        exp = ref.preprocess(img[b:b + 1, y0:y0 + h, x0:x0 + w].contiguous(), 16, 13, MEAN, STD,
                             0, cpad, torch.float32)
        if flip:
            exp = torch.flip(exp, dims=(2,))
        t, bo, l, r = pad or (0, 0, 0, 0)
        assert torch.equal(out[b:b + 1, t:t + 16, l:l + 13], exp)
        border = out[b].clone()
        border[t:t + 16, l:l + 13] = 0
        assert not border.any() and not out[b, ..., 3:].any()
    assert out.shape == (6, 16 + (pad[0] + pad[1] if pad else 0),
                         13 + (pad[2] + pad[3] if pad else 0), cpad)
    # through the op layer (the CPU training path)
    via = Fn.preprocess(img, (16, 13), MEAN, STD, 0, cpad, out_dtype=torch.float32, pad=pad,
                        boxes=boxes)
    assert torch.equal(via, out)


def test_op_layer_rejects_bad_boxes_cpu():
    img = torch.zeros(2, 12, 10, 3, dtype=torch.uint8)
    ok = [[0, 0, 12, 10, 0], [1, 1, 3, 3, 1]]
    Fn.preprocess(img, (4, 4), MEAN, STD, 0, 3, out_dtype=torch.float32, boxes=ok)
    for bad in ([[0, 0, 13, 10, 0], ok[1]], [[0, 1, 12, 10, 0], ok[1]], [ok[0], [1, 1, 0, 3, 0]],
                [ok[0], [1, 1, 3, 3, 2]], [ok[0], [-1, 1, 3, 3, 0]], [ok[0]]):
        with pytest.raises(ValueError):
            Fn.preprocess(img, (4, 4), MEAN, STD, 0, 3, out_dtype=torch.float32, boxes=bad)
    with pytest.raises(ValueError):   # inside the slot but outside the image's extent
        Fn.preprocess(img, (4, 4), MEAN, STD, 0, 3, out_dtype=torch.float32,
                      extents=[[12, 10], [3, 3]], boxes=ok)
    with pytest.raises(ValueError):
        Fn.preprocess(img, (4, 4), MEAN, STD, 2, 3, out_dtype=torch.float32, boxes=ok)


# ----------------------------------------------------------------------------- sampler
def _mixed_extents(n):
    base = np.array([[300, 200], [97, 311], [8, 9], [224, 224], [640, 60], [31, 500], [9, 8],
                     [1, 1], [3, 40]])
    return base[np.arange(n) % len(base)]


def _ids(n):
    return sample_ids(["synthetic/{:08d}.jpg".format(i) for i in range(n)])


@pytest.mark.parametrize("scale_min", [0.08, 0.35])
def test_sampler_invariants(scale_min):
    ext = _mixed_extents(N)
    bx = sample_boxes(_ids(N), ext, epoch=3, seed=11, scale=(scale_min, 1.0)).astype(np.int64)
    assert bx.shape == (N, 5) and set(np.unique(bx[:, 4])) <= {0, 1}
    y0, x0, h, w = bx[:, 0], bx[:, 1], bx[:, 2], bx[:, 3]
    H, W = ext[:, 0], ext[:, 1]
    assert (h >= 1).all() and (w >= 1).all() and (y0 >= 0).all() and (x0 >= 0).all()
    assert (y0 + h <= H).all() and (x0 + w <= W).all()
    # fallback rows are exactly the centred crop of the clamped ratio
    fb = np.array([fallback_box(int(a), int(b), RATIO) for a, b in ext])
    is_fb = (bx[:, :4] == fb).all(axis=1)
    assert (2 * fb[:, 0] + fb[:, 2] - H).__abs__().max() <= 1      # centred
    assert (2 * fb[:, 1] + fb[:, 3] - W).__abs__().max() <= 1
    # every other row: h, w are roundings of a (h', w') with h' w' in [scale_min, 1] x area
    # and w' / h' in ratio; |h - h'|, |w - w'| <= 1/2
    area = (H * W).astype(np.float64)
    acc = ~is_fb
    assert (h * w <= area).all()
    assert ((h + 0.5) * (w + 0.5) >= scale_min * area)[acc].all()
    assert ((w + 0.5) / np.maximum(h - 0.5, 1e-9) >= RATIO[0])[acc].all()
    assert ((w - 0.5) / (h + 0.5) <= RATIO[1])[acc].all()
    # near-square images accept a try with probability > 0.4 (0.8 for a square one at
    # scale_min 0.35), so ten tries fall back in < 1 % of draws: the fallback is the exception
    near = (np.maximum(H, W) * 2 <= np.minimum(H, W) * 3) & (area > 1)
    assert near.sum() > 1000 and is_fb[near].mean() < 0.1
    flips = bx[:, 4].mean()
    assert abs(flips - 0.5) <= 0.05, flips    # > 6 sigma for a fair coin at 4096
    # positions are spread: not every accepted box sits at the origin
    assert (y0[acc] > 0).any() and (x0[acc] > 0).any()


def test_flip_only_boxes_are_full_extent():
    ext = _mixed_extents(N)
    bx = sample_boxes(_ids(N), ext, epoch=0, seed=1, crop=False)
    assert (bx[:, :2] == 0).all() and (bx[:, 2:4] == ext).all()
    assert abs(bx[:, 4].mean() - 0.5) <= 0.05
    assert (sample_boxes(_ids(64), ext[:64], 0, 1, crop=False, flip_p=0.0)[:, 4] == 0).all()


def test_sampler_determinism():
    ext = _mixed_extents(N)
    ids = _ids(N)
    a = sample_boxes(ids, ext, epoch=2, seed=7)
    assert np.array_equal(a, sample_boxes(ids, ext, epoch=2, seed=7))
    # any sub-batch, in any order, gives the same rows
    perm = np.random.default_rng(0).permutation(N)[:301]
    assert np.array_equal(sample_boxes(ids[perm], ext[perm], 2, 7), a[perm])
    assert np.array_equal(sample_boxes(ids[5:6], ext[5:6], 2, 7), a[5:6])
    # another epoch or seed redraws.  Images no more elongated than 2:1 are counted: a very
    # elongated one (640x60) mostly falls back to its one centre crop, whatever the draw,
    # and then only its flip can change
    ok = np.maximum(ext[:, 0], ext[:, 1]) <= 2 * np.minimum(ext[:, 0], ext[:, 1])
    ok &= (ext[:, 0] * ext[:, 1]) > 1
    assert ok.sum() > 1500
    for other in (sample_boxes(ids, ext, 3, 7), sample_boxes(ids, ext, 2, 8)):
        changed = (other != a).any(axis=1)[ok].mean()
        assert changed >= 0.9, changed


# ---------------------------------------------------------------------- ManifestBatches
def _loader(names, labels, batch, augment, shuffle=True, seed=0):
    from mpi_pytorch_amd.engine.trainer import ManifestBatches
    return ManifestBatches(names, labels, batch, (16, 16), torch.device("cpu"),
                           SyntheticImages((40, 36)), shuffle, seed, augment=augment)


def _rows(loader, epoch):
    """file name -> that sample's tensor, over one epoch (the loader's own order)."""
    order = np.arange(len(loader.names))
    if loader.shuffle:
        np.random.default_rng(loader.seed * 7919 + epoch).shuffle(order)
    xs = torch.cat([x for x, _y in loader.epoch(epoch)], 0)
    assert xs.shape[0] == len(order)
    return {loader.names[i]: xs[k] for k, i in enumerate(order)}


def test_manifest_batches_shard_invariance_and_validation_untouched():
    names = ["synthetic/{:08d}.jpg".format(i) for i in range(23)]
    labels = list(range(23))
    aug = Config(augment="rrc", seed=4).augment_spec
    assert aug == dict(kind="rrc", scale_min=0.08, seed=4)
    whole = _rows(_loader(names, labels, 8, aug, seed=4), 1)
    plain = _rows(_loader(names, labels, 8, None, seed=4), 1)
    assert sum(not torch.equal(whole[n], plain[n]) for n in names) >= 20   # it augments
    # a 2-way shard (other batch size, other shuffle seeds): same file -> same tensor
    for r, sl in enumerate((slice(0, 12), slice(12, 23))):
        part = _rows(_loader(names[sl], labels[sl], 5, aug, seed=4 + r), 1)
        assert set(part) == set(names[sl])
        for n, x in part.items():
            assert torch.equal(x, whole[n]), n
    # another epoch: other crops for the same files
    nxt = _rows(_loader(names, labels, 8, aug, seed=4), 2)
    assert sum(not torch.equal(whole[n], nxt[n]) for n in names) >= 20
    # flip-only: every image is the plain one or its mirror
    fl = _rows(_loader(names, labels, 8, dict(kind="flip", seed=4)), 1)
    kinds = [torch.equal(fl[n], plain[n]) or torch.equal(fl[n], torch.flip(plain[n], (1,)))
             for n in names]
    assert all(kinds) and any(not torch.equal(fl[n], plain[n]) for n in names)
    with pytest.raises(ValueError):
        _loader(names, labels, 8, dict(kind="mixup"))


def test_run_training_augments_train_loader_only(tmp_path, monkeypatch):
    """The driver hands ``augment`` to the training loader and never to the validation
    loader, whose batches are identical with and without it."""
    import mpi_pytorch_amd.parallel.dist as D
    from mpi_pytorch_amd.engine import trainer
    made = []
    real = trainer.ManifestBatches

    class Spy(real):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    monkeypatch.setattr(trainer, "ManifestBatches", Spy)
    val = {}
    for aug in ("none", "rrc"):
        D._WORLD = None
        made.clear()
        cfg = Config(synthetic_images=16, image_size=32, NUM_EPOCHS=2, BATCH_SIZE=8,
                     NUM_CLASSES=10, device="cpu", augment=aug,
                     CHECKPOINT_DIR=str(tmp_path) + "/ck_%s/" % aug,
                     log_file=str(tmp_path / ("l_" + aug)))
        out = trainer.run_training(cfg)
        assert all(np.isfinite(r["train_loss"]) for r in out["history"])
        train, vl = made
        assert vl.augment is None and not vl.shuffle
        assert (train.augment is None) == (aug == "none")
        val[aug] = torch.cat([x for x, _y in vl.epoch(0)], 0)
    D._WORLD = None
    assert torch.equal(val["none"], val["rrc"])


# ------------------------------------------------------------------------------ config
def test_config_augment_fields(monkeypatch):
    c = Config()
    assert c.augment == "none" and c.aug_scale_min == 0.08 and c.augment_spec is None
    c = Config.from_args(["--augment", "rrc", "--aug-scale-min", "0.25", "--seed", "3"])
    assert c.augment_spec == dict(kind="rrc", scale_min=0.25, seed=3)
    monkeypatch.setenv("MPA_AUGMENT", "flip")
    monkeypatch.setenv("MPA_AUG_SCALE_MIN", "0.5")
    c = Config.from_env()
    assert c.augment == "flip" and c.aug_scale_min == 0.5
    assert Config.from_args(["--augment", "rrc"]).augment == "rrc"   # flags beat the environment
    monkeypatch.delenv("MPA_AUGMENT")
    monkeypatch.delenv("MPA_AUG_SCALE_MIN")
    for kw in (dict(augment="mixup"), dict(aug_scale_min=0.0), dict(aug_scale_min=1.5)):
        with pytest.raises(ValueError):
            Config(**kw)
    assert Config(aug_scale_min=1.0).aug_scale_min == 1.0
