"""Crop boxes and flips in the bilinear preprocess launch (``Fn.preprocess(boxes=)``,
``csrc/kernels/preprocess.hip``) on the GPU.

The defining property: the interpolation arithmetic is box-relative, so image b of a boxed
launch is BITWISE the plain launch of the contiguous crop ``img[b, y0:y0+h, x0:x0+w]``, and
a flipped image is bitwise the mirror of the unflipped one.  Shapes are the smallest that
reach every path: slot widths 64 / 20 / 21 (16-B, 4-B and byte staging loads), a
1400-wide slot (taps from global memory), an odd output width, an upscale, the three output
layouts, and one batch whose work items exceed the grid (the stride loop)."""
import numpy as np
import pytest
import torch

from mpi_pytorch_amd.config import Config
from mpi_pytorch_amd.data.augment import sample_boxes
from mpi_pytorch_amd.ops import functional as Fn
from mpi_pytorch_amd.ops import ref

pytestmark = pytest.mark.gpu
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

SLOTS = [(24, 64), (17, 20), (19, 21), (12, 1400)]     # VEC 16, VEC 4, VEC 1, unstaged
DSTS = [(16, 16), (37, 91), (48, 80)]                  # (48, 80): an upscale of the small slots
LAYOUTS = [(3, None), (8, None), (4, (3, 3, 3, 3))]
CASES = [(s, d, l) for s in SLOTS for d in DSTS for l in LAYOUTS]


def _boxes_for(H, W):
    """Boxes (flip 0) of an [H][W] slot: the full slot, 1x1, flush with each edge and
    corner, one-pixel rows / columns, and x0 with x0*3 % 16 != 0 and x0*3 % 4 != 0."""
    return np.array([[0, 0, H, W, 0], [H // 2, W // 3, 1, 1, 0], [0, 0, H - 3, W - 5, 0],
                     [3, 5, H - 3, W - 5, 0], [0, 7, H, W - 7, 0], [H - 1, 0, 1, W, 0],
                     [0, W - 1, H, 1, 0], [2, 1, H - 4, W - 2, 0], [1, 3, 5, 7, 0],
                     [H - 2, W - 9, 2, 9, 0]], dtype=np.int32)


def _interior(x, dst, pad):
    t, _b, l, _r = pad or (0, 0, 0, 0)
    return x[:, t:t + dst[0], l:l + dst[1], :3]


def _crops_alone(img, boxes, dst, cpad, pad, gpu):
    """Every image's crop as a contiguous batch of one through the un-boxed kernel."""
    outs = []
    for b, (y0, x0, h, w, _f) in enumerate(boxes.tolist()):
        crop = img[b:b + 1, y0:y0 + h, x0:x0 + w].contiguous()
        outs.append(Fn.preprocess(crop.to(gpu), dst, MEAN, STD, 0, cpad, pad=pad))
    return torch.cat(outs, 0)


_CACHE = {}


def _case(case, gpu):
    """(img u8 host, boxes, boxed output with flip 0) of a case, computed once."""
    if case not in _CACHE:
        (H, W), dst, (cpad, pad) = case
        g = torch.Generator().manual_seed(H * 1000 + W + dst[1])
        boxes = _boxes_for(H, W)
        img = torch.randint(0, 256, (len(boxes), H, W, 3), generator=g, dtype=torch.uint8)
        out = Fn.preprocess(img.to(gpu), dst, MEAN, STD, 0, cpad, pad=pad, boxes=boxes)
        _CACHE[case] = (img, boxes, out)
    return _CACHE[case]


@pytest.mark.parametrize("case", CASES, ids=str)
def test_box_equals_unboxed_kernel_on_the_crop(gpu, case):
    (H, W), dst, (cpad, pad) = case
    img, boxes, out = _case(case, gpu)
    exp = _crops_alone(img, boxes, dst, cpad, pad, gpu)
    assert out.dtype == torch.bfloat16 and out.shape == exp.shape
    assert torch.equal(out, exp)


@pytest.mark.parametrize("case", CASES, ids=str)
def test_flip_is_mirror_of_unflipped_and_border_is_zero(gpu, case):
    (H, W), dst, (cpad, pad) = case
    img, boxes, out = _case(case, gpu)
    fb = boxes.copy()
    fb[::2, 4] = 1                                   # every other image mirrored
    outf = Fn.preprocess(img.to(gpu), dst, MEAN, STD, 0, cpad, pad=pad, boxes=fb)
    exp = _interior(out, dst, pad).clone()
    exp[::2] = torch.flip(exp[::2], dims=(2,))
    assert torch.equal(_interior(outf, dst, pad), exp)
    rest = outf.clone()                              # canvas border + padding channels
    _interior(rest, dst, pad).zero_()
    assert not rest.any()


@pytest.mark.parametrize("case", CASES[::4], ids=str)
def test_pixels_outside_the_box_do_not_matter(gpu, case):
    (H, W), dst, (cpad, pad) = case
    img, boxes, out = _case(case, gpu)
    ext = np.array([[min(H, y0 + h + b % 2), min(W, x0 + w + b % 3)]
                    for b, (y0, x0, h, w, _f) in enumerate(boxes.tolist())])
    oute = Fn.preprocess(img.to(gpu), dst, MEAN, STD, 0, cpad, pad=pad, extents=ext, boxes=boxes)
    assert torch.equal(oute, out)                    # the extent only bounds the box
    other = 255 - img                                # every pixel differs
    for b, (y0, x0, h, w, _f) in enumerate(boxes.tolist()):
        other[b, y0:y0 + h, x0:x0 + w] = img[b, y0:y0 + h, x0:x0 + w]
    for e in (None, ext):                            # inside and outside the extents
        out2 = Fn.preprocess(other.to(gpu), dst, MEAN, STD, 0, cpad, pad=pad, extents=e,
                             boxes=boxes)
        assert torch.equal(out2, out)


@pytest.mark.parametrize("case", CASES, ids=str)
def test_boxed_kernel_against_oracle(gpu, case):
    (H, W), dst, (cpad, pad) = case
    img, boxes, _out = _case(case, gpu)
    fb = boxes.copy()
    fb[1::2, 4] = 1
    out = Fn.preprocess(img.to(gpu), dst, MEAN, STD, 0, cpad, pad=pad, boxes=fb)
    exp = ref.preprocess(img, dst[0], dst[1], MEAN, STD, 0, cpad, torch.float32, pad, boxes=fb)
    assert out.shape == exp.shape
    err = float((out.float().cpu() - exp).abs().max())
    print("max abs err", err)
    assert err < 0.05


@pytest.mark.parametrize("slot,dst,cpad,pad", [((24, 64), (16, 16), 8, None),
                                               ((19, 21), (37, 91), 4, (3, 3, 3, 3)),
                                               # identity size: the no-box call takes the
                                               # copy fast path (cpad 4) / the bilinear kernel
                                               ((24, 64), (24, 64), 4, (3, 3, 3, 3)),
                                               ((24, 64), (24, 64), 3, None)])
def test_full_extent_boxes_change_nothing(gpu, slot, dst, cpad, pad):
    H, W = slot
    g = torch.Generator().manual_seed(H + W)
    img = torch.randint(0, 256, (5, H, W, 3), generator=g, dtype=torch.uint8).to(gpu)
    full = np.tile(np.array([[0, 0, H, W, 0]], dtype=np.int32), (5, 1))
    plain = Fn.preprocess(img, dst, MEAN, STD, 0, cpad, pad=pad)
    assert torch.equal(Fn.preprocess(img, dst, MEAN, STD, 0, cpad, pad=pad, boxes=full), plain)
    ext = np.array([[H, W], [H - 1, W], [H, W - 3], [5, 7], [H - 2, W - 1]])
    fe = np.concatenate([np.zeros((5, 2), np.int32), ext.astype(np.int32),
                         np.zeros((5, 1), np.int32)], 1)
    pe = Fn.preprocess(img, dst, MEAN, STD, 0, cpad, pad=pad, extents=ext)
    assert torch.equal(Fn.preprocess(img, dst, MEAN, STD, 0, cpad, pad=pad, extents=ext,
                                     boxes=fe), pe)


def test_more_items_than_blocks(gpu):
    """300 images x 9 row groups = 2700 work items on the 2048-block grid: the stride loop
    re-stages LDS per item with another image's box and slack."""
    B, dst, pad = 300, (64, 64), (3, 3, 3, 3)
    g = torch.Generator().manual_seed(300)
    img = torch.randint(0, 256, (B, 24, 24, 3), generator=g, dtype=torch.uint8)
    boxes = sample_boxes(np.arange(B), np.tile([[24, 24]], (B, 1)), epoch=0, seed=9)
    assert 0 < boxes[:, 4].sum() < B and len(np.unique(boxes[:, 1] % 4)) == 4
    out = Fn.preprocess(img.to(gpu), dst, MEAN, STD, 0, 4, pad=pad, boxes=boxes)
    exp = _crops_alone(img, boxes, dst, 4, pad, gpu)
    fl = torch.from_numpy(boxes[:, 4] == 1).to(gpu)
    inner = _interior(exp, dst, pad)
    inner[fl] = torch.flip(inner[fl], dims=(2,))
    assert torch.equal(out, exp)


def test_bad_boxes_are_rejected_on_the_host(gpu):
    img = torch.zeros(2, 12, 10, 3, dtype=torch.uint8, device=gpu)
    ok = [[0, 0, 12, 10, 0], [1, 1, 3, 3, 1]]
    for bad in ([[0, 0, 13, 10, 0], ok[1]], [[0, 1, 12, 10, 0], ok[1]], [[1, 0, 12, 10, 0], ok[1]],
                [ok[0], [1, 1, 0, 3, 0]], [ok[0], [1, 1, 3, 0, 0]], [ok[0], [1, 1, 3, 3, 2]],
                [ok[0], [-1, 1, 3, 3, 0]], [ok[0]], ok + ok[:1]):
        with pytest.raises(ValueError):
            Fn.preprocess(img, (4, 4), MEAN, STD, 0, 3, boxes=bad)
    with pytest.raises(ValueError):   # inside the slot, outside the image's extent
        Fn.preprocess(img, (4, 4), MEAN, STD, 0, 3, extents=[[12, 10], [3, 3]], boxes=ok)
    for mode in (1, 2):
        with pytest.raises(ValueError):
            Fn.preprocess(img, (4, 4), MEAN, STD, mode, 3, boxes=ok)
    # the binding's own argument checks (shape, dtype, device, mode)
    from mpi_pytorch_amd.ops import _ext
    k = _ext.ext()
    good = torch.tensor(ok, dtype=torch.int32, device=gpu)
    k.preprocess(img, 4, 4, list(MEAN), list(STD), 0, 3, [], None, box=good)
    for box, mode in ((good.long(), 0), (good.cpu(), 0), (good[:1], 0), (good[:, :4], 0),
                      (good, 2)):
        with pytest.raises(RuntimeError):
            k.preprocess(img, 4, 4, list(MEAN), list(STD), mode, 3, [], None, box=box)


class _HostSource:
    """A non-synthetic image source: ``load`` returns host arrays (uniform batch) or a list
    of arrays of different sizes (the decoded-JPEG path)."""

    def __init__(self, ragged):
        self.ragged = ragged

    def load(self, names):
        out = []
        for n in names:
            k = int(n)
            rng = np.random.default_rng(k)
            hw = (30 + 3 * (k % 4), 41 - 2 * (k % 3)) if self.ragged else (30, 41)
            out.append(rng.integers(0, 256, hw + (3,), dtype=np.uint8))
        return out if self.ragged else np.stack(out)


@pytest.mark.parametrize("ragged", [False, True])
def test_manifest_batches_host_image_paths(gpu, ragged):
    """The uniform-batch and padded-batch paths of the loader carry the boxes too: GPU
    batches match the CPU loader's (the oracle) for the same files."""
    from mpi_pytorch_amd.engine.trainer import ManifestBatches
    names = [str(i) for i in range(11)]
    aug = dict(kind="rrc", scale_min=0.08, seed=2)
    mk = lambda dev, a: ManifestBatches(names, [0] * 11, 4, (16, 16), dev, _HostSource(ragged),
                                        False, augment=a)
    on_gpu = torch.cat([x for x, _y in mk(gpu, aug).epoch(1)], 0)
    on_cpu = torch.cat([x for x, _y in mk(torch.device("cpu"), aug).epoch(1)], 0)
    plain = torch.cat([x for x, _y in mk(gpu, None).epoch(1)], 0)
    assert on_gpu.shape == on_cpu.shape == plain.shape
    assert float((on_gpu.float().cpu() - on_cpu).abs().max()) < 0.05
    assert float((on_gpu.float() - plain.float()).abs().max()) > 0.5   # it did augment


def test_training_with_rrc_end_to_end(gpu, tmp_path, monkeypatch):
    import mpi_pytorch_amd.parallel.dist as D
    from mpi_pytorch_amd.engine import trainer
    made = []
    real = trainer.ManifestBatches

    class Spy(real):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    monkeypatch.setattr(trainer, "ManifestBatches", Spy)
    D._WORLD = None
    cfg = Config(synthetic_images=32, image_size=32, NUM_EPOCHS=2, BATCH_SIZE=16, NUM_CLASSES=10,
                 VALIDATE=False, device="cuda", augment="rrc", watchdog_s=0,
                 CHECKPOINT_DIR=str(tmp_path) + "/ck/", log_file=str(tmp_path / "training.log"))
    out = trainer.run_training(cfg)
    D._WORLD = None
    losses = [r["train_loss"] for r in out["history"]]
    assert len(losses) == 2 and all(np.isfinite(v) for v in losses), losses
    (train,) = made
    assert train.augment == dict(kind="rrc", scale_min=0.08, seed=0)
    train.shuffle = False                            # same files at the same rows
    e0 = torch.cat([x for x, _y in train.epoch(0)], 0)
    e1 = torch.cat([x for x, _y in train.epoch(1)], 0)
    assert e0.shape == e1.shape and e0.shape[0] == 32
    differ = (e0 != e1).flatten(1).any(dim=1)
    assert int(differ.sum()) >= 29                   # >= 90 % of the files got another crop
    assert torch.equal(e0, torch.cat([x for x, _y in train.epoch(0)], 0))   # and epoch 0 repeats
