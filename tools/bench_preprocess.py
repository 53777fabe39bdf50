"""Time of the training preprocess launch (mode 0: bilinear resize + normalize -> bf16 NHWC),
plain, with crop boxes (random-resized crop + flip in the same launch) and mixed (Mixup /
CutMix in the same launch).

    python tools/bench_preprocess.py --batch 256 --src 448 448 --out 224 224
    python tools/bench_preprocess.py --batch 2048 --src 224 224 --out 224 224

Times the kernel launch alone (the binding, device-resident images and boxes) with HIP
events: ``--iters`` back-to-back launches per timed window, ``--repeats`` windows after
``--warmup`` launches; every variant is warmed first and the windows then alternate between
the variants, so all of them see the same state of the device.  Variants:
  plain       no boxes (the identity-size copy fast path where it applies)
  plain_bilinear  identity sizes only: no boxes with the copy fast path switched off, i.e.
              the bilinear kernel the boxed variants run - their like-for-like baseline
  full_boxes  every box the whole image, flip 0 (same output as plain, through the BOX kernel)
  rrc_boxes   boxes drawn by data/augment.py (scale_min .. 1, ratio 3/4 .. 4/3, flips)
  mixup       rrc_boxes + a Mixup row per image (partner = the next image, lam ~ Beta(.2, .2)):
              every output pixel reads two source images
  cutmix      rrc_boxes + a CutMix row per image (alpha 1): the partner is read only by the
              row groups its rectangle crosses
Prints one JSON line per variant: microseconds per launch (median / min / max over the
windows) and the source + output bytes the launch has to move.  A build without box
support (an older checkout) reports the plain variant only, one without mixing no mixed rows."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from mpi_pytorch_amd.data.loader import IMAGENET_MEAN, IMAGENET_STD
from mpi_pytorch_amd.ops import _ext

try:
    from mpi_pytorch_amd.data.augment import sample_boxes
except ImportError:  # a build from before the augmentation
    sample_boxes = None
try:
    from mpi_pytorch_amd.data.augment import sample_mix
except ImportError:  # a build from before the mixing
    sample_mix = None


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--src", type=int, nargs=2, default=(448, 448), metavar=("H", "W"))
    p.add_argument("--out", type=int, nargs=2, default=(224, 224), metavar=("H", "W"))
    p.add_argument("--cpad", type=int, default=4)
    p.add_argument("--pad", type=int, nargs=4, default=(3, 3, 3, 3))
    p.add_argument("--scale-min", type=float, default=0.08)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--repeats", type=int, default=9)
    p.add_argument("--tag", default="")
    a = p.parse_args()
    assert torch.cuda.is_available(), "bench_preprocess needs a GPU"
    k = _ext.ext()
    dev = torch.device("cuda", 0)
    B, (H, W), (OH, OW) = a.batch, a.src, a.out
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).to(dev)
    mean, std, pad = list(IMAGENET_MEAN), list(IMAGENET_STD), list(a.pad)
    out_bytes = B * (OH + pad[0] + pad[1]) * (OW + pad[2] + pad[3]) * a.cpad * 2

    variants = [("plain", None)]
    if (H, W) == (OH, OW):
        variants.append(("plain_bilinear", None))
    if sample_boxes is not None:
        full = np.tile(np.array([[0, 0, H, W, 0]], dtype=np.int32), (B, 1))
        rrc = sample_boxes(np.arange(B), np.tile([[H, W]], (B, 1)), 0, 0,
                           scale=(a.scale_min, 1.0))
        variants += [("full_boxes", full), ("rrc_boxes", rrc)]
        if sample_mix is not None:
            variants += [("mixup", rrc), ("cutmix", rrc)]
    runs = []
    for name, boxes in variants:
        kw = {}
        src_bytes = B * H * W * 3
        if boxes is not None:
            kw["box"] = torch.from_numpy(boxes).to(dev)
            src_bytes = int((boxes[:, 2].astype(np.int64) * boxes[:, 3]).sum()) * 3
        if name in ("mixup", "cutmix"):
            alphas = (0.2, 0.0) if name == "mixup" else (0.0, 1.0)
            mix, lam = sample_mix(np.arange(B), 0, 0, (OH, OW), *alphas)
            kw["mix"] = torch.from_numpy(mix).to(dev)
            kw["lam"] = torch.from_numpy(lam).to(dev)

        def launch(kw=kw):
            return k.preprocess(img, OH, OW, mean, std, 0, a.cpad, pad, None, **kw)

        runs.append((name, launch, src_bytes, []))
        k.preprocess_set_copy(0 if name == "plain_bilinear" else 1)
        for _ in range(a.warmup):
            launch()
    torch.cuda.synchronize()
    for _ in range(a.repeats):
        for name, launch, _src, us in runs:
            k.preprocess_set_copy(0 if name == "plain_bilinear" else 1)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                launch()
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / a.iters)
    k.preprocess_set_copy(1)
    for name, _launch, src_bytes, us in runs:
        med = statistics.median(us)
        print(json.dumps({"metric": "preprocess mode 0 us/launch", "tag": a.tag, "variant": name,
                          "batch": B, "src": [H, W], "out": [OH, OW], "cpad": a.cpad, "pad": pad,
                          "us_median": round(med, 2), "us_min": round(min(us), 2),
                          "us_max": round(max(us), 2), "src_mb": round(src_bytes / 1e6, 2),
                          "out_mb": round(out_bytes / 1e6, 2),
                          "gb_per_s": round((src_bytes + out_bytes) / med / 1e3, 1),
                          "iters": a.iters, "repeats": a.repeats}), flush=True)


if __name__ == "__main__":
    main()
