"""Time of the training preprocess launch (mode 0: bilinear resize + normalize -> bf16 NHWC),
plain and with crop boxes (random-resized crop + flip in the same launch).

    python tools/bench_preprocess.py --batch 256 --src 448 448 --out 224 224
    python tools/bench_preprocess.py --batch 2048 --src 224 224 --out 224 224

Times the kernel launch alone (the binding, device-resident images and boxes) with HIP
events: ``--iters`` back-to-back launches per timed window, ``--repeats`` windows after
``--warmup`` launches.  Variants:
  plain       no boxes (the identity-size copy fast path where it applies)
  plain_bilinear  identity sizes only: no boxes with the copy fast path switched off, i.e.
              the bilinear kernel the boxed variants run - their like-for-like baseline
  full_boxes  every box the whole image, flip 0 (same output as plain, through the BOX kernel)
  rrc_boxes   boxes drawn by data/augment.py (scale_min .. 1, ratio 3/4 .. 4/3, flips)
Prints one JSON line per variant: microseconds per launch (median / min / max over the
windows) and the source + output bytes the launch has to move.  A build without box
support (an older checkout) reports the plain variant only."""
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
    for name, boxes in variants:
        kw = {}
        src_bytes = B * H * W * 3
        if boxes is not None:
            kw["box"] = torch.from_numpy(boxes).to(dev)
            src_bytes = int((boxes[:, 2].astype(np.int64) * boxes[:, 3]).sum()) * 3

        def launch():
            return k.preprocess(img, OH, OW, mean, std, 0, a.cpad, pad, None, **kw)

        k.preprocess_set_copy(0 if name == "plain_bilinear" else 1)
        for _ in range(a.warmup):
            launch()
        torch.cuda.synchronize()
        us = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                launch()
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / a.iters)
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
