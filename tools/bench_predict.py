"""Timing of the prediction path.

kernel:   topk_predict (k = 1, 5, 16) at [rows, 64,500] bf16 logits with row stride 64,512,
          against argmax_correct (one pass over the same bytes) and ATen softmax(float) +
          topk on the same logits: each warmed, then alternating repetitions of medians, so
          every kernel's own spread stands next to the differences.
pipeline: the evaluation pipeline (ResNet-18 at 224^2, 2 lanes, 64,500 classes, synthetic
          images) with --predictions_csv / --predict_topk 5 against the same run without
          them, in alternating pairs: img/s from the driver's _Throughput line.
Results: docs/NOTES.md "Predictions".

    python tools/bench_predict.py kernel [rows] [iters] [reps]
    python tools/bench_predict.py pipeline [images] [pairs] [out_dir]
"""
import os
import re
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from mpi_pytorch_amd.ops import _ext


def median_us(fn, iters):
    """Median of ``iters`` single-call device times, after a warm-up."""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(iters)]
    for s, e in ev:
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    return statistics.median(s.elapsed_time(e) for s, e in ev) * 1e3


def kernel(rows=256, iters=200, reps=5):
    C = _ext.ext()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    full = (torch.randn(rows, 64512, device=dev) * 3).to(torch.bfloat16)
    logits = full[:, :64500]
    labels = torch.randint(0, 64500, (rows,), device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    outs = {k: (torch.empty(rows, k, dtype=torch.int32, device=dev),
                torch.empty(rows, k, dtype=torch.float32, device=dev)) for k in (1, 5, 16)}
    group = [("argmax_correct", lambda: C.argmax_correct(logits, labels, cnt))]
    for k in (1, 5, 16):
        group.append(("topk_predict k=%d" % k,
                      lambda k=k: C.topk_predict(logits, k, *outs[k])))
        group.append(("softmax+topk k=%d" % k,
                      lambda k=k: torch.softmax(logits.float(), 1).topk(k, 1)))
    times = {name: [] for name, _ in group}
    for _ in range(reps):
        for name, fn in group:
            times[name].append(median_us(fn, iters))
    print("[%d, 64500] logits (ld 64512), %d alternating repetitions of a median over %d "
          "calls: us (min .. max)" % (rows, reps, iters))
    for name, _ in group:
        t = times[name]
        print("%-18s %s  (%.1f .. %.1f)" % (name, " ".join("%7.1f" % v for v in t),
                                            min(t), max(t)))


def pipeline(images=131072, pairs=4, out_dir=None):  # (16,384 images: 0.3 s, too short to read)
    from mpi_pytorch_amd.config import Config
    from mpi_pytorch_amd.engine.eval_pipeline import run_pipeline
    out_dir = out_dir or tempfile.mkdtemp(prefix="bench_predict_")
    os.makedirs(out_dir, exist_ok=True)
    rates = {"off": [], "on": []}
    walls = {"off": [], "on": []}  # the whole call: model load, the run, gather and file

    def one(tag, i, **kw):
        log = os.path.join(out_dir, "%s_%d.log" % (tag, i))
        t0 = time.perf_counter()
        run_pipeline(Config(MODEL_NAME="resnet18", image_size=224, eval_lanes=2,
                            synthetic_images=images, device="cuda", log_file=log,
                            CHECKPOINT_DIR=os.path.join(out_dir, "ck") + "/", **kw))
        walls.setdefault(tag, []).append(time.perf_counter() - t0)
        return float(re.findall(r"_Throughput: ([\d.]+) img/s", open(log).read())[-1])

    one("warm", 0)  # code objects, allocator, pinned slots
    for i in range(pairs):
        rates["off"].append(one("off", i))
        rates["on"].append(one("on", i, predict_topk=5,
                               predictions_csv=os.path.join(out_dir, "pred_%d.csv" % i)))
    print("ResNet-18 224^2, 2 lanes, %d images, %d alternating pairs: img/s" % (images, pairs))
    for tag in ("off", "on"):
        t = rates[tag]
        print("predictions %-3s %s  (%.0f .. %.0f, median %.0f)" % (
            tag, " ".join("%8.0f" % v for v in t), min(t), max(t), statistics.median(t)))
    for tag in ("off", "on"):
        print("whole call  %-3s %s  s" % (tag, " ".join("%8.2f" % v for v in walls[tag])))


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    args = sys.argv[2:]
    if what == "kernel":
        kernel(*(int(a) for a in args[:3]))
    else:
        pipeline(*(int(a) for a in args[:2]), *args[2:3])
