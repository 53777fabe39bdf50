"""Pipelined inference: read -> resize -> normalize -> predict as HIP-stream stages.

Reference (``/root/reference/evaluation_pipeline.py:44-199``): an MPMD job with one MPI
rank per stage - rank 0 decodes images and sends pickled PIL images (~2 MB each) to rank
1, which resizes (PIL bicubic+antialias, :89) and sends to rank 2, which runs
ToTensor+Normalize (:116-122) and sends 3x128x128 fp32 tensors to one of the predictor
ranks 3..N-1 chosen uniformly at random per image (:178); predictors run batch-1 forward
passes from the checkpoint (:132-159); the per-predictor ``corrects / dataset_size`` are
SUM-reduced to rank 0 (:196) which logs ``Accuracy is ...`` (:199).  Needs >= 4 ranks.

Here, on one MI355X:
  stage 0  read/decode   the native ``BatchRing`` (csrc/runtime): C++ threads copy each
                         manifest row's synthetic image (a texture window,
                         ``SyntheticImages``) into pinned slots, or PIL decode threads write
                         real JPEGs into a slot (each image at its own extent inside the
                         slot pitch); slots come back to the consumer in batch order;
  stage 1  transfer      pinned slot -> HBM copy on a copy stream (event-ordered); the slot
                         returns to the ring once its copy event has completed;
  stage 2  resize+norm   the PIL-exact preprocess kernels (mode 1, bit-exact with PIL's
                         uint8 resize, per-image extents) on a preprocess stream;
  stage 3  predict       ``lanes`` predictor lanes, each a HIP stream running a *batched*
                         eval forward + fused argmax/correct-count; each batch goes to a
                         lane chosen at random (reference behaviour) or round-robin.
Stages overlap through events; ring depth bounds the in-flight batches (the end-of-stream
sentinel is the ring's batch count).  Accuracy = sum over lanes of correct_lane /
dataset_size, like the reference's reduce.  With several GPUs each rank takes an
``array_split`` shard and the per-rank partial accuracies are SUM-reduced (RCCL) -
predictor fan-out across GPUs.  The CPU path runs the same stages without streams.
"""
from __future__ import annotations

import csv
import os
import tempfile
import time
import threading
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional, Sequence

import numpy as np
import torch

from ..config import Config
from ..checkpoint import read_checkpoint, EMA_KEY
from ..data.loader import IMAGENET_MEAN, IMAGENET_STD
from ..data.manifest import SyntheticImages, FolderImages, images_available, synthetic_manifest
from ..models import initialize_model, input_spec
from ..ops import functional as Fn
from ..parallel import (init_world, reduce_scalar, shard_dataframe, broadcast_object,
                        all_gather_object, ParamArena)
from ..parallel.comm import mpi_all_reduce
from ..metrics import macro_scores
from ..utils.logging import init_logger


def load_predictor(cfg: Config, device, ckpt_path: Optional[str] = None):
    """``initialize_model(..., use_pretrained=False)`` + checkpoint ``state_dict``
    (evaluation_pipeline.py:138-147).  ``cfg.eval_ema``: the checkpoint's averaged weights
    (``ema_state_dict``, written by a run with ``ema_decay`` > 0) instead."""
    model, _ = initialize_model(cfg.MODEL_NAME, cfg.NUM_CLASSES, False, use_pretrained=False)
    model = model.to(device)
    model._mpa_arena = ParamArena(model, device)
    path = ckpt_path or os.path.join(cfg.CHECKPOINT_DIR, "checkpoint_{}.pt".format(cfg.MODEL_NAME))
    if cfg.eval_ema and not os.path.exists(path):
        raise FileNotFoundError("eval_ema: no checkpoint at {}".format(path))
    if os.path.exists(path):
        ck = read_checkpoint(path)
        if cfg.eval_ema and EMA_KEY not in ck:
            raise KeyError("eval_ema: checkpoint {} has no {} (it was written by a run without "
                           "ema_decay); evaluate it without --eval_ema".format(path, EMA_KEY))
        sd = ck[EMA_KEY if cfg.eval_ema else "state_dict"]
        model.load_state_dict(sd)
        model._mpa_arena.sync_shadow()
    model.eval()
    return model


class StreamPipeline:
    def __init__(self, model, device, out_hw, lanes: int = 1, depth: int = 4,
                 assign: str = "random", seed: int = 0, mode: int = 1, cpad=None, pad=None,
                 topk: int = 0, macro: bool = False, predict_k: int = 0):
        self.model = model
        if cpad is None:  # the model stem's input layout (models.input_spec)
            spec = input_spec(model, out_hw)
            cpad, pad = spec["cpad"], spec["pad"]
        self.pad = pad
        self.device = torch.device(device)
        self.out_hw = out_hw
        self.lanes = max(1, lanes)
        self.depth = max(2, depth)
        self.assign = assign
        self.rng = np.random.default_rng(seed)
        self.mode = mode
        self.cpad = cpad
        self.cuda = self.device.type == "cuda"
        if self.cuda:
            self.copy_stream = torch.cuda.Stream(self.device)
            self.prep_stream = torch.cuda.Stream(self.device)
            self.lane_streams = [torch.cuda.Stream(self.device) for _ in range(self.lanes)]
        self.counts = [torch.zeros(1, dtype=torch.int64, device=self.device)
                       for _ in range(self.lanes)]
        # topk > 1: a second per-lane counter of rows whose label is among the k largest
        # logits, filled from the same forward as ``counts``
        self.topk = int(topk) if topk and topk > 1 else 0
        self.topk_counts = [torch.zeros(1, dtype=torch.int64, device=self.device)
                            for _ in range(self.lanes)] if self.topk else []
        # macro: per-lane per-class counters int64 [3, NC] (support, predicted, true
        # positives), filled by the argmax pass that fills ``counts`` (made at the first batch,
        # when the head's width is known)
        self.macro = bool(macro)
        self.stats = [None] * self.lanes if self.macro else []
        # predict_k > 0: the k best classes of every row of the shard and their probabilities,
        # int32 / float32 [rows, k] on the device (made by ``run`` / ``run_ring``, which take
        # the row count).  A lane writes its batch's rows [lo, lo + n) on its own stream:
        # disjoint windows, so no lane count or assignment changes a bit
        self.predict_k = int(predict_k)
        if self.predict_k and not 1 <= self.predict_k <= 16:
            raise ValueError("predict_k must be in [1, 16] (0 = off), got %r" % (predict_k,))
        self.pred_idx = self.pred_prob = None
        self.seen = [0] * self.lanes
        self._pinned = {}
        self._last_slot = None

    def _count(self, out, labels, lane: int) -> None:
        if self.macro:
            if self.stats[lane] is None:
                self.stats[lane] = torch.zeros(3, out.shape[1], dtype=torch.int64,
                                               device=self.device)
            Fn.count_class_stats(out, labels, self.counts[lane], self.stats[lane])
        else:
            Fn.count_correct(out, labels, self.counts[lane])
        if self.topk:
            Fn.count_topk(out, labels, self.topk, self.topk_counts[lane])

    def _alloc_predictions(self, rows: Optional[int]) -> None:
        if not self.predict_k:
            return
        if rows is None:
            raise ValueError("predict_k > 0: run / run_ring need the shard's row count (rows=)")
        self.pred_idx = torch.full((rows, self.predict_k), -1, dtype=torch.int32,
                                   device=self.device)
        self.pred_prob = torch.zeros(rows, self.predict_k, dtype=torch.float32,
                                     device=self.device)
        if self.cuda:  # the fills above run on the current stream
            filled = torch.cuda.Event()
            filled.record()
            for s in self.lane_streams:
                s.wait_event(filled)

    def _predict(self, out, lo: int) -> None:
        """Rows [lo, lo + n) of the prediction arrays from the batch's logits."""
        n = out.shape[0]
        Fn.predict_topk(out, self.predict_k, self.pred_idx[lo:lo + n],
                        self.pred_prob[lo:lo + n])

    def predictions(self):
        """(class ids int32 [rows, k], probabilities float32 [rows, k]) as host arrays in the
        order of the shard's rows, -1 / 0 in empty slots (None unless ``predict_k > 0`` and a
        run was made); call after a run."""
        if self.pred_idx is None:
            return None
        return self.pred_idx.cpu().numpy(), self.pred_prob.cpu().numpy()

    def topk_correct(self) -> List[int]:
        """Per-lane top-k correct counts (empty unless ``topk > 1``); call after a run."""
        return [int(c.item()) for c in self.topk_counts]

    def class_stats(self) -> Optional[torch.Tensor]:
        """The lanes' per-class counters summed, int64 [3, NC] on the device (None unless
        ``macro`` and a batch was seen); call after a run."""
        got = [s for s in self.stats if s is not None]
        return torch.stack(got).sum(0) if got else None

    def _lane_for(self, i: int) -> int:
        if self.assign == "roundrobin":
            return i % self.lanes
        return int(self.rng.integers(0, self.lanes))

    def _staging(self, g: torch.Tensor) -> torch.Tensor:
        """Copy a host batch into a reusable pinned buffer (a ring of ``depth + 2``
        slots; a slot is reused only after the copy that read it has completed)."""
        key = (tuple(g.shape), g.dtype)
        ring = self._pinned.setdefault(key, [])
        for slot in ring:
            if slot[1] is None or slot[1].query():
                buf = slot[0]
                break
        else:
            if len(ring) >= self.depth + 2:
                ring[0][1].synchronize()
                buf = ring[0][0]
                slot = ring[0]
            else:
                buf = torch.empty(g.shape, dtype=g.dtype).pin_memory()
                slot = [buf, None]
                ring.append(slot)
        buf.copy_(g)
        self._last_slot = slot
        return buf

    def _preprocess(self, imgs):
        ext = None
        if not isinstance(imgs, np.ndarray):  # decoded images of different sizes: one
            imgs, ext = pad_batch(imgs)        # padded batch + extents, ONE preprocess
        g = torch.from_numpy(imgs)
        if not self.cuda:
            return Fn.preprocess(g, self.out_hw, IMAGENET_MEAN, IMAGENET_STD, self.mode,
                                 self.cpad, out_dtype=torch.float32, pad=self.pad,
                                 extents=ext), None
        g = self._staging(g)
        with torch.cuda.stream(self.copy_stream):
            gd = g.to(self.device, non_blocking=True)
            copied = torch.cuda.Event()
            copied.record(self.copy_stream)
        self._last_slot[1] = copied  # pinned slot free once this copy is done
        self.prep_stream.wait_stream(self.copy_stream)
        with torch.cuda.stream(self.prep_stream):
            gd.record_stream(self.prep_stream)
            x = Fn.preprocess(gd, self.out_hw, IMAGENET_MEAN, IMAGENET_STD, self.mode,
                              self.cpad, pad=self.pad, extents=ext)
            ev = torch.cuda.Event()
            ev.record(self.prep_stream)
        return x, ev

    @torch.no_grad()
    def run(self, batches, rows: Optional[int] = None) -> List[int]:
        """``batches`` yields (uint8 images, int64 labels); returns per-lane correct counts.
        ``rows``: the number of images in all (needed with ``predict_k``)."""
        self._alloc_predictions(rows)
        inflight = []
        lo = 0
        for i, (imgs, labels) in enumerate(batches):
            x, ev = self._preprocess(imgs)
            lane = self._lane_for(i)
            if self.cuda:
                s = self.lane_streams[lane]
                s.wait_event(ev)
                with torch.cuda.stream(s):
                    x.record_stream(s)
                    y = labels.pin_memory().to(self.device, non_blocking=True)
                    out = self.model(x)
                    self._count(out, y, lane)
                    if self.predict_k:
                        self._predict(out, lo)
                    done = torch.cuda.Event()
                    done.record(s)
                inflight.append(done)
                if len(inflight) >= self.depth:
                    inflight.pop(0).synchronize()
            else:
                out = self.model(x)
                self._count(out, labels, lane)
                if self.predict_k:
                    self._predict(out, lo)
            self.seen[lane] += int(labels.shape[0])
            lo += int(labels.shape[0])
        if self.cuda:
            for s in self.lane_streams:
                s.synchronize()
        return [int(c.item()) for c in self.counts]

    @torch.no_grad()
    def run_ring(self, ring, nbatches: int, rows: Optional[int] = None) -> List[int]:
        """GPU stages fed by a native ``BatchRing``: no per-batch host copy, pinning or
        Python image work on the consumer thread.  Returns per-lane correct counts.
        ``rows``: the number of images in all (needed with ``predict_k``)."""
        self._alloc_predictions(rows)
        pending = []   # (slot, copy event): the slot returns to the ring once copied
        inflight = []  # lane completion events (bounds the batches in flight)
        depth = ring.depth()
        for i in range(nbatches):
            keep = []
            for k, (slot, ev) in enumerate(pending):
                if ev.query() or len(pending) - k >= depth - 1:
                    ev.synchronize()
                    ring.release(slot)
                else:
                    keep.append((slot, ev))
            pending = keep
            slot, img_h, lab_h, bidx = ring.acquire()
            n, ext_h = ring.info(slot)
            ext = ext_h[:n].numpy().copy()
            uniform = bool((ext[:, 0] == img_h.shape[1]).all() and (ext[:, 1] == img_h.shape[2]).all())
            with torch.cuda.stream(self.copy_stream):
                img_d = img_h[:n].to(self.device, non_blocking=True)
                lab_d = lab_h[:n].to(self.device, non_blocking=True)
                copied = torch.cuda.Event()
                copied.record(self.copy_stream)
            pending.append((slot, copied))
            self.prep_stream.wait_event(copied)
            with torch.cuda.stream(self.prep_stream):
                img_d.record_stream(self.prep_stream)
                x = Fn.preprocess(img_d, self.out_hw, IMAGENET_MEAN, IMAGENET_STD, self.mode,
                                  self.cpad, pad=self.pad, extents=None if uniform else ext)
                prepped = torch.cuda.Event()
                prepped.record(self.prep_stream)
            lane = self._lane_for(i)
            s = self.lane_streams[lane]
            s.wait_event(prepped)
            with torch.cuda.stream(s):
                x.record_stream(s)
                lab_d.record_stream(s)
                out = self.model(x)
                self._count(out, lab_d, lane)
                if self.predict_k:  # the ring hands batches out in index order
                    self._predict(out, bidx * img_h.shape[0])
                done = torch.cuda.Event()
                done.record(s)
            inflight.append(done)
            if len(inflight) >= self.depth:
                inflight.pop(0).synchronize()
            self.seen[lane] += n
        for slot, ev in pending:
            ev.synchronize()
            ring.release(slot)
        for s in self.lane_streams:
            s.synchronize()
        return [int(c.item()) for c in self.counts]


def global_class_stats(pipe: StreamPipeline, num_classes: int) -> torch.Tensor:
    """``pipe``'s per-class counters summed over its lanes, then over the ranks (int64
    [3, num_classes] on every rank): integer counts, so the order does not matter.  A
    collective: every rank calls it."""
    stats = pipe.class_stats()
    if stats is None:  # (a rank whose shard is empty)
        stats = torch.zeros(3, num_classes, dtype=torch.int64, device=pipe.device)
    return mpi_all_reduce(stats)


def pad_batch(imgs):
    """A list of uint8 HWC images of different sizes -> one zero-padded [B, Hmax, Wmax, 3]
    batch and the per-image extents [B, 2] (each image at the top-left of its slot)."""
    H = max(a.shape[0] for a in imgs)
    W = max(a.shape[1] for a in imgs)
    buf = np.zeros((len(imgs), H, W, 3), dtype=np.uint8)
    for b, a in enumerate(imgs):
        buf[b, :a.shape[0], :a.shape[1]] = a
    return buf, np.array([a.shape[:2] for a in imgs], dtype=np.int64)


def make_ring(names: Sequence[str], labels: Sequence[int], batch: int, source, num_classes: int,
              depth: int = 8, threads: int = 4, pitch=None):
    """Stage 0 on the native ring for one manifest shard.  ``SyntheticImages``: window mode
    (C++ threads, bitwise ``source.load``).  ``FolderImages``: PIL decode threads write each
    image into its slot at its own extent (``pitch`` = the largest image, from the
    manifest's height/width columns when given).  Returns (ring, number of batches)."""
    from ..ops import _ext
    nb = (len(names) + batch - 1) // batch
    if isinstance(source, SyntheticImages):
        H, W = source.hw
        ring = _ext.ext().BatchRing(batch, H, W, num_classes, depth, threads, 0, 0, 1, False)
        offs = torch.tensor([source._offset(n) for n in names], dtype=torch.int64).view(-1, 2)
        ring.set_window_source(torch.from_numpy(source.tex), offs,
                               torch.as_tensor(np.asarray(labels, dtype=np.int64)))
        return ring, nb
    if pitch is None:
        raise ValueError("make_ring: real images need the slot pitch (max height, width)")
    ring = _ext.ext().BatchRing(batch, int(pitch[0]), int(pitch[1]), num_classes, depth, threads,
                                0, 0, 1, False)
    _feed_external(ring, list(names), np.asarray(labels, dtype=np.int64), batch, source, threads)
    return ring, nb


_FEED_ERRORS = {}  # id(ring) -> decode exceptions of its feeder threads


def feed_error(ring):
    """The first exception a decode thread of ``ring`` hit (it then stopped the ring), or
    None."""
    errs = _FEED_ERRORS.get(id(ring))
    return errs[0] if errs else None


def _feed_external(ring, names, labels, batch, source, threads: int) -> None:
    """PIL decode threads for real images: each takes an empty slot, THEN the next batch
    index, decodes its images straight into the slot (top-left, extent recorded) and
    commits it.  The ring hands batches to the consumer in index order, so a thread must
    own a slot before it owns an index: otherwise later indices could fill every free slot
    while the thread holding the next one waits for a slot forever.  A decode error stops
    the ring (the consumer's acquire raises instead of hanging; ``feed_error`` has it)."""
    nb = (len(names) + batch - 1) // batch
    lock = threading.Lock()
    nxt = [0]
    errors = _FEED_ERRORS.setdefault(id(ring), [])

    def worker():
        from PIL import Image
        while True:
            try:
                slot, img, lab, ext = ring.acquire_empty()
            except RuntimeError:  # ring stopped
                return
            with lock:
                bi = nxt[0]
                nxt[0] += 1
            if bi >= nb:
                ring.release(slot)
                return
            try:
                a = img.numpy()
                e = ext.numpy()
                lo, hi = bi * batch, min((bi + 1) * batch, len(names))
                for b, j in enumerate(range(lo, hi)):
                    with Image.open(os.path.join(source.root, names[j])) as im:
                        arr = np.asarray(im.convert("RGB"))
                    h, w = min(arr.shape[0], a.shape[1]), min(arr.shape[1], a.shape[2])
                    a[b, :h, :w] = arr[:h, :w]
                    e[b] = (h, w)
                    lab.numpy()[b] = labels[j]
            except Exception as ex:  # noqa: BLE001 - reported through feed_error
                errors.append(ex)
                ring.stop()
                return
            ring.commit(slot, bi, hi - lo)

    for _ in range(max(1, threads)):
        threading.Thread(target=worker, name="mpa-decode", daemon=True).start()


def _batches(names, labels, batch: int, source, prefetch: int = 2):
    """Stage 0: host read/decode in a worker pool, ``prefetch`` batches ahead."""
    pool = ThreadPoolExecutor(max_workers=2)
    idx = [np.arange(i, min(i + batch, len(names))) for i in range(0, len(names), batch)]
    futs = [pool.submit(source.load, [names[j] for j in ix]) for ix in idx[:prefetch]]
    for k, ix in enumerate(idx):
        imgs = futs[k].result()
        if k + prefetch < len(idx):
            futs.append(pool.submit(source.load, [names[j] for j in idx[k + prefetch]]))
        yield imgs, torch.as_tensor(np.asarray([labels[j] for j in ix], dtype=np.int64))
    pool.shutdown()


def run_pipeline(cfg: Config, ckpt_path: Optional[str] = None, max_images: int = 0) -> float:
    world = init_world(cfg.device, cfg.timeout_s)
    log = init_logger(world.rank, cfg.log_file or "evaluation.log", cfg.log_per_rank_files)
    df = None
    if world.rank == 0:
        log.info("Logger Initialized")
        if os.path.exists(cfg.TEST_CSV) and cfg.synthetic_images <= 0:
            import pandas as pd
            df = pd.read_csv(cfg.TEST_CSV)
        else:
            df = synthetic_manifest(cfg.synthetic_images or 256, cfg.NUM_CLASSES, cfg.seed)
        if max_images:
            df = df.iloc[:max_images]
    df = broadcast_object(df)
    dataset_size = len(df)
    shard = shard_dataframe(df, world.world_size)[world.rank]
    out_hw = cfg.input_hw if cfg.MODEL_NAME != "inception" else (299, 299)
    names = list(shard["file_name"].values)
    # a manifest without labels (a real test set): every label is -1, which the counting
    # kernels ignore, and no accuracy is reported
    labelled = "category_id" in df.columns
    labels = list(shard["category_id"].values) if labelled else [-1] * len(names)
    if not cfg.synthetic and images_available(cfg.TRAIN_DIR, names):
        source = FolderImages(cfg.TRAIN_DIR, cfg.num_workers)  # reads TRAIN_DIR like :59
    else:
        # synthetic sources at the model's input size by default (eval_src > 0: that side):
        # the resize stage still runs (PIL-exact bicubic), but stage 0 copies and the H2D
        # link carries 150 KB per 224^2 image instead of the 600 KB of a 448^2 source,
        # which capped the pipeline near PCIe's ~50 GB/s / 600 KB = 83k img/s
        side = cfg.eval_src
        source = SyntheticImages((side, side) if side > 0 else tuple(out_hw))
    model = load_predictor(cfg, world.device, ckpt_path)
    pipe = StreamPipeline(model, world.device, out_hw, cfg.eval_lanes, assign=cfg.eval_assign,
                          seed=cfg.seed + world.rank, topk=cfg.eval_topk, macro=cfg.eval_macro,
                          predict_k=cfg.predict_topk if cfg.predictions_csv else 0)
    t0 = time.perf_counter()
    if world.device.type == "cuda":
        pitch = None
        if isinstance(source, FolderImages):
            pitch = (int(shard["height"].max()), int(shard["width"].max())) \
                if {"height", "width"} <= set(shard.columns) else (1024, 1024)
        ring, nb = make_ring(names, labels, cfg.eval_batch, source, cfg.NUM_CLASSES,
                             threads=max(2, cfg.num_workers), pitch=pitch)
        try:
            counts = pipe.run_ring(ring, nb, rows=len(names))
        except RuntimeError as e:
            fe = feed_error(ring)
            if fe is not None:
                raise RuntimeError("eval pipeline: image decode failed: %r" % (fe,)) from e
            raise
        finally:
            ring.stop()
            _FEED_ERRORS.pop(id(ring), None)
    else:
        counts = pipe.run(_batches(names, labels, cfg.eval_batch, source), rows=len(names))
    dt = time.perf_counter() - t0
    acc_local = 0.0
    for lane, c in enumerate(counts):
        a = c / max(dataset_size, 1)
        acc_local += a
        log.info("Finished node {}, acc {}".format(world.rank * pipe.lanes + lane + 3, a))
    total = reduce_scalar(acc_local, root=0)
    total_k = None
    if pipe.topk:
        total_k = reduce_scalar(sum(pipe.topk_correct()) / max(dataset_size, 1), root=0)
    macro = macro_scores(global_class_stats(pipe, cfg.NUM_CLASSES)) if pipe.macro else None
    # shard_dataframe's shards are contiguous: the ranks' arrays, in rank order, are the
    # manifest's rows in order
    parts = all_gather_object(pipe.predictions()) if pipe.predict_k else None
    if world.rank == 0:
        if not labelled:
            log.info("No labels in {}: accuracy not computed".format(cfg.TEST_CSV))
        else:
            log.info("Accuracy is {}".format(total))
            if pipe.topk:
                log.info("Top-{} accuracy is {}".format(pipe.topk, total_k))
            if macro is not None:
                log.info("Macro-F1 is {}".format(macro["macro_f1"]))
                log.info("Balanced accuracy is {}".format(macro["balanced_acc"]))
        # the source extent is part of the number: a synthetic source at the model's input
        # size skips the downscale real ~1000x677 herbarium JPEGs need (cfg.eval_src)
        src = "real images" if isinstance(source, FolderImages) else \
            "synthetic {}x{} source".format(*source.hw)
        log.info("_Throughput: {:.1f} img/s ({} images, {} lanes x {} ranks, {})".format(
            dataset_size / dt if dt > 0 else 0.0, dataset_size, pipe.lanes, world.world_size,
            src))
        if parts is not None:
            ids = df["id" if "id" in df.columns else "file_name"].values
            write_predictions(cfg.predictions_csv, ids, np.concatenate([p[0] for p in parts]),
                              np.concatenate([p[1] for p in parts]))
            log.info("Predictions written to {} ({} rows, top-{})".format(
                cfg.predictions_csv, len(ids), pipe.predict_k))
    if not labelled:
        return float("nan")
    return float(total) if total is not None else acc_local


def write_predictions(path: str, ids, idx: np.ndarray, prob: np.ndarray) -> None:
    """The predictions file: a header ``Id,Predicted,Probability`` (then ``Predicted_j,
    Probability_j`` for j = 2..k) and one row per id; class ids are integers (-1: an empty
    slot) and probabilities ``%.9g``, which a float32 survives.  Written to a temporary file
    in the same directory and moved into place, so a crash leaves no truncated file."""
    n, k = idx.shape
    if len(ids) != n or prob.shape != idx.shape:
        raise ValueError("write_predictions: {} ids, idx {}, prob {}".format(
            len(ids), idx.shape, prob.shape))
    header = ["Id", "Predicted", "Probability"]
    for j in range(2, k + 1):
        header += ["Predicted_%d" % j, "Probability_%d" % j]
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    fd, tmp = tempfile.mkstemp(prefix="tmp_pred_", suffix=".csv", dir=d)
    try:
        with os.fdopen(fd, "w", newline="") as fh:
            w = csv.writer(fh, lineterminator="\n")
            w.writerow(header)
            for i in range(n):
                row = [ids[i]]
                for j in range(k):
                    row += [int(idx[i, j]), "%.9g" % float(prob[i, j])]
                w.writerow(row)
        # mkstemp made the file owner-only; give it the mode a plain open() would have
        umask = os.umask(0)
        os.umask(umask)
        os.chmod(tmp, 0o666 & ~umask)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


@torch.no_grad()
def plain_eval(model, names, labels, batch, source, device, out_hw, mode=1) -> int:
    """Non-pipelined batched evaluation (oracle for the pipeline tests): host batches,
    one preprocess call per batch in the model's input layout (images of different sizes
    padded into one batch with extents), forward, correct count."""
    spec = input_spec(model, out_hw)
    correct = torch.zeros(1, dtype=torch.int64, device=device)
    for imgs, lab in _batches(names, labels, batch, source):
        ext = None
        if not isinstance(imgs, np.ndarray):
            imgs, ext = pad_batch(imgs)
        g = torch.from_numpy(imgs).to(device)
        x = Fn.preprocess(g, out_hw, IMAGENET_MEAN, IMAGENET_STD, mode, spec["cpad"],
                          out_dtype=torch.float32, pad=spec["pad"], extents=ext)
        Fn.count_correct(model(x), lab.to(device), correct)
    return int(correct.item())


@torch.no_grad()
def plain_predict(model, names, batch, source, device, out_hw, k: int, mode=1):
    """Non-pipelined batched prediction (oracle for the pipeline's ``predictions()``): the
    same two host arrays from one preprocess + forward + ``predict_topk`` per batch on the
    current stream, with the pipeline's preprocess arguments (the model's input layout; bf16
    on the GPU, fp32 on the CPU)."""
    device = torch.device(device)
    spec = input_spec(model, out_hw)
    dtype = {} if device.type == "cuda" else {"out_dtype": torch.float32}
    idx = torch.full((len(names), k), -1, dtype=torch.int32, device=device)
    prob = torch.zeros(len(names), k, dtype=torch.float32, device=device)
    lo = 0
    for imgs, _lab in _batches(names, [-1] * len(names), batch, source):
        ext = None
        if not isinstance(imgs, np.ndarray):
            imgs, ext = pad_batch(imgs)
        g = torch.from_numpy(imgs).to(device)
        x = Fn.preprocess(g, out_hw, IMAGENET_MEAN, IMAGENET_STD, mode, spec["cpad"],
                          pad=spec["pad"], extents=ext, **dtype)
        n = x.shape[0]
        Fn.predict_topk(model(x), k, idx[lo:lo + n], prob[lo:lo + n])
        lo += n
    return idx.cpu().numpy(), prob.cpu().numpy()
