"""Random-resized-crop and horizontal-flip parameters for the training preprocess launch.

The preprocess kernel (``csrc/kernels/preprocess.hip``, ``Fn.preprocess(boxes=)``) crops,
resizes, mirrors and normalises in one launch; the host only draws five integers per
image, ``(y0, x0, h, w, flip)``.  :func:`sample_boxes` draws them with torchvision's
``RandomResizedCrop.get_params`` algorithm followed by a fair-coin ``RandomHorizontalFlip``.

Randomness is counter-based: every uniform is a 32-bit hash of ``(seed, epoch, id, draw
index)`` (the murmur3-style mix of the dropout kernel's ``hash3``), vectorised over the
batch.  ``id`` is stable per sample (:func:`sample_ids`: crc32 of the file name, the key
``SyntheticImages`` already uses), so a sample's box and flip depend on nothing but
``(seed, epoch, id, extent)`` - not on its batch, its position in the batch, the batch
size or the number of ranks.

Mixup / CutMix (:func:`sample_mix`) pair every sample with the next one of its batch, so
their parameters belong to the batch: one generator per call, keyed by ``(seed, epoch, the
ids in batch order)`` and dropped afterwards.  The preprocess launch blends the images
(``Fn.preprocess(mix=, lam=)``) and the fused cross-entropy the labels
(:func:`label_weights`).
"""
from __future__ import annotations

import math
import zlib
from typing import Sequence, Tuple

import numpy as np

TRIES = 10                    # get_params' attempts before the centre-crop fallback
_DRAWS = 4                    # per try: area, aspect, top, left
_FLIP_DRAW = TRIES * _DRAWS   # draw index of the flip coin


def sample_ids(names: Sequence[str]) -> np.ndarray:
    """Stable per-sample ids: crc32 of the file name (uint32 [N])."""
    return np.array([zlib.crc32(str(n).encode()) for n in names], dtype=np.uint32)


def _mix(h: np.ndarray) -> np.ndarray:
    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x85EBCA6B)
    h = h ^ (h >> np.uint32(13))
    h = h * np.uint32(0xC2B2AE35)
    return h ^ (h >> np.uint32(16))


def hash4(seed: int, epoch: int, ids: np.ndarray, draw: np.ndarray) -> np.ndarray:
    """uint32 hash of (seed, epoch, id, draw index), broadcast over ``ids`` and ``draw``:
    ``hash3`` of preprocess.hip over (seed, epoch, id), finalised again with the draw."""
    ids = np.asarray(ids).astype(np.uint32)
    draw = np.asarray(draw).astype(np.uint32)
    a = np.uint32(seed & 0xFFFFFFFF) * np.uint32(0x9E3779B1)
    b = (np.uint32(epoch & 0xFFFFFFFF) + np.uint32(0x7F4A7C15)) * np.uint32(0x85EBCA77)
    h = _mix(a ^ b ^ (ids * np.uint32(0xC2B2AE3D)))
    return _mix(h ^ ((draw + np.uint32(0x165667B1)) * np.uint32(0x27D4EB2F)))


def _uniform(seed, epoch, ids, draw) -> np.ndarray:
    """float64 uniforms in [0, 1) with 24 random bits (as the dropout kernel's)."""
    return (hash4(seed, epoch, ids, draw) >> np.uint32(8)).astype(np.float64) / 16777216.0


def fallback_box(H: int, W: int, ratio=(3.0 / 4.0, 4.0 / 3.0)) -> Tuple[int, int, int, int]:
    """get_params' fallback: the centre crop with the image's ratio clamped into ``ratio``."""
    in_ratio = W / H
    if in_ratio < min(ratio):
        w = W
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = H
        w = int(round(h * max(ratio)))
    else:
        h, w = H, W
    h, w = min(max(h, 1), H), min(max(w, 1), W)
    return (H - h) // 2, (W - w) // 2, h, w


def sample_boxes(ids, extents, epoch: int, seed: int, scale=(0.08, 1.0),
                 ratio=(3.0 / 4.0, 4.0 / 3.0), flip_p: float = 0.5,
                 crop: bool = True) -> np.ndarray:
    """int32 [B, 5] rows (y0, x0, h, w, flip) for images of ``extents`` [B, 2] = (H, W).

    crop: up to ``TRIES`` attempts, each a target area uniform in ``scale`` x the image's
    area and a log-uniform aspect ratio in ``ratio``; the first whose rounded (h, w) fits
    the image is placed uniformly over the valid corners; if none fits, the centre crop of
    :func:`fallback_box`.  ``crop=False``: the full extent (flip only).  flip: 1 with
    probability ``flip_p``."""
    with np.errstate(over="ignore"):  # uint32 wrap-around is the hash
        ids = np.asarray(ids).astype(np.uint32).reshape(-1)
        ext = np.asarray(extents, dtype=np.int64).reshape(-1, 2)
        B = ids.shape[0]
        if ext.shape[0] != B:
            raise ValueError("sample_boxes: %d ids for %d extents" % (B, ext.shape[0]))
        if B and (ext < 1).any():
            raise ValueError("sample_boxes: empty extent")
        H, W = ext[:, 0], ext[:, 1]
        out = np.zeros((B, 5), dtype=np.int32)
        out[:, 4] = _uniform(seed, epoch, ids, _FLIP_DRAW) < flip_p
        if not crop:
            out[:, 2], out[:, 3] = H, W
            return out
        t = np.arange(TRIES, dtype=np.uint32)[None, :] * np.uint32(_DRAWS)   # [1, T]
        u = [_uniform(seed, epoch, ids[:, None], t + np.uint32(k)) for k in range(_DRAWS)]
        area = (H * W).astype(np.float64)[:, None] * (scale[0] + (scale[1] - scale[0]) * u[0])
        lr = (math.log(ratio[0]), math.log(ratio[1]))
        aspect = np.exp(lr[0] + (lr[1] - lr[0]) * u[1])
        w = np.rint(np.sqrt(area * aspect)).astype(np.int64)                   # [B, T]
        h = np.rint(np.sqrt(area / aspect)).astype(np.int64)
        ok = (w > 0) & (w <= W[:, None]) & (h > 0) & (h <= H[:, None])
        first = np.argmax(ok, axis=1)                                          # first accepted try
        rows = np.arange(B)
        hh, ww = h[rows, first], w[rows, first]
        y0 = np.floor(u[2][rows, first] * (H - hh + 1)).astype(np.int64)
        x0 = np.floor(u[3][rows, first] * (W - ww + 1)).astype(np.int64)
        hit = ok.any(axis=1)
        fb = np.array([fallback_box(int(a), int(b), ratio) for a, b in ext[~hit]],
                      dtype=np.int64).reshape(-1, 4)
        out[hit, 0], out[hit, 1], out[hit, 2], out[hit, 3] = y0[hit], x0[hit], hh[hit], ww[hit]
        out[~hit, :4] = fb
        return out


def _mix_draws(ids, epoch: int, seed: int, mixup_alpha: float, cutmix_alpha: float,
               prob: float, switch_prob: float):
    """The per-sample draws of :func:`sample_mix`: (mixed, cut) bool [B], beta [B] (Mixup's
    lam or CutMix's l0; 1 where neither applies) and the rectangle centres (uy, ux) in
    [0, 1).  Always the same number of draws in the same order, whatever the arguments."""
    ids = np.ascontiguousarray(np.asarray(ids).astype(np.uint32).reshape(-1))
    B = ids.shape[0]
    rng = np.random.default_rng([int(seed) & 0xFFFFFFFF, int(epoch) & 0xFFFFFFFF,
                                 zlib.crc32(ids.tobytes()), B])
    u_use, u_cut, uy, ux = rng.random((4, B))
    b_mix = rng.beta(mixup_alpha, mixup_alpha, B) if mixup_alpha > 0 else np.ones(B)
    b_cut = rng.beta(cutmix_alpha, cutmix_alpha, B) if cutmix_alpha > 0 else np.ones(B)
    mixed = (u_use < prob) & (mixup_alpha > 0 or cutmix_alpha > 0)
    if mixup_alpha > 0 and cutmix_alpha > 0:
        cut = mixed & (u_cut < switch_prob)
    else:
        cut = mixed & (cutmix_alpha > 0)
    beta = np.where(cut, b_cut, np.where(mixed, b_mix, 1.0))
    return mixed, cut, beta, uy, ux


def sample_mix(ids, epoch: int, seed: int, out_hw, mixup_alpha: float, cutmix_alpha: float,
               prob: float = 1.0, switch_prob: float = 0.5) -> Tuple[np.ndarray, np.ndarray]:
    """``(mix int32 [B, 5], lam float32 [B])`` for ``Fn.preprocess(mix=, lam=)``: rows
    (partner, y0, x0, h, w) with the rectangle in pixels of the (OH, OW) output.

    partner: the next sample of the batch, ``(i + 1) % B``.  Per sample, with probability
    ``1 - prob`` nothing (lam 1, no rectangle); otherwise CutMix with probability
    ``switch_prob`` and Mixup otherwise when both alphas are > 0, or the one that is on.
    Mixup: lam ~ Beta(a, a), no rectangle.  CutMix: l0 ~ Beta(a, a), r = sqrt(1 - l0), a
    rectangle of sides int(OH * r), int(OW * r) around a centre uniform over the image,
    clipped to the image; lam is 1 (the rectangle does the mixing) and the label's weight is
    the area that stays (:func:`label_weights`).  A function of (seed, epoch, ids in batch
    order, arguments) only: no generator state outlives the call."""
    if mixup_alpha < 0 or cutmix_alpha < 0:
        raise ValueError("sample_mix: alphas must be >= 0")
    if not (0.0 <= prob <= 1.0 and 0.0 <= switch_prob <= 1.0):
        raise ValueError("sample_mix: probabilities must be in [0, 1]")
    OH, OW = int(out_hw[0]), int(out_hw[1])
    mixed, cut, beta, uy, ux = _mix_draws(ids, epoch, seed, mixup_alpha, cutmix_alpha, prob,
                                          switch_prob)
    B = beta.shape[0]
    mix = np.zeros((B, 5), dtype=np.int32)
    mix[:, 0] = (np.arange(B) + 1) % max(B, 1)
    r = np.sqrt(1.0 - beta)
    h, w = (OH * r).astype(np.int64), (OW * r).astype(np.int64)
    cy, cx = (uy * OH).astype(np.int64), (ux * OW).astype(np.int64)
    y0, y1 = np.clip(cy - h // 2, 0, OH), np.clip(cy + h // 2, 0, OH)
    x0, x1 = np.clip(cx - w // 2, 0, OW), np.clip(cx + w // 2, 0, OW)
    box = cut & (y1 > y0) & (x1 > x0)
    mix[box, 1], mix[box, 2] = y0[box], x0[box]
    mix[box, 3], mix[box, 4] = (y1 - y0)[box], (x1 - x0)[box]
    lam = np.where(mixed & ~cut, beta, 1.0).astype(np.float32)
    return mix, lam


def label_weights(mix: np.ndarray, lam: np.ndarray, out_hw) -> np.ndarray:
    """float32 [B]: the weight of each sample's own label under :func:`sample_mix`'s rows -
    Mixup: lam; CutMix: ``1 - area / (OH * OW)`` of the clipped rectangle; unmixed: 1."""
    area = mix[:, 3].astype(np.float64) * mix[:, 4].astype(np.float64)
    keep = 1.0 - area / float(int(out_hw[0]) * int(out_hw[1]))
    return np.where(area > 0, keep, lam.astype(np.float64)).astype(np.float32)
