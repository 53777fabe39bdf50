"""Class-balanced validation scores from the per-class counters that
``ops.functional.count_class_stats`` accumulates (``argmax_stats`` in csrc/kernels/loss.hip).
"""
from __future__ import annotations

import torch


def macro_scores(stats: torch.Tensor) -> dict:
    """``stats``: integer [3, NC] = (support, predicted, true positives) per class.  Returns
    float64 results computed on ``stats``' device (one host sync, once per evaluation):

    * ``macro_f1``: the mean of ``2 tp / (support + predicted)`` over the classes with
      ``support + predicted > 0`` - the label set of sklearn's ``f1_score(average="macro")``,
      the classes that occur among the labels or the predictions;
    * ``balanced_acc``: the mean of the recall ``tp / support`` over the classes with
      ``support > 0``;
    * ``classes_seen``: the number of classes with ``support > 0``.

    No class at all gives 0.0 for both scores."""
    if stats.dim() != 2 or stats.shape[0] != 3:
        raise ValueError("macro_scores: stats must be [3, NC], got %s" % (tuple(stats.shape),))
    support, predicted, tp = stats.to(torch.float64).unbind(0)
    denom = support + predicted
    in_f1 = denom > 0
    seen = support > 0
    f1 = torch.where(in_f1, 2.0 * tp / denom.clamp(min=1.0), torch.zeros_like(tp))
    recall = torch.where(seen, tp / support.clamp(min=1.0), torch.zeros_like(tp))
    out = torch.stack([f1.sum(), in_f1.sum().to(torch.float64), recall.sum(),
                       seen.sum().to(torch.float64)]).tolist()
    return {"macro_f1": out[0] / out[1] if out[1] else 0.0,
            "balanced_acc": out[2] / out[3] if out[3] else 0.0,
            "classes_seen": int(out[3])}
