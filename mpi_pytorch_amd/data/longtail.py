"""Class priors of a long-tailed training set, for the logit-adjusted loss (Menon et al.
2021, "Long-tail learning via logit adjustment"): the training loss is cross-entropy of
``logits + tau * log(prior)``, so a head class has to win by its prior's margin and the tail
is not swamped.  ``ops.functional.cross_entropy(logit_bias=)`` adds the term inside the loss
kernels.
"""
from __future__ import annotations

import numpy as np
import torch


def class_log_prior(labels, num_classes: int) -> torch.Tensor:
    """fp32 [num_classes]: ``log((n_c + 1) / (N + num_classes))`` from the labels of the whole
    (unsharded) training manifest, computed in float64.  The Laplace count keeps a class
    without a training image finite.  Labels outside [0, num_classes) are not counted.  The
    result depends on the label counts only, so every rank that sees the same manifest holds
    the same vector bitwise."""
    nc = int(num_classes)
    if nc < 1:
        raise ValueError("class_log_prior: num_classes must be >= 1")
    lab = np.asarray(labels, dtype=np.int64).reshape(-1)
    lab = lab[(lab >= 0) & (lab < nc)]
    counts = np.bincount(lab, minlength=nc).astype(np.float64)
    logp = np.log((counts + 1.0) / (float(lab.size) + float(nc)))
    return torch.from_numpy(logp.astype(np.float32))


def logit_bias(labels, num_classes: int, tau: float, device=None) -> torch.Tensor:
    """``tau * class_log_prior(labels, num_classes)`` as a contiguous fp32 tensor on
    ``device``: the ``logit_bias`` of the training loss (the product is taken in fp32 on the
    host, so it does not depend on the device either)."""
    if not tau >= 0.0:
        raise ValueError("logit_adjust_tau must be >= 0 (0 = off)")
    bias = (class_log_prior(labels, num_classes) * float(tau)).contiguous()
    return bias if device is None else bias.to(device)
