"""Typed run configuration.

The reference keeps every tunable as a hand-edited module constant in ``utils.py``
(``/root/reference/utils.py:4-45``) with no CLI or environment overrides.  This module
keeps the *same field names* (so ``cfg.MODEL_NAME``, ``cfg.BATCH_SIZE`` ... read exactly
like the reference) and adds:

* CLI overrides (``--MODEL_NAME resnet34`` or ``--model-name resnet34``),
* environment overrides (``MPA_MODEL_NAME=resnet34``),
* MI355X fields the reference does not have: ``dtype``, ``bucket_mb``, ``synthetic``,
  ``image_size``, ``optimizer``, ``momentum``, ``per_gpu_batch``, ``backend`` ...

Precedence: defaults < environment < explicit kwargs/CLI.
"""
from __future__ import annotations

import argparse
import dataclasses
import os
from dataclasses import dataclass, field, fields
from typing import Any, Dict, List, Optional

MODEL_NAMES = ("resnet18", "resnet34", "alexnet", "vgg", "vgg16", "squeezenet",
               "densenet", "inception")

_ENV_PREFIX = "MPA_"


@dataclass
class Config:
    # ---- reference fields (utils.py:4-45) -------------------------------------------
    MODEL_NAME: str = "resnet18"           # utils.py:4
    FROM_CHECKPOINT: bool = False          # utils.py:5
    VALIDATE: bool = True                  # utils.py:6
    CHECKPOINT_NAME: str = ""              # utils.py:7 (derived from MODEL_NAME if empty)
    DEBUG: bool = True                     # utils.py:13
    N_IMAGES: int = 50000                  # utils.py:14
    TRAIN_DIR: str = "./data/train/"       # utils.py:22
    TRAIN_FILE: str = "metadata.json"      # utils.py:23
    TEST_DIR: str = "./data/test/"         # utils.py:24
    CHECKPOINT_DIR: str = "./checkpoints/"  # utils.py:26
    MODELS_DIR: str = "./models/"          # utils.py:27
    WIDTH: int = 128                       # utils.py:33
    HEIGHT: int = 128                      # utils.py:34
    NUM_CLASSES: int = 64500               # utils.py:39
    BATCH_SIZE: int = 128                  # utils.py:40 (per rank)
    LR: float = 4e-4                       # utils.py:41
    NUM_EPOCHS: int = 10                   # utils.py:42
    FEATURE_EXTRACT: bool = False          # utils.py:43
    USE_PRETRAINED: bool = False           # utils.py:45 (no hub download offline)

    # ---- manifest paths (hard-coded in the reference: main.py:77,81-82) ----------------
    TRAIN_CSV: str = "./data/train_sample.csv"
    TEST_CSV: str = "./data/test_sample.csv"
    DEBUG_SAMPLE: int = 1000               # main.py:78 sample(1000, random_state=0)

    # ---- new fields --------------------------------------------------------------------
    device: str = "auto"                   # auto | cuda | cpu
    dtype: str = "bf16"                    # compute dtype on GPU (bf16); CPU always fp32
    synthetic: bool = True                 # synthetic images (no Herbarium data offline)
    synthetic_images: int = 0              # images per epoch in synthetic mode (0 => 800 like DEBUG)
    image_size: int = 0                    # 0 => use WIDTH/HEIGHT
    optimizer: str = "adam"                # adam | sgd | adamw | lamb | lars
    momentum: float = 0.9
    weight_decay: float = 0.0              # adam | sgd: coupled L2; adamw | lamb | lars: decoupled
    trust_coef: float = 0.001              # lars: the trust ratio's coefficient
    wd_exclude_1d: bool = True             # adamw | lamb | lars: no decay / trust ratio on 1-D
                                           # parameters (BN, biases); adam | sgd decay everything
    # training recipe on the device (optim.py; all off by default = the reference's recipe)
    lr_schedule: str = "constant"          # constant | cosine | step (after the warm-up)
    warmup_steps: int = 0                  # linear warm-up: lr * (k + 1) / warmup_steps
    lr_min_ratio: float = 0.0              # cosine floor, as a fraction of LR
    lr_gamma: float = 0.1                  # step: LR * lr_gamma ^ floor(k / lr_decay_steps)
    lr_decay_steps: int = 0
    clip_grad_norm: float = 0.0            # global-norm gradient clipping (0.0 = off)
    # input augmentation of the training loader, inside the preprocess launch
    # (data/augment.py; off by default = the reference's ToTensor -> Resize -> Normalize)
    augment: str = "none"                  # none | flip | rrc (random-resized crop + flip)
    aug_scale_min: float = 0.08            # rrc: smallest crop, as a fraction of the image area
    label_smoothing: float = 0.0           # training-loss label smoothing in [0, 1] (0 = off)
    # long-tail head (data/longtail.py, metrics.py; both off by default)
    logit_adjust_tau: float = 0.0          # training loss on logits + tau * log(class prior); 0 = off
    eval_macro: bool = False               # also report macro-F1 and balanced accuracy
    # sample mixing of the training loader (data/augment.py::sample_mix): images blended in
    # the preprocess launch, labels in the fused cross-entropy; off when both alphas are 0
    mixup_alpha: float = 0.0               # Mixup: lam ~ Beta(alpha, alpha)
    cutmix_alpha: float = 0.0              # CutMix: the pasted rectangle's area from Beta(alpha, alpha)
    mix_prob: float = 1.0                  # probability that a sample is mixed at all
    mix_switch_prob: float = 0.5           # both on: probability of CutMix (else Mixup)
    # exponential moving average of the weights on the device (ema.py; off at 0)
    ema_decay: float = 0.0                 # in [0, 1): ema += (1 - d_t) * (p - ema) after each update
    ema_warmup: bool = True                # d_t = min(ema_decay, (1 + t) / (10 + t))
    eval_ema: bool = False                 # evaluation pipeline: load the checkpoint's averaged weights
    bucket_mb: float = 16.0                # gradient all-reduce bucket size (MiB)
    grad_comm_dtype: str = "fp32"          # fp32 | bf16 (wire dtype of the gradient all-reduce)
    overlap_comm: bool = True              # launch bucket all-reduce during backward
    grad_comm_ctas: int = -1               # >0: overlapped buckets on a CTA-capped RCCL
                                           # communicator + comm-aware persistent conv grids
                                           # (0 off; -1: MPA_COMM_CTAS or the default)
    resume_epoch: bool = True              # honour saved epoch (reference restarts at 0: main.py:142)
    graph: str = "auto"                    # auto | on | off : HIP-graph capture of the train step
    seed: int = 0
    log_file: str = "training.log"
    log_per_rank_files: bool = False       # reference appends all ranks to one file (main.py:32)
    metrics_jsonl: str = ""                # machine-readable per-epoch metrics
    step_timers: bool = False              # per-phase HIP-event step times in the metrics
    num_workers: int = 2                   # native decode/prefetch threads
    eval_lanes: int = 1                    # predictor lanes in the eval pipeline
    eval_batch: int = 64
    eval_assign: str = "random"            # random (reference) | roundrobin
    eval_topk: int = 0                     # also report top-k accuracy (0 or 1: top-1 only)
    eval_src: int = 0                      # synthetic eval source side (0: the model input size)
    predictions_csv: str = ""              # evaluation pipeline: write Id,Predicted,Probability here
    predict_topk: int = 1                  # ... with the k best classes per row (1..16)
    max_steps: int = 0                     # stop an epoch early (0 = full epoch)
    checksum_every: int = 0                # cross-rank replica checksum period (steps, 0=off)
    timeout_s: float = 1800.0              # rendezvous/collective timeout
    watchdog_s: float = 900.0              # abort a rank with no step progress (0: off)
    reserve_gib: float = 0.0               # grow the allocator by one segment up front
                                           # (engine.reserve_device_memory; NOTES "Slow processes")

    def __post_init__(self) -> None:
        if not self.CHECKPOINT_NAME:
            self.CHECKPOINT_NAME = "checkpoint_{}.pt".format(self.MODEL_NAME)
        if self.MODEL_NAME not in MODEL_NAMES:
            raise ValueError("Invalid model name {!r}; expected one of {}".format(
                self.MODEL_NAME, MODEL_NAMES))
        if self.optimizer not in ("adam", "sgd", "adamw", "lamb", "lars"):
            raise ValueError("optimizer must be adam|sgd|adamw|lamb|lars")
        if not self.trust_coef > 0.0:
            raise ValueError("trust_coef must be > 0")
        if self.lr_schedule not in ("constant", "cosine", "step"):
            raise ValueError("lr_schedule must be constant|cosine|step")
        if self.warmup_steps < 0 or self.lr_decay_steps < 0:
            raise ValueError("warmup_steps and lr_decay_steps must be >= 0")
        if not 0.0 <= self.lr_min_ratio <= 1.0:
            raise ValueError("lr_min_ratio must be in [0, 1]")
        if self.lr_schedule == "step" and (self.lr_decay_steps <= 0 or self.lr_gamma <= 0.0):
            raise ValueError("lr_schedule=step needs lr_decay_steps > 0 and lr_gamma > 0")
        if not self.clip_grad_norm >= 0.0:
            raise ValueError("clip_grad_norm must be >= 0 (0 = off)")
        if self.augment not in ("none", "flip", "rrc"):
            raise ValueError("augment must be none|flip|rrc")
        if not 0.0 < self.aug_scale_min <= 1.0:
            raise ValueError("aug_scale_min must be in (0, 1]")
        if not 0.0 <= self.label_smoothing <= 1.0:
            raise ValueError("label_smoothing must be in [0, 1]")
        if not self.logit_adjust_tau >= 0.0:
            raise ValueError("logit_adjust_tau must be >= 0 (0 = off)")
        if not (self.mixup_alpha >= 0.0 and self.cutmix_alpha >= 0.0):
            raise ValueError("mixup_alpha and cutmix_alpha must be >= 0 (0 = off)")
        if not (0.0 <= self.mix_prob <= 1.0 and 0.0 <= self.mix_switch_prob <= 1.0):
            raise ValueError("mix_prob and mix_switch_prob must be in [0, 1]")
        if not 0.0 <= self.ema_decay < 1.0:
            raise ValueError("ema_decay must be in [0, 1) (0 = off)")
        if self.eval_topk < 0:
            raise ValueError("eval_topk must be >= 0 (0 or 1 = top-1 only)")
        if not 1 <= self.predict_topk <= 16:
            raise ValueError("predict_topk must be in [1, 16]")

    # -----------------------------------------------------------------------------------
    @property
    def recipe_on(self) -> bool:
        """True when a schedule, a warm-up or gradient clipping is configured."""
        return (self.lr_schedule != "constant" or self.warmup_steps > 0
                or self.clip_grad_norm > 0.0)

    @property
    def augment_spec(self) -> Optional[Dict[str, Any]]:
        """The training loader's ``augment`` argument (None when augmentation is off).  The
        seed is the run's, not the rank's: a sample's crop does not depend on the sharding."""
        if self.augment == "none":
            return None
        return dict(kind=self.augment, scale_min=self.aug_scale_min, seed=self.seed)

    @property
    def mix_spec(self) -> Optional[Dict[str, Any]]:
        """The training loader's ``mix`` argument (None when both alphas are 0).  The seed is
        the run's; the batch a sample sits in (and so its partner) is the rank's."""
        if self.mixup_alpha == 0.0 and self.cutmix_alpha == 0.0:
            return None
        return dict(mixup_alpha=self.mixup_alpha, cutmix_alpha=self.cutmix_alpha,
                    prob=self.mix_prob, switch_prob=self.mix_switch_prob, seed=self.seed)

    @property
    def input_hw(self):
        if self.image_size:
            return (self.image_size, self.image_size)
        return (self.HEIGHT, self.WIDTH)

    def to_dict(self) -> Dict[str, Any]:
        return dataclasses.asdict(self)

    @classmethod
    def from_env(cls, **overrides) -> "Config":
        kw: Dict[str, Any] = {}
        for f in fields(cls):
            for key in (_ENV_PREFIX + f.name, _ENV_PREFIX + f.name.upper()):
                if key in os.environ:
                    kw[f.name] = _coerce(f.type, os.environ[key])
                    break
        kw.update(overrides)
        return cls(**kw)

    @classmethod
    def add_arguments(cls, p: argparse.ArgumentParser) -> None:
        for f in fields(cls):
            names = ["--" + f.name]
            alt = "--" + f.name.lower().replace("_", "-")
            if alt != names[0]:
                names.append(alt)
            p.add_argument(*names, dest=f.name, default=None, type=str,
                           help="(default: {})".format(f.default))

    @classmethod
    def from_args(cls, argv: Optional[List[str]] = None, **defaults) -> "Config":
        """Config from command-line flags; ``defaults`` are entry-point defaults (e.g.
        ``log_file="evaluation.log"``) that explicit flags override."""
        p = argparse.ArgumentParser(add_help=True)
        cls.add_arguments(p)
        ns, _unknown = p.parse_known_args(argv)
        kw = {}
        types = {f.name: f.type for f in fields(cls)}
        for k, v in vars(ns).items():
            if v is not None:
                kw[k] = _coerce(types[k], v)
        for k, v in defaults.items():
            kw.setdefault(k, v)
        return cls.from_env(**kw)


def _coerce(tp: Any, value: Any) -> Any:
    if not isinstance(value, str):
        return value
    t = tp if isinstance(tp, str) else getattr(tp, "__name__", str(tp))
    if t == "bool":
        return value.strip().lower() in ("1", "true", "yes", "on", "y")
    if t == "int":
        return int(float(value))
    if t == "float":
        return float(value)
    return value
