"""Fused flat-arena optimizers (Adam, SGD+momentum).

The reference builds ``torch.optim.Adam(model.parameters(), lr=utils.LR)``
(``/root/reference/main.py:125``) and steps it after the gradient average
(``main.py:155``).  Here the whole update is ONE streaming HIP kernel over the flat
fp32 master / gradient / moment buffers of :class:`~mpi_pytorch_amd.parallel.ParamArena`:
it applies the DP ``1/N`` gradient scale, weight decay, the Adam (or SGD-momentum)
update, and writes the bf16 weight shadow that the MFMA kernels read - one HBM pass
instead of per-tensor launches plus a cast pass.

``state_dict()`` / ``load_state_dict()`` speak ``torch.optim.Adam`` / ``torch.optim.SGD``
format exactly (per-parameter ``exp_avg``/``exp_avg_sq``/``step`` or ``momentum_buffer``
in the torchvision layout, ``param_groups`` with ``params`` = indices into
``model.parameters()``), so checkpoints round-trip with the reference's
``helpers.load_checkpoint`` (``helpers.py:10-15``).

Training recipe (beyond the reference, off by default): ``set_schedule`` / ``set_clip``
turn on a per-step learning-rate schedule and global-norm gradient clipping that are
computed on the device from the device step counter, so they cost no host sync and stay
correct under HIP-graph replay.  ``step()`` then runs ``grad_sqnorm`` (only with clipping)
-> ``hyper_update`` -> ``adam_step_dev`` / ``sgd_step_dev``; with the recipe off it
launches exactly the kernels it always did.  With ``k`` the 0-based index of the update
(``step_t`` before it), ``W`` warm-up steps, ``T`` total steps and ``r = lr_min_ratio``:

* ``k < W``:  ``lr = base * (k + 1) / W``;
* constant:   ``lr = base``;
* cosine:     ``lr = base * (r + (1 - r) * 0.5 * (1 + cos(pi * (k - W) / max(1, T - W))))``
  for ``k < T`` and ``base * r`` from ``T`` on;
* step:       ``lr = base * gamma ** floor(k / decay_steps)``.

Clipping is ``torch.nn.utils.clip_grad_norm_`` on the averaged gradient: ``total =
grad_scale * sqrt(sum g^2)`` over the trainable arena, ``coef = min(1, max_norm / (total +
1e-6))`` (exactly 1 when ``total <= max_norm``), and the optimizer scales gradients by
``grad_scale * coef`` before weight decay.  While clipping is on, a step whose ``sum g^2``
is inf / NaN is skipped - weights, moments and bf16 shadow stay bitwise unchanged and the
device counter ``nonfinite_steps`` goes up - but ``step_t`` still advances: a skipped step
counts for the schedule and for Adam's bias correction.

Layer-wise optimizers (beyond the reference): ``FusedAdamW`` (decoupled weight decay),
``FusedLAMB`` and ``FusedLARS`` (a per-parameter trust ratio) run on a segment and chunk
plan over the arena (``build_segment_plan``) that tells the kernels which parameter an
element belongs to.  Per-parameter norms are fixed-order sums (no float atomics), so they
are bitwise reproducible and equal on every data-parallel rank.  These optimizers always go
through the hyper record, and by default (``wd_exclude_1d``) 1-D parameters - BN scale and
shift, biases - get no weight decay and a trust ratio of 1.  ``adam`` and ``sgd`` are
unchanged: coupled L2 decay on every element.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch
import torch.nn as nn

from .ops import functional as Fn
from .ops import ref as _ref
from .parallel.arena import ParamArena

SCHEDULE_KINDS = _ref.SCHEDULE_KINDS


def scheduled_lr(base: float, k: int, kind: str = "constant", warmup_steps: int = 0,
                 total_steps: int = 0, lr_min_ratio: float = 0.0, gamma: float = 0.1,
                 decay_steps: int = 0) -> float:
    """The schedule in host float64 (the module docstring's formulas) for update index
    ``k``: what the device record holds to fp32 rounding.  For logs and tests."""
    import math
    W, T, r = warmup_steps, total_steps, lr_min_ratio
    if k < W:
        return base * (k + 1) / W
    if kind == "cosine":
        if k >= T:
            return base * r
        p = (k - W) / max(1, T - W)
        return base * (r + (1 - r) * 0.5 * (1 + math.cos(math.pi * p)))
    if kind == "step":
        return base * gamma ** (k // decay_steps)
    return base


def _export(p, t):
    f = getattr(p, "_mpa_export", None)
    return f(t) if f is not None else t


def _import(p, t):
    f = getattr(p, "_mpa_import", None)
    return f(t) if f is not None else t


class _FlatOptimizer:
    kind = "base"

    def __init__(self, params: List[nn.Parameter], arena: ParamArena):
        self.params = list(params)
        self.arena = arena
        dev = arena.device
        self.step_t = torch.zeros(1, dtype=torch.float32, device=dev)
        self.grad_scale = 1.0
        # the recipe's device record (ops/ref.py HYPER_*: lr, effective grad scale, grad
        # norm, clip coefficient, skip flag, non-finite step count, sum of squares) and the
        # norm's per-block workspace: tensor attributes, so TrainStep snapshots / restores
        # them around graph capture with the rest of the optimizer state
        self.hyper = None
        self.norm_ws = None
        self._schedule: Optional[Dict] = None
        self._max_norm = 0.0
        self.param_groups = [self._group_defaults()]
        self.param_groups[0]["params"] = self.params

    # torch.optim-like surface ------------------------------------------------------
    def zero_grad(self, set_to_none: bool = False) -> None:
        self.arena.zero_grad()

    @property
    def lr(self) -> float:
        return self.param_groups[0]["lr"]

    @lr.setter
    def lr(self, v: float) -> None:
        self.param_groups[0]["lr"] = v

    def _group_defaults(self) -> Dict:
        raise NotImplementedError

    def _update(self, lo: int, hi: int) -> None:
        raise NotImplementedError

    def _update_dev(self, lo: int, hi: int) -> None:
        raise NotImplementedError

    # training recipe -----------------------------------------------------------------
    @property
    def recipe_on(self) -> bool:
        return self._schedule is not None or self._max_norm > 0.0

    def _ensure_record(self) -> None:
        if self.hyper is None:
            dev = self.arena.device
            k = self._kernel()
            self.hyper = torch.zeros(_ref.HYPER_N, dtype=torch.float32, device=dev)
            self.hyper[_ref.HYPER_LR] = float(self.lr)
            self.hyper[_ref.HYPER_SCALE] = float(self.grad_scale)
            self.hyper[_ref.HYPER_COEF] = 1.0
            self.norm_ws = torch.zeros(int(k.grad_sqnorm_grid_cap()), dtype=torch.float32,
                                       device=dev)

    def set_schedule(self, kind: str = "constant", warmup_steps: int = 0, total_steps: int = 0,
                     lr_min_ratio: float = 0.0, gamma: float = 0.1, decay_steps: int = 0) -> None:
        """Per-step learning-rate schedule computed on the device (module docstring).
        Set it before a step is captured into a HIP graph: the schedule's constants are
        kernel arguments, only the step counter and the gradients are read per replay."""
        if kind not in SCHEDULE_KINDS:
            raise ValueError("schedule must be one of {}".format("|".join(SCHEDULE_KINDS)))
        if warmup_steps < 0 or total_steps < 0 or decay_steps < 0:
            raise ValueError("warmup_steps, total_steps and decay_steps must be >= 0")
        if not 0.0 <= lr_min_ratio <= 1.0:
            raise ValueError("lr_min_ratio must be in [0, 1]")
        if kind == "step" and (decay_steps <= 0 or gamma <= 0.0):
            raise ValueError("the step schedule needs decay_steps > 0 and gamma > 0")
        if kind == "cosine" and total_steps <= warmup_steps:
            raise ValueError("the cosine schedule needs total_steps > warmup_steps")
        self._schedule = dict(kind=str(kind), warmup_steps=int(warmup_steps),
                              total_steps=int(total_steps), lr_min_ratio=float(lr_min_ratio),
                              gamma=float(gamma), decay_steps=int(decay_steps))
        self._ensure_record()

    def set_clip(self, max_norm: float) -> None:
        """Clip the global norm of the averaged gradient to ``max_norm`` (0 turns it off)."""
        if max_norm < 0 or max_norm != max_norm:
            raise ValueError("max_norm must be >= 0")
        self._max_norm = float(max_norm)
        if self._max_norm > 0:
            self._ensure_record()

    def _recipe_step(self) -> None:
        """norm (only with clipping) -> hyper record -> device-argument update."""
        self._hyper_step()
        self._update_dev(0, self.arena.n_train)

    def _hyper_step(self) -> None:
        n = self.arena.n_train
        k = self._kernel()
        nparts = 0
        if self._max_norm > 0.0:
            nparts = int(k.grad_sqnorm(self.arena.grad[:n], self.norm_ws))
        sc = self._schedule or dict(kind="constant", warmup_steps=0, total_steps=0,
                                    lr_min_ratio=0.0, gamma=0.1, decay_steps=0)
        k.hyper_update(self.step_t, self.hyper, self.norm_ws, nparts,
                       SCHEDULE_KINDS.index(sc["kind"]), float(self.lr),
                       float(sc["warmup_steps"]), float(sc["total_steps"]),
                       float(sc["lr_min_ratio"]), float(sc["gamma"]), float(sc["decay_steps"]),
                       float(self._max_norm), float(self.grad_scale))

    def step(self) -> None:
        if self.arena.n_train == 0:
            return
        if self.recipe_on:
            self._recipe_step()
        else:
            self._update(0, self.arena.n_train)
        self.arena.refresh_transposed(step_inc=self.step_t)

    def _read(self, slot: int) -> float:
        if self.hyper is None:
            raise RuntimeError("no schedule or clipping is set on this optimizer")
        return float(self.hyper[slot].item())

    def current_lr(self) -> float:
        """The learning rate the last update used (the base LR before any; one host sync)."""
        return self._read(_ref.HYPER_LR) if self.hyper is not None else float(self.lr)

    def last_grad_norm(self) -> float:
        """Global norm of the last step's averaged gradient, before clipping (one sync)."""
        return self._read(_ref.HYPER_NORM)

    def nonfinite_steps(self) -> int:
        """Updates skipped so far for inf / NaN gradients (one sync)."""
        return int(self._read(_ref.HYPER_NONFINITE))

    def _kernel(self):
        return Fn.K(self.arena.master)

    def _shadow(self):
        s = self.arena.train_shadow()
        return s if s is not None else torch.empty(0, device=self.arena.device)

    def state_dict(self) -> Dict:
        state = {}
        torch_step = float(self.step_t.item())
        for i, p in enumerate(self.params):
            if not p.requires_grad or torch_step == 0:
                continue
            o, e = self.arena.slice_of(p)
            state[i] = self._param_state(p, o, e, torch_step)
        g = {k: v for k, v in self.param_groups[0].items() if k != "params"}
        g["params"] = list(range(len(self.params)))
        g["mpa_step"] = torch_step
        if self.recipe_on:  # plain Python types only (weights_only=True loading)
            g["initial_lr"] = float(self.lr)
            g["lr"] = self.current_lr()  # the last scheduled value, as torch schedulers leave it
            g["mpa_schedule"] = dict(self._schedule) if self._schedule is not None else None
            g["mpa_clip_grad_norm"] = float(self._max_norm)
            g["mpa_nonfinite_steps"] = self.nonfinite_steps()
        return {"state": state, "param_groups": [g]}

    def load_state_dict(self, sd: Dict) -> None:
        g = sd["param_groups"][0]
        for k, v in g.items():
            if k != "params" and not k.startswith("mpa_") and k != "initial_lr":
                self.param_groups[0][k] = v
        if "initial_lr" in g:  # a recipe checkpoint's "lr" is the last scheduled value
            self.param_groups[0]["lr"] = float(g["initial_lr"])
        if g.get("mpa_schedule") is not None:
            self.set_schedule(**g["mpa_schedule"])
        if g.get("mpa_clip_grad_norm", 0.0) > 0.0:
            self.set_clip(g["mpa_clip_grad_norm"])
        if self.hyper is not None:
            self.hyper[_ref.HYPER_LR] = float(g.get("lr", self.lr))
            self.hyper[_ref.HYPER_NONFINITE] = float(g.get("mpa_nonfinite_steps", 0))
        steps = []
        for i, st in sd["state"].items():
            p = self.params[int(i)]
            if not p.requires_grad:
                continue
            o, e = self.arena.slice_of(p)
            steps.append(self._load_param_state(p, o, e, st))
        if "mpa_step" in g:  # (SGD's per-parameter state carries no step)
            self.step_t.fill_(float(g["mpa_step"]))
        elif steps:
            self.step_t.fill_(max(steps))


class FusedAdam(_FlatOptimizer):
    kind = "adam"

    def __init__(self, params, arena: ParamArena, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=0.0):
        self._init = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay)
        super().__init__(params, arena)
        n = max(arena.n_train, 1)
        self.exp_avg = torch.zeros(n, dtype=torch.float32, device=arena.device)
        self.exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=arena.device)

    def _group_defaults(self):
        d = dict(self._init)
        d.update(amsgrad=False, maximize=False, foreach=None, capturable=False,
                 differentiable=False, fused=None)
        return d

    def _update(self, lo: int, hi: int) -> None:
        g = self.param_groups[0]
        b1, b2 = g["betas"]
        sh = self._shadow()
        self._kernel().adam_step(self.arena.master[lo:hi], self.arena.grad[lo:hi],
                                 self.exp_avg[lo:hi], self.exp_avg_sq[lo:hi],
                                 sh[lo:hi] if sh.numel() else sh, self.step_t,
                                 float(g["lr"]), float(b1), float(b2), float(g["eps"]),
                                 float(g["weight_decay"]), float(self.grad_scale))

    def _update_dev(self, lo: int, hi: int) -> None:
        g = self.param_groups[0]
        b1, b2 = g["betas"]
        sh = self._shadow()
        self._kernel().adam_step_dev(self.arena.master[lo:hi], self.arena.grad[lo:hi],
                                     self.exp_avg[lo:hi], self.exp_avg_sq[lo:hi],
                                     sh[lo:hi] if sh.numel() else sh, self.step_t, self.hyper,
                                     float(b1), float(b2), float(g["eps"]),
                                     float(g["weight_decay"]))

    def _param_state(self, p, o, e, step):
        return {"step": torch.tensor(step),
                "exp_avg": _export(p, self.exp_avg[o:e].view(p.shape)).detach().cpu().clone(),
                "exp_avg_sq": _export(p, self.exp_avg_sq[o:e].view(p.shape)).detach().cpu().clone()}

    def _load_param_state(self, p, o, e, st):
        self.exp_avg[o:e].copy_(_import(p, st["exp_avg"].to(self.exp_avg.device)).reshape(-1))
        self.exp_avg_sq[o:e].copy_(_import(p, st["exp_avg_sq"].to(self.exp_avg.device)).reshape(-1))
        s = st.get("step", 0)
        return float(s.item() if torch.is_tensor(s) else s)


class FusedSGD(_FlatOptimizer):
    kind = "sgd"

    def __init__(self, params, arena: ParamArena, lr=0.1, momentum=0.9, dampening=0.0,
                 weight_decay=0.0, nesterov=False):
        self._init = dict(lr=lr, momentum=momentum, dampening=dampening,
                          weight_decay=weight_decay, nesterov=nesterov)
        super().__init__(params, arena)
        self.momentum_buffer = torch.zeros(max(arena.n_train, 1), dtype=torch.float32,
                                           device=arena.device)

    def _group_defaults(self):
        d = dict(self._init)
        d.update(maximize=False, foreach=None, differentiable=False, fused=None)
        return d

    def _update(self, lo: int, hi: int) -> None:
        g = self.param_groups[0]
        sh = self._shadow()
        self._kernel().sgd_step(self.arena.master[lo:hi], self.arena.grad[lo:hi],
                                self.momentum_buffer[lo:hi], sh[lo:hi] if sh.numel() else sh,
                                self.step_t, float(g["lr"]), float(g["momentum"]),
                                float(g["dampening"]), float(g["weight_decay"]),
                                bool(g["nesterov"]), float(self.grad_scale))

    def _update_dev(self, lo: int, hi: int) -> None:
        g = self.param_groups[0]
        sh = self._shadow()
        self._kernel().sgd_step_dev(self.arena.master[lo:hi], self.arena.grad[lo:hi],
                                    self.momentum_buffer[lo:hi],
                                    sh[lo:hi] if sh.numel() else sh, self.step_t, self.hyper,
                                    float(g["momentum"]), float(g["dampening"]),
                                    float(g["weight_decay"]), bool(g["nesterov"]))

    def _param_state(self, p, o, e, step):
        return {"momentum_buffer":
                _export(p, self.momentum_buffer[o:e].view(p.shape)).detach().cpu().clone()}

    def _load_param_state(self, p, o, e, st):
        mb = st.get("momentum_buffer")
        if mb is not None:
            self.momentum_buffer[o:e].copy_(_import(p, mb.to(self.momentum_buffer.device)).reshape(-1))
        return 1.0


# ------------------------------------------------------- layer-wise: AdamW / LAMB / LARS
def build_segment_plan(arena: ParamArena, wd_exclude_1d: bool = True,
                       chunk: Optional[int] = None):
    """The segment and chunk plan of ``arena``'s trainable region, as CPU tensors.

    ``seg`` [nseg][5] int64 = (offset, aligned length, first chunk, chunk count, flags):
    segment ``s`` is the aligned slice of ``arena.trainable[s]`` (grouped parameters stay
    one segment each), so the segments tile ``[0, n_train)`` and start on ``ALIGN``
    boundaries.  ``chunk_seg`` [nchunks] int32: each segment is cut into consecutive chunks
    of at most ``chunk`` elements (the kernels' ``seg_chunk()``), none crossing a segment.
    Flags: ``SEG_DECAY`` (weight decay applies) and ``SEG_ADAPT`` (a trust ratio applies);
    with ``wd_exclude_1d`` parameters stored with ``ndim <= 1`` (BN scale / shift, biases -
    a ``pad_out`` bias is still 1-D) get neither."""
    from .parallel.arena import _align
    chunk = int(_ref.seg_chunk() if chunk is None else chunk)
    rows, chunk_seg, off = [], [], 0
    for s, p in enumerate(arena.trainable):
        assert arena.offsets[id(p)] == off, "trainable parameters must tile the arena"
        ln = _align(p.numel())
        nch = (ln + chunk - 1) // chunk
        flags = 0 if (wd_exclude_1d and p.ndim <= 1) else _ref.SEG_DECAY | _ref.SEG_ADAPT
        rows.append([off, ln, len(chunk_seg), nch, flags])
        chunk_seg.extend([s] * nch)
        off += ln
    assert off == arena.n_train
    seg = torch.tensor(rows, dtype=torch.int64).reshape(-1, _ref.SEG_COLS)
    return seg, torch.tensor(chunk_seg, dtype=torch.int32)


class _Layerwise:
    """Mixin over a flat optimizer: the segment plan, per-parameter fixed-order norms and
    trust ratios, and the ``step()`` that always goes through the hyper record.

    ``step()``: ``grad_sqnorm`` (only with clipping) -> ``hyper_update`` -> norms ->
    ``trust_ratio`` -> update -> ``refresh_transposed(step_inc=...)``.  Plan, partials,
    ratios and norms are tensor attributes, so ``TrainStep`` snapshots and restores them
    around graph capture with the rest of the optimizer state."""
    trust_mode: Optional[int] = None  # ref.TRUST_LAMB | ref.TRUST_LARS | None (no ratio)

    def _init_plan(self, trust_coef: float, wd_exclude_1d: bool) -> None:
        self.trust_coef = float(trust_coef)
        self.wd_exclude_1d = bool(wd_exclude_1d)
        dev = self.arena.device
        k = self._kernel()
        seg, chunk_seg = build_segment_plan(self.arena, self.wd_exclude_1d, int(k.seg_chunk()))
        self.plan_seg = seg.to(dev)
        self.plan_chunk_seg = chunk_seg.to(dev)
        nseg, nch = seg.shape[0], chunk_seg.numel()
        # the CPU twins accumulate (and keep) the norms' partials in float64
        pt = torch.float32 if dev.type == "cuda" else torch.float64
        self.seg_part = torch.zeros(2, max(nch, 1), dtype=pt, device=dev)
        self.seg_ratio = torch.ones(max(nseg, 1), dtype=torch.float32, device=dev)
        self.seg_norms = torch.zeros(max(nseg, 1), 2, dtype=torch.float32, device=dev)
        self._ensure_record()

    def _layerwise_update(self, n: int) -> None:
        raise NotImplementedError

    def _trust_ratio(self) -> None:
        g = self.param_groups[0]
        self._kernel().trust_ratio(self.plan_seg, self.plan_chunk_seg, self.seg_part[0],
                                   self.seg_part[1], self.hyper, int(self.trust_mode),
                                   float(self.trust_coef), float(g["weight_decay"]),
                                   self.seg_ratio, self.seg_norms)

    def step(self) -> None:
        n = self.arena.n_train
        if n == 0:
            return
        self._hyper_step()
        self._layerwise_update(n)
        self.arena.refresh_transposed(step_inc=self.step_t)

    def last_trust_ratios(self) -> Dict[str, float]:
        """{parameter name: trust ratio of the last update} (1.0 before any update, for
        parameters without a ratio, and always for AdamW); one host sync."""
        r = self.seg_ratio.cpu().tolist()
        a = self.arena
        return {a.names[id(p)]: r[s] for s, p in enumerate(a.trainable)}

    def last_param_norms(self) -> Dict[str, tuple]:
        """{parameter name: (|p|, |u| or |g^|)} of the last update's norms (one sync)."""
        nv = self.seg_norms.cpu().tolist()
        a = self.arena
        return {a.names[id(p)]: tuple(nv[s]) for s, p in enumerate(a.trainable)}

    def state_dict(self) -> Dict:
        sd = super().state_dict()
        g = sd["param_groups"][0]
        g["mpa_trust_coef"] = float(self.trust_coef)
        g["mpa_wd_exclude_1d"] = bool(self.wd_exclude_1d)
        return sd

    def load_state_dict(self, sd: Dict) -> None:
        g = sd["param_groups"][0]
        super().load_state_dict(sd)
        self.trust_coef = float(g.get("mpa_trust_coef", self.trust_coef))
        ex = bool(g.get("mpa_wd_exclude_1d", self.wd_exclude_1d))
        if ex != self.wd_exclude_1d:  # the flags are part of the plan: rebuild it in place
            self.wd_exclude_1d = ex
            seg, _ = build_segment_plan(self.arena, ex, int(self._kernel().seg_chunk()))
            self.plan_seg.copy_(seg)


class FusedAdamW(_Layerwise, FusedAdam):
    """``torch.optim.AdamW``: decoupled weight decay, by default not on 1-D parameters."""
    kind = "adamw"

    def __init__(self, params, arena: ParamArena, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=1e-2, trust_coef=0.001, wd_exclude_1d=True):
        FusedAdam.__init__(self, params, arena, lr=lr, betas=betas, eps=eps,
                           weight_decay=weight_decay)
        self._init_plan(trust_coef, wd_exclude_1d)

    def _group_defaults(self):
        d = FusedAdam._group_defaults(self)
        d["decoupled_weight_decay"] = True
        return d

    def _adam_args(self):
        g = self.param_groups[0]
        b1, b2 = g["betas"]
        return float(b1), float(b2), float(g["eps"]), float(g["weight_decay"])

    def _step_kernel(self, n: int, adamw: bool) -> None:
        a, sh = self.arena, self._shadow()
        self._kernel().lamb_step_dev(a.master[:n], a.grad[:n], self.exp_avg[:n],
                                     self.exp_avg_sq[:n], sh[:n] if sh.numel() else sh,
                                     self.step_t, self.hyper, self.plan_seg,
                                     self.plan_chunk_seg, self.seg_ratio, *self._adam_args(),
                                     adamw)

    def _layerwise_update(self, n: int) -> None:
        self._step_kernel(n, True)


class FusedLAMB(FusedAdamW):
    """LAMB (You et al. 2020, with bias correction): Adam's direction plus decoupled decay,
    scaled per parameter by ``|p| / |u|``.  Stage 1 norms the update the step would apply,
    stage 2 recomputes and applies it: no update buffer, the gradient arena stays intact."""
    kind = "lamb"
    trust_mode = _ref.TRUST_LAMB

    def _layerwise_update(self, n: int) -> None:
        a = self.arena
        self._kernel().lamb_norms(a.master[:n], a.grad[:n], self.exp_avg[:n],
                                  self.exp_avg_sq[:n], self.step_t, self.hyper, self.plan_seg,
                                  self.plan_chunk_seg, self.seg_part[0], self.seg_part[1],
                                  *self._adam_args())
        self._trust_ratio()
        self._step_kernel(n, False)


class FusedLARS(_Layerwise, FusedSGD):
    """LARS (You et al. 2017) on SGD-momentum: per parameter ``g' = ratio * (g^ + wd * p)``
    with ``ratio = trust_coef * |p| / (|g^| + wd * |p| + 1e-8)``, ``g^`` the averaged,
    clipped gradient."""
    kind = "lars"
    trust_mode = _ref.TRUST_LARS

    def __init__(self, params, arena: ParamArena, lr=0.1, momentum=0.9, dampening=0.0,
                 weight_decay=0.0, nesterov=False, trust_coef=0.001, wd_exclude_1d=True):
        FusedSGD.__init__(self, params, arena, lr=lr, momentum=momentum, dampening=dampening,
                          weight_decay=weight_decay, nesterov=nesterov)
        self._init_plan(trust_coef, wd_exclude_1d)

    def _layerwise_update(self, n: int) -> None:
        a, k, g, sh = self.arena, self._kernel(), self.param_groups[0], self._shadow()
        k.seg_sqnorm(a.master[:n], self.plan_seg, self.plan_chunk_seg, self.hyper, False,
                     self.seg_part[0])
        k.seg_sqnorm(a.grad[:n], self.plan_seg, self.plan_chunk_seg, self.hyper, True,
                     self.seg_part[1])
        self._trust_ratio()
        k.lars_step_dev(a.master[:n], a.grad[:n], self.momentum_buffer[:n],
                        sh[:n] if sh.numel() else sh, self.step_t, self.hyper, self.plan_seg,
                        self.plan_chunk_seg, self.seg_ratio, float(g["momentum"]),
                        float(g["dampening"]), float(g["weight_decay"]), bool(g["nesterov"]))


OPTIMIZERS = ("adam", "sgd", "adamw", "lamb", "lars")


def build_optimizer(name: str, model: nn.Module, lr: float, momentum: float = 0.9,
                    weight_decay: float = 0.0, trust_coef: float = 0.001,
                    wd_exclude_1d: bool = True):
    """``trust_coef`` (LARS) and ``wd_exclude_1d`` apply to adamw | lamb | lars only."""
    arena = model._mpa_arena
    params = list(model.parameters())
    if name == "adam":
        return FusedAdam(params, arena, lr=lr, weight_decay=weight_decay)
    if name == "sgd":
        return FusedSGD(params, arena, lr=lr, momentum=momentum, weight_decay=weight_decay)
    if name in ("adamw", "lamb"):
        cls = FusedAdamW if name == "adamw" else FusedLAMB
        return cls(params, arena, lr=lr, weight_decay=weight_decay, trust_coef=trust_coef,
                   wd_exclude_1d=wd_exclude_1d)
    if name == "lars":
        return FusedLARS(params, arena, lr=lr, momentum=momentum, weight_decay=weight_decay,
                         trust_coef=trust_coef, wd_exclude_1d=wd_exclude_1d)
    raise ValueError("optimizer must be one of {}, got {!r}".format("|".join(OPTIMIZERS), name))
