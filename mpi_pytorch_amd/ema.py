"""Exponential moving average of the weights on the flat arena (timm's ``ModelEma``,
``torch.optim.swa_utils.AveragedModel`` with ``get_ema_multi_avg_fn``).

The averaged weights, not the last iterate, are what large-batch recipes validate,
checkpoint and ship.  The weights live in :class:`~mpi_pytorch_amd.parallel.ParamArena`
(fp32 masters, a bf16 shadow, a transposed shadow), so the average is ONE streaming HIP
kernel over the trainable masters ``[0, n_train)`` plus ONE launch over the model's
floating-point buffers (BN running statistics, separate small tensors reached through a
device table built once).  Per element, every operation rounded on its own in fp32::

    t   = step_t                  # updates completed (the optimizer's device counter)
    d_t = min(decay, (1 + t) / (10 + t)) if warmup else decay
    ema = ema + (1 - d_t) * (p - ema)

``t`` is read on the device, so a captured HIP graph replays the warm-up.  Frozen
parameters are not averaged (they never change) and integer buffers
(``num_batches_tracked``) are not either.  Every data-parallel rank keeps its own average
and nothing is communicated: identical weights give identical averages.
"""
from __future__ import annotations

import contextlib
from typing import Dict, List

import torch
import torch.nn as nn

from .ops import functional as Fn
from .ops import ref as _ref
from .parallel.arena import ALIGN, ParamArena, _align


class ModelEMA:
    """The average of ``model``'s trainable parameters and floating-point buffers.

    ``update()`` runs right after ``optimizer.step()`` (``TrainStep`` calls it inside the
    "opt" phase, so it lands inside a captured graph).  A step that the recipe skips for a
    non-finite gradient still averages the (unchanged) weights and counts for the warm-up,
    as ``AveragedModel.update_parameters`` after a skipped ``optimizer.step()`` does.

    ``ema`` (fp32, the arena's trainable region) and ``ema_buf`` (fp32, the buffers' slots,
    each ``ALIGN``-aligned) are the state; ``table`` [nbuf][3] int64 = (source address,
    offset into ``ema_buf``, length) is what ``ema_update_multi`` reads, ``table_host`` its
    CPU twin.  The table holds addresses: the model's buffers must stay where they are
    (in-place loads keep them there; ``model.to(...)`` needs a new ``ModelEMA``)."""

    def __init__(self, model: nn.Module, optimizer, decay: float, warmup: bool = True):
        if not 0.0 <= decay < 1.0:
            raise ValueError("ema decay must be in [0, 1), got {!r}".format(decay))
        self.model = model
        self.arena: ParamArena = model._mpa_arena
        self.decay = float(decay)
        self.warmup = bool(warmup)
        self.step_t = optimizer.step_t  # (loads fill it in place: the reference stays valid)
        dev = self.arena.device
        self.ema = torch.zeros(max(self.arena.n_train, ALIGN), dtype=torch.float32, device=dev)
        self.buffers: List[torch.Tensor] = []
        seen, rows, off = set(), [], 0
        for name, b in model.named_buffers():
            if not b.is_floating_point() or id(b) in seen:
                continue
            seen.add(id(b))
            if b.dtype != torch.float32 or not b.is_contiguous() or b.device != dev:
                raise ValueError("ModelEMA: buffer {} must be contiguous fp32 on {}".format(
                    name, dev))
            self.buffers.append(b)
            rows.append([b.data_ptr(), off, b.numel()])
            off += _align(b.numel())
        self.ema_buf = torch.zeros(max(off, ALIGN), dtype=torch.float32, device=dev)
        self.table_host = torch.tensor(rows, dtype=torch.int64).reshape(-1, _ref.EMA_COLS)
        self.table = self.table_host.to(dev)
        self.reset()

    def _slots(self):
        for (_a, off, ln), b in zip(self.table_host.tolist(), self.buffers):
            yield self.ema_buf[off:off + ln], b

    @torch.no_grad()
    def reset(self) -> None:
        """Start the average from the current masters and buffers (after a checkpoint load
        and ``sync_params``, so every rank starts from the synced weights)."""
        n = self.arena.n_train
        self.ema[:n].copy_(self.arena.master[:n])
        for slot, b in self._slots():
            slot.copy_(b.reshape(-1))

    def update(self) -> None:
        """The two kernels, nothing else (the CPU path runs their oracles)."""
        n = self.arena.n_train
        k = Fn.K(self.arena.master)
        if n:
            k.ema_update(self.ema[:n], self.arena.master[:n], self.step_t, self.decay,
                         self.warmup)
        if self.buffers:
            k.ema_update_multi(self.ema_buf, self.table, self.table_host, self.buffers,
                               self.step_t, self.decay, self.warmup)

    # ------------------------------------------------------------------ the averaged model
    @torch.no_grad()
    def _load_averages(self) -> None:
        n = self.arena.n_train
        self.arena.master[:n].copy_(self.ema[:n])
        for slot, b in self._slots():
            b.copy_(slot.view_as(b))

    @contextlib.contextmanager
    def swapped_in(self):
        """The model with the averages in place of the live weights, for epoch-boundary use
        (validation, export): saves the live masters ``[0, n_train)`` and float buffers,
        copies the averages in and refreshes the bf16 / transposed shadows; on exit - also
        when the body raises - restores them and refreshes the shadows again, so masters,
        shadows and buffers are bitwise what they were.  Inside, ``model(x)`` and
        ``model.state_dict()`` see the averaged model (torchvision names, OIHW weights)."""
        n = self.arena.n_train
        with torch.no_grad():
            live = self.arena.master[:n].clone()
            live_bufs = [b.clone() for b in self.buffers]
            self._load_averages()
            self.arena.sync_shadow()
        try:
            yield self.model
        finally:
            with torch.no_grad():
                self.arena.master[:n].copy_(live)
                for b, c in zip(self.buffers, live_bufs):
                    b.copy_(c)
                self.arena.sync_shadow()

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """``model.state_dict()`` of the averaged model (copies)."""
        with self.swapped_in():
            sd = self.model.state_dict()
            return type(sd)((k, v.detach().clone()) for k, v in sd.items())

    @torch.no_grad()
    def load_state_dict(self, sd) -> None:
        """The reverse of :meth:`state_dict`: the average becomes ``sd``'s weights and float
        buffers; the live model (frozen weights and batch counts included) is left as it
        was."""
        live = self.arena.master.clone()
        live_bufs = [(b, b.clone()) for b in self.model.buffers()]
        hosts = [(m, m._batches_host) for m in self.model.modules()
                 if hasattr(m, "_batches_host")]
        try:
            self.model.load_state_dict(sd)
            self.reset()
        finally:
            self.arena.master.copy_(live)
            for b, c in live_bufs:
                b.copy_(c)
            for m, h in hosts:
                m._batches_host = h
            self.arena.sync_shadow()
