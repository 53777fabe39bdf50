"""Autograd functions over the kernel API (NHWC activations, fused epilogues).

Each function dispatches on the activation's device: CUDA/HIP tensors go to the native
gfx950 kernels (``mpi_pytorch_amd._C``; missing extension => loud error), CPU tensors to
``ops/ref.py``.  The ops the reference reaches through ATen map to:

* ``conv_bn_act``   conv (implicit-GEMM MFMA, BN batch statistics accumulated in the conv
                    epilogue) -> BN apply (+ residual add) (+ ReLU)  [K1-K5, K8]
* ``conv_act``      conv + bias (+ ReLU) epilogue                     [K1, K5]
* ``bn_act``        standalone BN (+ReLU) for pre-activation nets (DenseNet)  [K4]
* ``linear_act``    Linear + bias (+ ReLU) on the same MFMA engine   [K9]
* ``max_pool2d``, ``avg_pool2d``, ``adaptive_avg_pool2d``            [K6, K7]
* ``dropout``                                                        [K14]
* ``cross_entropy`` fused log-softmax + NLL (mean), grad recomputed from saved LSE  [K10]

Parameter gradients never travel through autograd: backward kernels accumulate them in
fp32 directly into the flat gradient arena (``p.grad``) and then signal the DP bucketer
(``grad_done``), which may start that bucket's all-reduce immediately.  Parameters are
still autograd *inputs* so that backward reaches the first layer even though the image
tensor does not require grad.
"""
from __future__ import annotations

import os
from typing import Optional, Tuple

import numpy as np
import torch

from . import ref
from . import _ext
from ..parallel.arena import weight_of, weight_t_of, grad_sink, grad_done

_EMPTY = {}
_NO_SHIFT = os.environ.get("MPA_NO_STATS_SHIFT", "0") == "1"  # diagnostics only


def K(t: torch.Tensor):
    """Kernel namespace for a tensor's device."""
    if t.is_cuda:
        return _ext.ext()
    return ref


def _empty(t: torch.Tensor) -> torch.Tensor:
    key = (t.device, torch.float32)
    e = _EMPTY.get(key)
    if e is None:
        e = torch.empty(0, device=t.device, dtype=torch.float32)
        _EMPTY[key] = e
    return e


def _or_empty(x: Optional[torch.Tensor], like: torch.Tensor) -> torch.Tensor:
    return x if x is not None else _empty(like)


def _sink(p: Optional[torch.nn.Parameter], like: torch.Tensor) -> torch.Tensor:
    if p is None:
        return _empty(like)
    s = grad_sink(p)
    return s if s is not None else _empty(like)


def _fresh(p: torch.nn.Parameter) -> bool:
    """Whether ``p``'s arena gradient is untouched since zero_grad (consumed by the call)."""
    a = getattr(p, "_mpa_arena", None)
    return a.take_fresh(p) if a is not None else False


def _done(*ps) -> None:
    for p in ps:
        if p is not None:
            grad_done(p)


def _grads(fn, *grads):
    """A backward's return value: ``grads`` for the leading inputs of ``fn.forward``, None for
    every other argument."""
    return grads + (None,) * (fn.forward.__code__.co_argcount - 1 - len(grads))


# ================================================================ weight-gradient stream
# Inside TrainStep's eager backward (single GPU; MPA_WGRAD_STREAM=0 turns it off), the conv
# weight gradients run on a second HIP stream (+4 % ResNet-18, +2.7 % VGG-16 measured,
# profiles/ab_r4.txt).  A weight gradient reads only its op's dz and x and
# writes only the gradient arena, so it need not sit between the dgrad / BN-backward
# launches of the main chain: the memory-bound BN passes (no LDS, or 8 KiB) can run on the
# CUs beside a persistent MFMA-bound wgrad grid.  The step joins the stream before the
# optimizer (join_wgrad_stream); x / dz are record_stream'ed so the caching allocator does
# not hand their memory out while the side stream still reads it.
_WGRAD_STREAM = os.environ.get("MPA_WGRAD_STREAM", "1") == "1"
# (Linear weight gradients stay on the compute stream: on the side stream AlexNet lost
# 4.7 %, its three large FC weight gradients contending with the FC dgrads; round-4 A/B,
# profiles/ab_r4.txt call 21.)
_SIDE = {"stream": None, "on": False, "used": False}


def _capture_blocks_streams() -> bool:
    """A HIP-graph capture keeps one stream: replaying a multi-stream graph measured slower
    than the one-stream graph, and both slower than eager with streams (DenseNet-121 8.93k /
    9.07k / 9.53k img/s, profiles/ab_r4.txt call 15)."""
    return torch.cuda.is_current_stream_capturing()


# Halo weight-gradient form per step (unless MPA_HALO_WPROD pins it): the 4-wave kernel
# while the weight gradients run on the side stream, the producer-wave kernel when they
# share the compute stream (data parallelism).  Same-box round-5 A/B, ResNet-18 b1024:
# side stream 51.9k (4-wave) vs 51.0k (producer waves) img/s, one stream 50.4k vs 50.7k
# (profiles/halo_sched_r5.txt).
_WPROD_PINNED = "MPA_HALO_WPROD" in os.environ


def _halo_wgrad_form(side_on: bool) -> None:
    if not _WPROD_PINNED:
        _ext.ext().igemm_set_halo_wprod(0 if side_on else 1)


def wgrad_stream_begin(enabled: bool = True) -> None:
    """Route the following conv weight gradients to the side stream (TrainStep backward)."""
    _SIDE["on"] = bool(enabled and _WGRAD_STREAM)
    if torch.cuda.is_available():
        _halo_wgrad_form(_SIDE["on"])
        if _SIDE["on"]:
            _SIDE["main"] = torch.cuda.current_stream()


def wgrad_streams():
    """(compute stream, side stream) while side-stream weight gradients are routed and the
    side stream exists, else None: a gradient bucket launched then must wait for both
    (parallel/ddp.py GradBucketer._launch)."""
    if _SIDE["on"] and _SIDE["stream"] is not None and _SIDE.get("main") is not None:
        return _SIDE["main"], _SIDE["stream"]
    return None


def join_wgrad_stream() -> None:
    """Make the current stream wait for every side-stream weight gradient; route off."""
    _SIDE["on"] = False
    if _SIDE["used"]:
        torch.cuda.current_stream().wait_stream(_SIDE["stream"])
        _SIDE["used"] = False


def _run_wgrad(fn, *tensors) -> None:
    """Run ``fn`` (a weight-gradient launch and its arena notifications) on the side stream
    when routing is on, else in place."""
    t0 = tensors[0]
    if not (_SIDE["on"] and t0.is_cuda) or _capture_blocks_streams():
        fn()
        return
    main = torch.cuda.current_stream()
    side = _SIDE["stream"]
    if side is None or side.device != t0.device:
        side = _SIDE["stream"] = torch.cuda.Stream(t0.device)
    side.wait_stream(main)
    # (set_stream / restore instead of the torch.cuda.stream context: ~20 us less host
    # time per weight gradient, which the host-bound small-batch step feels)
    torch.cuda.set_stream(side)
    try:
        fn()
    finally:
        torch.cuda.set_stream(main)
    for t in tensors:
        t.record_stream(side)
    _SIDE["used"] = True


def _conv_wgrad(k, g, x, w, conv) -> None:
    """``conv``'s weight gradient of the output gradient ``g`` into ``w.grad`` (and its arena
    notifications), through ``_run_wgrad``."""
    sh, sw, ph, pw = conv.kgeom

    def wgrad():  # (_fresh consumed on the side stream's turn, not at the call)
        k.conv_wgrad(g, x, w.grad, sh, sw, ph, pw, overwrite=_fresh(w))
        conv.fix_grad(w.grad)
        _done(w)
    _run_wgrad(wgrad, g, x)


# ================================================================== branch stream (Inception)
# Inside TrainStep's step (single GPU, eager), an Inception block's longest branch chain is
# enqueued on a second stream and the block's other branches on the compute stream, joined
# before the block output is used (models/inception.py SideBranch).  Autograd runs each
# node's backward on the stream of its forward, so the chains' backwards overlap too.
# Every tensor that crosses between the streams is record_stream'ed on its consumer (the
# chain input and block buffer at the fork, the block-output gradient in
# _ChannelBuffer.backward, the chain-input gradient in _ConvGroupBNAct.backward), so the
# caching allocator never hands out memory the other stream still reads.
_BRANCH_STREAM = os.environ.get("MPA_BRANCH_STREAM", "1") == "1"
_BR = {"stream": None, "on": False, "used": False}


def branch_streams(enabled: bool) -> None:
    """Allow (TrainStep forward + backward) or stop side-branch streams."""
    _BR["on"] = bool(enabled and _BRANCH_STREAM)


def branch_stream(x: torch.Tensor):
    """The stream a side branch reading ``x`` runs on, or None (off, CPU, no grad, or a
    HIP-graph capture)."""
    if not (_BR["on"] and x.is_cuda and torch.is_grad_enabled()):
        return None
    if _capture_blocks_streams():
        return None
    s = _BR["stream"]
    if s is None or s.device != x.device:
        s = _BR["stream"] = torch.cuda.Stream(x.device)
    _BR["used"] = True
    return s


def join_branch_stream() -> None:
    """The compute stream waits for everything enqueued on the branch stream."""
    s = _BR["stream"]
    if s is not None and _BR["used"]:
        torch.cuda.current_stream(s.device).wait_stream(s)
    _BR["used"] = False


def _branch_use(*ts) -> None:
    """Mark tensors that may come from the other stream as used by the current one."""
    if _BR["on"] and _BR["stream"] is not None:
        cur = torch.cuda.current_stream(_BR["stream"].device)
        for t in ts:
            if t is not None and t.is_cuda:
                t.record_stream(cur)


# =============================================================================== conv+BN
class BNLink:
    """Backward hand-off between two fused conv+BN ops when the first op's output feeds ONLY
    the second (ResNet BasicBlock: conv1 -> bn1 -> relu -> conv2).  The consumer's dgrad
    epilogue then performs the producer's BN-backward reduction - it applies the ReLU
    mask and sums (g, g * x_hat) while the gradient is still in registers - and the
    producer's backward runs only the BN apply pass (no reduce pass, no re-read of dy/y).

    (Round 5 also built the producer's BN + ReLU into the consumer's operand staging; it
    measured 3.9 % slower - profiles/wprod_pre_ab_r5.txt - and was removed in round 6.)"""

    __slots__ = ("z", "y", "mean", "rstd", "gamma", "beta", "sums", "gacc")

    def __init__(self):
        self.z = self.y = self.mean = self.rstd = self.gamma = self.beta = self.sums = None
        # gacc: a DenseNet block gradient.  The consumer's (1x1) dgrad then ADDS gamma*rstd *
        # g into its first Ci channels instead of returning dx, and the producer side
        # (_DenseBlockGrad) finishes the BN backward with deferred per-channel corrections
        self.gacc = None


class BNDefer:
    """A train-mode BN whose apply pass runs in its one consumer (ResNet's downsample BN,
    read as bn2's residual): the producing op computes only the statistics half
    (``bn_stats_affine``: mean, rstd, running stats) and returns the raw conv output; ``aff``
    ([2, C] scale | shift) is what the consumer's ``bn_fwd_train(res_affine=)`` applies while
    reading it.  The tensor then stands for the BN output in autograd: the consumer hands
    back d/d(BN output), which the producer's backward turns into its own BN backward."""

    __slots__ = ("aff", "z", "mean", "rstd", "gamma", "beta", "done")

    def __init__(self):
        self.aff = None
        # the producer's BN inputs, for the consumer's fused backward (bn_bwd_pair): the
        # consumer then hands back d/dz directly and sets `done`
        self.z = self.mean = self.rstd = self.gamma = self.beta = None
        self.done = False


# MPA_BN_PAIR=0: the consumer of a deferred BN (ResNet bn2) writes g = dy * mask and the
# downsample op runs its own BN backward (reduce + apply) on it
_BN_PAIR = os.environ.get("MPA_BN_PAIR", "1") == "1"


class GradJoin:
    """Several gradient contributions to ONE activation, summed without separate add passes.

    A residual block's input x feeds two ops (conv1 and the shortcut: identity or the
    downsample conv); an Inception block's input feeds three or four branches (1x1 convs
    and a pool).  Autograd would sum those bf16 gradients with elementwise adds - a full
    extra read/read/write sweep of the activation per extra consumer.  Instead all
    consumers hold the same join, created with ``expected`` = their number.  Each backward
    that runs hands its contribution to the join and returns None for x, except the LAST
    one, which returns the sum (``add``).  Independent of autograd's execution order
    (autograd runs x's producer only after every consumer's backward).

    A contribution is a computed tensor (a pool or BN gradient), a ``_MaskedRes`` (a
    shortcut gradient dy * mask not yet written) or a ``_Dgrad`` (a conv dgrad not yet
    launched, which can write fresh or accumulate in its GEMM epilogue:
    ``conv_dgrad(..., accum=)``, fp32 add, one rounding per contribution).  How the
    running partial and a newcomer combine (``_combine``):

    ==============  ===================  ======================  ==========================
    partial         + tensor             + _MaskedRes            + _Dgrad
    ==============  ===================  ======================  ==========================
    (none)          kept                 kept unwritten (*)      parked (*)
    tensor          ``add_bf16_``        written, ``add_bf16_``  launched, accum = partial
    _MaskedRes      written,             both written,           ``conv_dgrad_res`` (stride
                    ``add_bf16_``        ``add_bf16_``           1, transposed weight), else
                                                                 written, then as a tensor
    parked _Dgrad   launched,            written, then as a      ``conv_dgrad_pair`` (_PAIR,
                    accum = tensor       tensor                  one of the two full), else
                                                                 two launches (**)
    ==============  ===================  ======================  ==========================

    (*)  the last contribution never stays pending: it is written / launched fresh.
    (**) the fresh write goes to a dgrad that covers every pixel and the other accumulates
         into it, so a 1x1/s2 downsample (three of four stride phases without taps) never
         needs a zero fill; when both or neither are full, the newcomer writes fresh."""

    __slots__ = ("partial", "expected", "arrived")

    def __init__(self, expected: int = 2):
        self.partial = None
        self.expected = int(expected)
        self.arrived = 0

    def add(self, k, c):
        """Hand in one contribution; the sum if it is the last one, else None."""
        self.arrived += 1
        last = self.arrived >= self.expected
        prev, self.partial = self.partial, None
        acc = _combine(k, prev, c, last)
        if last:
            return acc
        self.partial = acc
        return None


class _Dgrad:
    """A conv dgrad not yet launched: ``run(accum)`` launches it (fresh when accum is None);
    ``full``: every pixel of dx receives taps (no tap-less stride phase)."""

    __slots__ = ("k", "dz", "w", "wt", "conv", "in_hw", "full")

    def __init__(self, k, dz, w, wt, conv, in_hw):
        self.k, self.dz, self.w, self.wt, self.conv, self.in_hw = k, dz, w, wt, conv, in_hw
        sh, sw = conv.kgeom[:2]
        R, S = conv.weight.shape[1:3]
        self.full = sh <= R and sw <= S

    def run(self, accum=None):
        sh, sw, ph, pw = self.conv.kgeom
        return self.k.conv_dgrad(self.dz, self.w, self.in_hw[0], self.in_hw[1], sh, sw, ph, pw,
                                 self.wt, accum)


# MPA_DGRAD_PAIR=0: a residual stage's conv1 (3x3/s2) and 1x1/s2 shortcut dgrads run as two
# launches (the second accumulating into the first's dx) instead of one merged launch
_PAIR = os.environ.get("MPA_DGRAD_PAIR", "1") == "1"


def _dgrad_pair(k, a: _Dgrad, b: _Dgrad):
    """Both dgrads of one activation in one launch (``conv_dgrad_pair``): ``a`` covers every
    pixel, ``b`` is the other.  None when the merged launch does not apply."""
    sh, sw, ph, pw = a.conv.kgeom
    sh2, sw2, ph2, pw2 = b.conv.kgeom
    if (sh, sw) != (sh2, sw2) or (a.dz.is_cuda and (a.wt is None or b.wt is None)):
        return None
    if tuple(a.dz.shape) != tuple(b.dz.shape) or a.w.shape[3] != b.w.shape[3]:
        return None
    return k.conv_dgrad_pair(a.dz, a.w, a.wt, a.in_hw[0], a.in_hw[1], sh, sw, ph, pw,
                             b.dz, b.w, b.wt, ph2, pw2)


class _MaskedRes:
    """A residual block's shortcut gradient dy * (y > 0) not yet written: the block input's
    other consumer (conv1's stride-1 dgrad) adds it in its epilogue (``conv_dgrad_res``), or
    it is materialised when that is not available."""

    __slots__ = ("dy", "mask")

    def __init__(self, dy, mask):
        self.dy = dy
        self.mask = mask

    def materialize(self):
        if not self.dy.is_cuda:
            return (self.dy.float() * ref.bitmask_unpack(self.mask, self.dy.shape)).to(
                self.dy.dtype)
        bits = (self.mask.unsqueeze(-1) >> torch.arange(8, device=self.mask.device,
                                                         dtype=torch.uint8)) & 1
        return self.dy * bits.reshape(self.dy.shape).to(self.dy.dtype)


# MPA_RES_MASK=0: a residual block writes its shortcut gradient dy * mask for conv1's dgrad to
# accumulate, instead of conv1's dgrad epilogue reading dy and the bit mask itself
_RES_MASK = os.environ.get("MPA_RES_MASK", "1") == "1"


def _dgrad_res(k, d: _Dgrad, res: _MaskedRes):
    """``d`` with the unwritten shortcut gradient ``res`` added in its epilogue
    (``conv_dgrad_res``).  None when the fused launch does not apply."""
    sh, sw, ph, pw = d.conv.kgeom
    if (sh, sw) != (1, 1) or (d.wt is None and d.dz.is_cuda):
        return None
    return k.conv_dgrad_res(d.dz, d.w, d.wt, d.in_hw[0], d.in_hw[1], ph, pw, res.dy, res.mask)


def _combine(k, prev, new, last: bool):
    """``prev`` (a join's partial, or None) + ``new`` by GradJoin's table; ``last``: nothing
    follows ``new``.  Returns the sum as a tensor, or a first arrival left pending."""
    if isinstance(new, _MaskedRes) and (last or prev is not None):
        new = new.materialize()
    if prev is None:
        return new.run() if (last and isinstance(new, _Dgrad)) else new
    parked, dgrad = isinstance(prev, _Dgrad), isinstance(new, _Dgrad)
    if isinstance(prev, _MaskedRes):
        acc = _dgrad_res(k, new, prev) if dgrad else None
        if acc is not None:
            return acc
        prev = prev.materialize()
    if parked and dgrad:
        acc = None
        if _PAIR and new.full != prev.full:
            acc = _dgrad_pair(k, new, prev) if new.full else _dgrad_pair(k, prev, new)
        if acc is not None:
            return acc
        if new.full or not prev.full:
            return prev.run(new.run())
        return new.run(prev.run())
    if parked:
        return prev.run(new)  # (accumulates into the newcomer)
    if dgrad:
        return new.run(prev)
    acc = prev.contiguous()  # (Inception's Mixed_7a maxpool + aux-head avg-pool)
    k.add_bf16_(acc, new.contiguous())
    return acc


def _input_grad(k, g, w, conv, in_hw, join: Optional[GradJoin] = None,
                link: Optional[BNLink] = None, reduce_joined: bool = True):
    """What a conv op returns for its input x, from its output gradient ``g``.  ``link``
    (the BNLink of x's producer, a ReLU(BN)) selects a dgrad that also runs the producer's
    BN-backward reduction, leaving the sums in ``link.sums``: into a DenseNet block gradient
    (``link.gacc``: nothing is returned), or as dx * mask, which then goes through ``join``
    as a tensor - unless ``reduce_joined`` is off, when a join rules the fused reduction
    out.  Otherwise the plain dgrad, through ``join`` if there is one."""
    li = link
    wb, wt = weight_of(w), weight_t_of(w)
    gacc = li is not None and li.gacc is not None
    bnred = li is not None and li.z is not None and (join is None or reduce_joined)
    if ((gacc or bnred) and (wt is not None or not g.is_cuda)
            and k.conv_bnred_ok(w.shape[0], w.shape[3])):
        if gacc:
            li.sums = k.conv_dgrad_bnred_gacc(g, wb, wt, li.z, li.mean, li.rstd, li.gamma,
                                              li.beta, li.gacc)
            return None
        sh, sw, ph, pw = conv.kgeom
        dx, li.sums = k.conv_dgrad_bnred(g, wb, in_hw[0], in_hw[1], sh, sw, ph, pw, wt, li.z,
                                         _or_empty(li.y, g), li.mean, li.rstd, gamma=li.gamma,
                                         beta=li.beta)
        return dx if join is None else join.add(k, dx)
    d = _Dgrad(k, g, wb, wt, conv, in_hw)
    return d.run() if join is None else join.add(k, d)


class _ConvBNAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, w, b, gamma, beta, conv, bn, relu, link_in=None, link_out=None,
                join_x=None, join_res=None, defer=None, res_defer=None, out=None):
        k = K(x)
        sh, sw, ph, pw = conv.kgeom
        C = w.shape[0]
        stats = torch.empty(2, C, device=x.device, dtype=torch.float32)
        # BN statistics come out of the conv epilogue, shifted by the running mean
        z = k.conv_fwd(x, weight_of(w), _or_empty(b, x), sh, sw, ph, pw, False, stats,
                       _empty(x) if _NO_SHIFT else bn.running_mean)
        # relu(bn(z) + residual): the backward's ReLU mask as one bit per element, written by
        # the forward, so neither backward pass reads y (two activation-sized reads less)
        ymask = None
        if relu and residual is not None:
            ymask = torch.empty(z.numel() // 8, device=z.device, dtype=torch.uint8)
        if defer is not None:  # statistics only; the consumer applies this BN (BNDefer)
            mean, rstd, defer.aff = k.bn_stats_affine(z, stats, gamma, beta, bn.running_mean,
                                                      bn.running_var, bn.momentum_value(),
                                                      bn.eps, bn.num_batches_tracked)
            defer.z, defer.mean, defer.rstd, defer.gamma, defer.beta = z, mean, rstd, gamma, beta
            defer.done = False
            y = z
        else:
            y, mean, rstd = k.bn_fwd_train(z, stats, gamma, beta, bn.running_mean,
                                           bn.running_var, bn.momentum_value(), bn.eps,
                                           _or_empty(residual, x), relu,
                                           bn.num_batches_tracked, mask=ymask,
                                           res_affine=(res_defer.aff if res_defer is not None
                                                       else None), out=out)
        ctx.conv = conv
        ctx.relu = relu
        ctx.has_res = residual is not None
        ctx.bias = b
        ctx.params = (w, gamma, beta)
        ctx.in_hw = (x.shape[1], x.shape[2])
        # (relu(bn(z)) without a residual recomputes its mask from z: y is not kept)
        keep_y = relu and ymask is None and not (residual is None and beta is not None)
        ctx.save_for_backward(x, z, y if keep_y else None, mean, rstd, ymask)
        ctx.link_in = link_in
        ctx.link_out = link_out
        ctx.join_x = join_x
        ctx.join_res = join_res
        ctx.defer = defer
        ctx.res_defer = res_defer if (ymask is not None and relu and _BN_PAIR) else None
        if link_out is not None:
            link_out.z, link_out.mean, link_out.rstd = z, mean, rstd
            # ReLU without a residual: the consumer's halo dgrad recomputes the mask from z
            # (as the forward rounded y) when the BN is affine and never reads y (the
            # implicit-GEMM fallback does)
            zmask = relu and residual is None and gamma is not None and beta is not None
            link_out.y = y if relu else None
            link_out.gamma, link_out.beta = (gamma, beta) if zmask else (None, None)
            link_out.sums = None
        return y

    @staticmethod
    def _bn_backward(ctx, k, dy, z, y, mean, rstd, ymask, lo, want_g):
        """The BN (+ residual, ReLU) backward in the one form that applies.  Returns
        (dz, g, dres_pair): ``g`` = the residual's gradient dy * mask if ``want_g`` (a tensor,
        or a _MaskedRes left unwritten), ``dres_pair`` = d/dz of the deferred BN that produced
        the residual, when ``bn_bwd_pair`` ran that BN's backward too."""
        gamma, beta = ctx.params[1:]
        rd = ctx.res_defer
        if ctx.defer is not None and ctx.defer.done:
            # the consumer's bn_bwd_pair already ran this BN's backward: dy IS d/dz, and the
            # affine gradients are in place
            ctx.defer.done = False
            return dy, None, None
        if (rd is not None and rd.z is not None and ctx.needs_input_grad[1]
                and ctx.join_res is None):
            g2, b2 = rd.gamma, rd.beta
            dz, dres_pair = k.bn_bwd_pair(dy, z, ymask, mean, rstd, gamma, _sink(gamma, dy),
                                          _sink(beta, dy), rd.z, rd.mean, rd.rstd, g2,
                                          _sink(g2, dy), _sink(b2, dy))
            _done(g2, b2)
            rd.done = True
            rd.z = None
            return dz, None, dres_pair
        if lo is not None and lo.sums is not None:
            # the consumer's dgrad already masked dy and reduced (sum g, sum g*xhat)
            dz, g = k.bn_bwd_apply(dy, z, _empty(dy), mean, rstd, gamma, _sink(gamma, dy),
                                   _sink(beta, dy), lo.sums, True, want_g)
            lo.sums = None
            return dz, g, None
        if ctx.relu and not ctx.has_res and beta is not None:
            # relu(bn(z)) without a residual: the mask is recomputed from z, y is not read
            dz, g = k.bn_bwd(dy, z, _empty(dy), mean, rstd, gamma, _sink(gamma, dy),
                             _sink(beta, dy), True, want_g, beta)
            return dz, g, None
        # identity shortcut: conv1's dgrad adds dy * mask in its epilogue (_MaskedRes), so
        # g is not written here
        mres = (want_g and _RES_MASK and ymask is not None and ctx.join_res is not None
                and ctx.join_res.arrived == 0 and ctx.join_res.partial is None)
        dz, g = k.bn_bwd(dy, z, _or_empty(y, dy), mean, rstd, gamma, _sink(gamma, dy),
                         _sink(beta, dy), True, want_g and not mres, ymask=ymask)
        return dz, (_MaskedRes(dy, ymask) if mres else g), None

    @staticmethod
    def backward(ctx, dy):
        x, z, y, mean, rstd, ymask = ctx.saved_tensors
        w, gamma, beta = ctx.params
        k = K(dy)
        dy = _rows(dy)
        want_g = bool(ctx.has_res and ctx.needs_input_grad[1])
        lo = ctx.link_out
        # The link holds this op's own z and y, and y's grad_fn is this node: a reference
        # cycle that kept every linked activation (6.1 GB per ResNet-18 b2048 step) alive
        # until Python's next full cyclic collection - hundreds of steps away, or never
        # inside steps_without_gc.  The consumer's backward has run by now, so the node lets
        # go of the link and reference counting frees the step's activations again.
        ctx.link_out = None
        dz, g, dres = _ConvBNAct._bn_backward(ctx, k, dy, z, y, mean, rstd, ymask, lo, want_g)
        if ctx.defer is None or dz is not dy:
            _done(gamma, beta)
        if w.requires_grad:
            _conv_wgrad(k, dz, x, w, ctx.conv)
        _done(ctx.bias)
        if dres is None and want_g:  # (else d/dz of the deferred BN's producer: BNDefer.done)
            dres = g if ctx.join_res is None else ctx.join_res.add(k, g)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = _input_grad(k, dz, w, ctx.conv, ctx.in_hw, ctx.join_x, ctx.link_in)
        return _grads(_ConvBNAct, dx, dres)


def _rows(t: torch.Tensor) -> torch.Tensor:
    """``t`` if its rows are uniformly strided with contiguous channels (a channel window
    of a wider NHWC buffer, which the BN kernels read in place), else a contiguous copy."""
    if t.is_contiguous():
        return t
    if t.dim() >= 2 and t.stride(-1) == 1:
        ld, expect = t.stride(-2), t.stride(-2) * t.shape[-2]
        ok = ld >= t.shape[-1] and ld % 8 == 0
        for d in range(t.dim() - 3, -1, -1):
            ok = ok and (t.shape[d] == 1 or t.stride(d) == expect)
            expect *= t.shape[d]
        if ok:
            return t
    return t.contiguous()


def conv_bn_act(x, conv, bn, relu: bool = True, residual: Optional[torch.Tensor] = None,
                link_in: Optional[BNLink] = None, link_out: Optional[BNLink] = None,
                join_x: Optional[GradJoin] = None, join_res: Optional[GradJoin] = None,
                defer: Optional[BNDefer] = None, res_defer: Optional[BNDefer] = None,
                out: Optional[torch.Tensor] = None):
    """relu(bn(conv(x)) [+ residual]); BN in train or eval mode per ``bn.training``.
    ``out`` (train mode, no residual): a channel window of a wider NHWC buffer the result
    is written into (see ``channel_buffer``).

    A conv bias in front of a train-mode BN (VGG11_bn) is added before the statistics, so
    forward and running stats are exact; its gradient is exactly zero in exact arithmetic
    (BN removes any per-channel constant) and is left at zero instead of accumulating
    rounding noise."""
    x = conv.fit_input(x)
    if bn.training:
        # (defer: bn(conv(x)) without ReLU or residual, a train-mode affine BN)
        if defer is not None and (relu or residual is not None or bn.weight is None
                                  or bn.bias is None):
            defer = None
        if out is not None and (residual is not None or defer is not None or link_out is not None):
            out = None
        return _ConvBNAct.apply(x, residual, conv.weight, conv.bias, bn.weight, bn.bias, conv,
                                bn, relu, link_in, link_out, join_x, join_res, defer, res_defer,
                                out)
    k = K(x)
    sh, sw, ph, pw = conv.kgeom
    z = k.conv_fwd(x, weight_of(conv.weight), _or_empty(conv.bias, x), sh, sw, ph, pw, False,
                   _empty(x), _empty(x))
    return k.bn_fwd_eval(z, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps,
                         _or_empty(residual, x), relu)


class _ConvGroupBNAct(torch.autograd.Function):
    """relu(bn_b(conv_b(x))) for several 1x1 convs that read the same x (Inception's branch
    heads), as ONE GEMM over their joint output rows.

    The weights sit back to back in the arena (``_mpa_param_groups``), so the joint weight,
    its bf16 shadow and its gradient are flat views - no copies.  Forward: one conv over
    N = sum N_b columns with BN statistics from its epilogue, then each branch's BN+ReLU
    reads its channel window of z (strided rows).  A member with ``pool_after`` (Inception's
    pool branch: 1x1 conv and 3x3 average pool commute) average-pools its window first and
    takes its BN statistics from the pooled values.  Backward: each branch's BN (and pool)
    backward writes its window of ONE dz, then one wgrad (x read once, not once per branch)
    and ONE dgrad (one write of dx instead of a write plus an accumulate pass per extra
    branch).
    Reference: InceptionA/C/D/E branch heads of torchvision inception_v3, reached from
    ``/root/reference/models.py:83-95``."""

    @staticmethod
    def forward(ctx, x, W, mods, join, outs, *params):
        k = K(x)
        ntot = W.shape[0]
        stats = torch.empty(2, ntot, device=x.device, dtype=torch.float32)
        z = k.conv_fwd(x, W, _empty(x), 1, 1, 0, 0, False, stats, _empty(x))
        res, saved, o = [], [], 0
        for m in mods:
            bn, n = m.bn, m.conv.weight.shape[0]
            pool = getattr(m, "pool_after", None)
            if pool is not None:  # avg-pool the window, BN statistics of the pooled values
                zin = k.avgpool_fwd(z[..., o:o + n], *pool)
                st = _empty(x)
            else:
                zin, st = z[..., o:o + n], stats[:, o:o + n]
            dst = outs[len(res)] if outs is not None else None
            y, mean, rstd = k.bn_fwd_train(zin, st, bn.weight, bn.bias, bn.running_mean,
                                           bn.running_var, bn.momentum_value(), bn.eps,
                                           _empty(x), True, bn.num_batches_tracked, out=dst)
            res.append(y)
            saved.append((mean, rstd, o, n, zin if pool is not None else None, pool))
            o += n
        ctx.mods, ctx.join, ctx.saved, ctx.W = mods, join, saved, W
        ctx.in_hw = (x.shape[1], x.shape[2])
        ctx.nparams = len(params)
        ctx.save_for_backward(x, z)
        return tuple(res)

    @staticmethod
    def backward(ctx, *dys):
        x, z = ctx.saved_tensors
        _branch_use(*dys)  # (a member's gradient may come from a side-branch chain)
        k = K(z)
        dz = torch.empty_like(z)
        for m, (mean, rstd, o, n, zp, pool), dy in zip(ctx.mods, ctx.saved, dys):
            gamma, beta = m.bn.weight, m.bn.bias
            if pool is not None:
                dzp, _g = k.bn_bwd(_rows(dy), zp, _empty(dy), mean, rstd, gamma,
                                   _sink(gamma, dy), _sink(beta, dy), True, False, beta)
                k.avgpool_bwd(dzp, z.shape[1], z.shape[2], *pool, dx_out=dz[..., o:o + n])
            else:
                k.bn_bwd(_rows(dy), z[..., o:o + n], _empty(dy), mean, rstd, gamma,
                         _sink(gamma, dy), _sink(beta, dy), True, False, beta,
                         dx_out=dz[..., o:o + n])
            _done(gamma, beta)
        ws = [m.conv.weight for m in ctx.mods]
        if ws[0].requires_grad:
            def wgrad():
                fresh = [_fresh(w) for w in ws]  # (every flag consumed)
                G = ws[0]._mpa_arena.flat_view(ws, "grad").view(ctx.W.shape)
                k.conv_wgrad(dz, x, G, 1, 1, 0, 0, overwrite=all(fresh))
                _done(*ws)
            _run_wgrad(wgrad, dz, x)
        dx = None
        if ctx.needs_input_grad[0]:
            # (the joint weight is an arena view with no transposed copy: the plain dgrad)
            d = _Dgrad(k, dz, ctx.W, None, ctx.mods[0].conv, ctx.in_hw)
            dx = d.run() if ctx.join is None else ctx.join.add(k, d)
        ctx.W = None
        return (dx, None, None, None, None) + (None,) * ctx.nparams


def conv1x1_group_ok(x, mods) -> bool:
    """Whether ``conv1x1_group`` can run ``mods`` (train-mode 1x1/s1 BasicConv2d's whose
    weights are one flat arena range)."""
    ws = [m.conv.weight for m in mods]
    a = getattr(ws[0], "_mpa_arena", None)
    if a is None or not torch.is_grad_enabled() or not all(m.bn.training for m in mods):
        return False
    if any(m.conv.kgeom != (1, 1, 0, 0) or m.conv.weight.shape[1:3] != (1, 1) or
           m.conv.bias is not None or not w.requires_grad for m, w in zip(mods, ws)):
        return False
    if any(getattr(m, "pool_after", None) is not None and
           tuple(m.pool_after[2:6]) != (1, 1, (m.pool_after[0] - 1) // 2,
                                        (m.pool_after[1] - 1) // 2) for m in mods):
        return False  # (a pooled window must keep z's spatial size)
    return a.flat_view(ws, "master") is not None


def conv1x1_group(x, mods, join: Optional[GradJoin] = None, outs=None):
    """[relu(bn(conv(x))) for each BasicConv2d in mods] as one GEMM (see _ConvGroupBNAct);
    ``join``: x's gradient is summed with its other consumers' (one contribution here);
    ``outs``: per member, a channel window to write its output into, or None."""
    ws = [m.conv.weight for m in mods]
    a = ws[0]._mpa_arena
    W = a.flat_view(ws, "shadow" if a.shadow is not None else "master")
    ntot = sum(w.shape[0] for w in ws)
    W = W.view(ntot, 1, 1, ws[0].shape[-1])
    params = [p for m in mods for p in (m.conv.weight, m.bn.weight, m.bn.bias) if p is not None]
    return _ConvGroupBNAct.apply(x, W, list(mods), join, outs, *params)


def _pool_out(n: int, k: int, s: int, p: int, ceil: bool) -> int:
    """Pooled extent, ATen's rule (a ceil-mode window must start inside the padded input)."""
    o = (n + 2 * p - k + (s - 1 if ceil else 0)) // s + 1
    if ceil and (o - 1) * s >= n + p:
        o -= 1
    return o


class _ConvBNReLUPool(torch.autograd.Function):
    """maxpool(relu(bn(conv(x)))) -- the ResNet / DenseNet stem -- with BN, ReLU and the
    pool fused into one pass over the conv output z (forward) and the pool's gradient
    gathered straight into the BN backward (backward): the full-size BN output and its
    gradient never exist.  Reference: torchvision stems reached from ``models.py:24-30``
    (resnet) and ``models.py:74-80`` (densenet)."""

    @staticmethod
    def forward(ctx, x, w, b, gamma, beta, conv, bn, cfg):
        k = K(x)
        sh, sw, ph, pw = conv.kgeom
        C = w.shape[0]
        stats = torch.empty(2, C, device=x.device, dtype=torch.float32)
        shift = _empty(x) if _NO_SHIFT else bn.running_mean
        z = k.conv_fwd(x, weight_of(w), _or_empty(b, x), sh, sw, ph, pw, False, stats, shift)
        # zsel: raw z at each window's argmax, so the backward's reduction pass reads only
        # pooled-size tensors (maxpool_bn_bwd_sel_reduce_kernel)
        N, H, W, C_ = z.shape
        zsel = torch.empty(N, _pool_out(H, cfg[0], cfg[2], cfg[4], cfg[6]),
                           _pool_out(W, cfg[1], cfg[3], cfg[5], cfg[6]), C_,
                           device=z.device, dtype=z.dtype)
        y, idx, mean, rstd = k.bn_relu_maxpool_fwd(z, stats, gamma, beta, bn.running_mean,
                                                   bn.running_var, bn.momentum_value(),
                                                   bn.eps, *cfg, bn.num_batches_tracked,
                                                   zsel_out=zsel)
        ctx.conv = conv
        ctx.cfg = cfg
        ctx.bias = b
        ctx.params = (w, gamma, beta)
        ctx.in_hw = (x.shape[1], x.shape[2])
        ctx.save_for_backward(x, z, idx, mean, rstd, zsel)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, z, idx, mean, rstd, zsel = ctx.saved_tensors
        w, gamma, beta = ctx.params
        conv = ctx.conv
        k = K(dy)
        sh, sw, ph, pw = conv.kgeom
        dy = dy.contiguous()
        if (_STEM_POOL_WGRAD and w.requires_grad and not ctx.needs_input_grad[0]
                and ctx.bias is None and tuple(ctx.cfg) == (3, 3, 2, 2, 1, 1, False)
                and k.stem_pool_wgrad_ok(dy, idx, z, x, w.grad, sh, sw, ph, pw)):
            # image stem: the BN / pool backward's dz pass runs inside the weight
            # gradient's operand staging, so no full-resolution dz exists
            sums = k.maxpool_bn_bwd_sums(dy, zsel, mean, rstd, gamma, beta, _sink(gamma, dy),
                                         _sink(beta, dy))
            _done(gamma, beta)

            def wgrad():
                k.stem_pool_wgrad(dy, idx, z, mean, rstd, gamma, beta, sums, x, w.grad,
                                  sh, sw, ph, pw, _fresh(w))
                conv.fix_grad(w.grad)
                _done(w)
            _run_wgrad(wgrad, dy, idx, z, x, mean, rstd, sums)
            return _grads(_ConvBNReLUPool)
        dz = k.maxpool_bn_bwd(dy, idx, z, mean, rstd, gamma, beta, _sink(gamma, dy),
                              _sink(beta, dy), *ctx.cfg[:6], zsel=zsel)
        _done(gamma, beta)
        if w.requires_grad:
            _conv_wgrad(k, dz, x, w, conv)
        _done(ctx.bias)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = _input_grad(k, dz, w, conv, ctx.in_hw)
        return _grads(_ConvBNReLUPool, dx)


# (A/B switch) the stem's pool backward inside its weight gradient (on: 1.06 ms vs 1.63 ms
# two-pass at batch 1024 - profiles/stem_pool_r6.txt)
_STEM_POOL_WGRAD = os.environ.get("MPA_STEM_POOL_WGRAD", "1") == "1"


def conv_bn_relu_maxpool(x, conv, bn, pool):
    """``pool(relu(bn(conv(x))))`` for a MaxPool2d ``pool``; fused in train mode."""
    cfg = (pool.kernel_size[0], pool.kernel_size[1], pool.stride[0], pool.stride[1],
           pool.padding[0], pool.padding[1], bool(pool.ceil_mode))
    if bn.training and cfg[0] * cfg[1] <= 256:
        x = conv.fit_input(x)
        return _ConvBNReLUPool.apply(x, conv.weight, conv.bias, bn.weight, bn.bias, conv, bn,
                                     cfg)
    return pool(conv_bn_act(x, conv, bn, relu=True))


# ============================================================================ conv + bias
_UNIT = {}


def _unit_affine(C: int, device):
    """(mean 0, rstd 1, gamma 1, beta 0) of length C: the identity 'BN' through which a
    plain ReLU's mask and bias-gradient reduction ride the fused BN-backward-reduction
    dgrad (bn(y) = y, so the mask is y > 0 and sum g is the bias gradient)."""
    key = (C, device)
    t = _UNIT.get(key)
    if t is None:
        z, o = torch.zeros(C, device=device), torch.ones(C, device=device)
        t = _UNIT[key] = (z, o, o, z)
    return t


class _ConvAct(torch.autograd.Function):
    """act(conv(x) + b).  ``link_out`` (BNLink): this op's ReLU output feeds ONLY the next
    conv, whose dgrad applies the ReLU mask (y > 0) and reduces the bias gradient in its
    epilogue (the BN-backward-reduction flavour with an identity affine), so this op's
    backward runs no act_bwd pass (VGG / AlexNet conv -> ReLU -> conv chains,
    ``/root/reference/models.py:50,59``); ``link_in``: the BNLink of this op's input."""

    @staticmethod
    def forward(ctx, x, w, b, conv, relu, join=None, stats=None, shift=None, out=None,
                link_in=None, link_out=None):
        k = K(x)
        sh, sw, ph, pw = conv.kgeom
        if out is not None:  # written straight into a channel window of a wider buffer
            k.conv_fwd_into(x, weight_of(w), _or_empty(b, x), sh, sw, ph, pw, relu,
                            _or_empty(stats, x), _or_empty(shift, x), out)
            y = out
        else:
            y = k.conv_fwd(x, weight_of(w), _or_empty(b, x), sh, sw, ph, pw, relu,
                           _or_empty(stats, x), _or_empty(shift, x))
        ctx.conv = conv
        ctx.relu = relu
        ctx.params = (w, b)
        ctx.in_hw = (x.shape[1], x.shape[2])
        ctx.join = join
        ctx.link_in = link_in
        ctx.link_out = link_out
        if link_out is not None and relu and out is None:
            C = y.shape[-1]
            link_out.z = link_out.y = y
            link_out.mean, link_out.rstd, link_out.gamma, link_out.beta = \
                _unit_affine(C, y.device)
            link_out.sums = None
        ctx.save_for_backward(x, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y = ctx.saved_tensors
        w, b = ctx.params
        conv = ctx.conv
        k = K(dy)
        dy = dy.contiguous()
        lo = ctx.link_out
        ctx.link_out = None  # (breaks the y -> node -> link -> y cycle, see _ConvBNAct.backward)
        if lo is not None and lo.sums is not None:
            # the consumer's dgrad already applied the mask; its sum g is the bias gradient
            g = dy
            bs = _sink(b, dy)
            if bs.numel():
                k.add_f32_(bs, lo.sums[:bs.numel()])
            lo.sums = None
        else:
            g = k.act_bwd(dy, _or_empty(y, dy), _sink(b, dy))
        _done(b)
        if w.requires_grad:
            _conv_wgrad(k, g, x, w, conv)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = _input_grad(k, g, w, conv, ctx.in_hw, ctx.join, ctx.link_in,
                             reduce_joined=False)
        return _grads(_ConvAct, dx)


def conv_act(x, conv, relu: bool = False, join: Optional[GradJoin] = None,
             stats: Optional[torch.Tensor] = None, shift: Optional[torch.Tensor] = None,
             out: Optional[torch.Tensor] = None, link_in: Optional[BNLink] = None,
             link_out: Optional[BNLink] = None):
    """act(conv(x) + b); ``join``: x's gradient is summed with its other consumers' (see
    GradJoin); ``stats`` ([2, N] fp32, training): receives the output's per-channel
    [mean | var] from the GEMM epilogue (sums shifted by ``shift`` for precision); ``out``
    (training): a channel window of a wider NHWC buffer the output is written into (the
    result is that window; ``stats`` may then be a [2, N] window of a wider table)."""
    x = conv.fit_input(x)
    if torch.is_grad_enabled() and (conv.weight.requires_grad or x.requires_grad):
        return _ConvAct.apply(x, conv.weight, conv.bias, conv, relu, join, stats, shift, out,
                              link_in, link_out)
    k = K(x)
    sh, sw, ph, pw = conv.kgeom
    return k.conv_fwd(x, weight_of(conv.weight), _or_empty(conv.bias, x), sh, sw, ph, pw, relu,
                      _empty(x), _empty(x))


# ======================================================================== depthwise conv
class _DwConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, conv, stats=None, shift=None, join=None):
        k = K(x)
        sh, sw, ph, pw = conv.kgeom
        z = k.dwconv_fwd(x, weight_of(w), sh, sw, ph, pw, _or_empty(stats, x),
                         _or_empty(shift, x))
        ctx.conv, ctx.w, ctx.join = conv, w, join
        ctx.in_hw = (x.shape[1], x.shape[2])
        ctx.save_for_backward(x)
        return z

    @staticmethod
    def backward(ctx, dz):
        (x,) = ctx.saved_tensors
        w, conv = ctx.w, ctx.conv
        k = K(dz)
        dz = dz.contiguous()
        if w.requires_grad:
            sh, sw, ph, pw = conv.kgeom

            def wgrad():
                k.dwconv_wgrad(dz, x, w.grad, sh, sw, ph, pw, overwrite=_fresh(w))
                _done(w)
            _run_wgrad(wgrad, dz, x)
        dx = None
        if ctx.needs_input_grad[0]:
            sh, sw, ph, pw = conv.kgeom
            j = ctx.join
            # a join's running partial, when it is a written tensor, is accumulated into by
            # the kernel (fp32 add, one rounding); otherwise dx joins as a computed tensor
            prev = j.partial if j is not None else None
            if isinstance(prev, torch.Tensor) and prev.is_contiguous():
                j.partial = None
                dx = j.add(k, k.dwconv_dgrad(dz, weight_of(w), *ctx.in_hw, sh, sw, ph, pw, prev))
            else:
                dx = k.dwconv_dgrad(dz, weight_of(w), *ctx.in_hw, sh, sw, ph, pw)
                if j is not None:
                    dx = j.add(k, dx)
        return _grads(_DwConv, dx)


def dwconv(x, conv, stats: Optional[torch.Tensor] = None, shift: Optional[torch.Tensor] = None,
           join: Optional[GradJoin] = None):
    """Depthwise conv (``conv.groups == channels``, no bias); ``stats`` ([2, C] fp32): receives
    the output's per-channel [mean | var] from the kernel's epilogue (sums shifted by ``shift``)
    in the format ``bn_act(stats=)`` takes; ``join``: x's gradient is summed with its other
    consumers' (GradJoin)."""
    if not conv.depthwise or conv.bias is not None:
        raise ValueError("dwconv: a bias-free depthwise Conv2d (groups == channels) expected")
    if torch.is_grad_enabled() and (conv.weight.requires_grad or x.requires_grad):
        return _DwConv.apply(x, conv.weight, conv, stats, shift, join)
    sh, sw, ph, pw = conv.kgeom
    return K(x).dwconv_fwd(x, weight_of(conv.weight), sh, sw, ph, pw, _or_empty(stats, x),
                           _or_empty(shift, x))


def dwconv_bn_act(x, conv, bn, relu: bool = True):
    """relu?(bn(dwconv(x))): train mode takes the BN statistics from the conv's epilogue."""
    if bn.training:
        stats = torch.empty(2, conv.out_channels, device=x.device, dtype=torch.float32)
        z = dwconv(x, conv, stats, None if _NO_SHIFT else bn.running_mean)
        return bn_act(z, bn, relu=relu, stats=stats)
    return bn_act(dwconv(x, conv), bn, relu=relu)


# ========================================= LayerNorm / GELU / layer scale (ConvNeXt, ln.hip)
class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, pre, eps):
        y, stat = K(x).ln_fwd(x, _or_empty(pre, x), w, b, eps)
        ctx.params = (w, b, pre)
        ctx.save_for_backward(x, stat)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, stat = ctx.saved_tensors
        w, b, pre = ctx.params
        k = K(dy)
        dy = dy.contiguous()
        ps = [p for p in (w, b, pre) if p is not None]
        if not all(p.requires_grad for p in ps):  # frozen: gradients into scratch
            tmp = torch.empty(3, x.shape[-1], device=x.device, dtype=torch.float32)
            dx = k.ln_bwd(dy, x, _or_empty(pre, x), w, stat, tmp[0], tmp[1], _empty(x), True)
            return _grads(_LayerNorm, dx)
        # dx on the compute stream (the chain waits for it) with the parameter gradients: one
        # kernel produces both, so nothing is left for the side stream
        fresh = [_fresh(p) for p in ps]
        dx = k.ln_bwd(dy, x, _or_empty(pre, x), w, stat, grad_sink(w), grad_sink(b),
                      _sink(pre, x), all(fresh))
        _done(*ps)
        return _grads(_LayerNorm, dx)


def layer_norm(x, ln, pre_bias: Optional[torch.nn.Parameter] = None):
    """LayerNorm over the last (channel) axis of ``x + pre_bias``; ``pre_bias`` is the bias of the
    depthwise conv that produced ``x``, added in the kernel's registers."""
    if torch.is_grad_enabled() and (ln.weight.requires_grad or x.requires_grad):
        return _LayerNorm.apply(x, ln.weight, ln.bias, pre_bias, ln.eps)
    return K(x).ln_fwd(x, _or_empty(pre_bias, x), ln.weight, ln.bias, ln.eps)[0]


def dwconv_ln(x, conv, ln, join: Optional[GradJoin] = None):
    """ln(dwconv(x) + conv.bias): the conv runs bias-free and the LayerNorm kernel adds the bias."""
    if not conv.depthwise:
        raise ValueError("dwconv_ln: a depthwise Conv2d (groups == channels) expected")
    if torch.is_grad_enabled() and (conv.weight.requires_grad or x.requires_grad):
        z = _DwConv.apply(x, conv.weight, conv, None, None, join)
    else:
        sh, sw, ph, pw = conv.kgeom
        z = K(x).dwconv_fwd(x, weight_of(conv.weight), sh, sw, ph, pw, _empty(x), _empty(x))
    return layer_norm(z, ln, conv.bias)


class _Gelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h):
        ctx.save_for_backward(h)
        return K(h).gelu_fwd(h)

    @staticmethod
    def backward(ctx, da):
        (h,) = ctx.saved_tensors
        return K(da).gelu_bwd(da.contiguous(), h, _empty(da))


def gelu(x):
    """Exact (erf) GELU, ``nn.GELU()``."""
    if torch.is_grad_enabled() and x.requires_grad:
        return _Gelu.apply(x)
    return K(x).gelu_fwd(x)


class _LinearGelu(torch.autograd.Function):
    """gelu(x W^T + b): the pre-activation is kept, and the GELU backward reduces the bias
    gradient from the dh it stores (the role ``act_bwd`` plays for ReLU)."""

    @staticmethod
    def forward(ctx, x, w, b):
        k = K(x)
        h = k.linear_fwd(x, weight_of(w), _or_empty(b, x), False)
        ctx.params = (w, b)
        ctx.save_for_backward(x, h)
        return k.gelu_fwd(h)

    @staticmethod
    def backward(ctx, da):
        x, h = ctx.saved_tensors
        w, b = ctx.params
        k = K(da)
        g = k.gelu_bwd(da.contiguous(), h, _sink(b, da))
        dx = (k.linear_dgrad(g, weight_of(w), weight_t_of(w)) if ctx.needs_input_grad[0]
              else None)
        _done(b)
        if w.requires_grad:
            k.linear_wgrad(g, x, w.grad, overwrite=_fresh(w))
            _done(w)
        return dx, None, None


def linear_gelu(x, lin):
    """gelu(lin(x)) over rows [M, in]; the layer's output width must be stored unpadded."""
    if lin.weight.shape[0] != lin.out_features:
        raise ValueError("linear_gelu: out_features must be a multiple of 32")
    if torch.is_grad_enabled() and (lin.weight.requires_grad or x.requires_grad):
        return _LinearGelu.apply(x, lin.weight, lin.bias)
    k = K(x)
    return k.gelu_fwd(k.linear_fwd(x, weight_of(lin.weight), _or_empty(lin.bias, x), False))


class _ScaleResidual(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, gamma, res, join=None):
        ctx.gamma, ctx.join = gamma, join
        ctx.save_for_backward(y)
        return K(y).scale_add_fwd(y, gamma, res)

    @staticmethod
    def backward(ctx, dout):
        (y,) = ctx.saved_tensors
        gamma = ctx.gamma
        k = K(dout)
        dout = dout.contiguous()
        if gamma.requires_grad:
            dy = k.scale_add_bwd(dout, y, gamma, grad_sink(gamma), _fresh(gamma))
            _done(gamma)
        else:
            dy = k.scale_add_bwd(dout, y, gamma, torch.empty_like(gamma, dtype=torch.float32),
                                 True)
        # the residual's gradient is dout itself: through the join it becomes the accumulate
        # operand of the block's depthwise dgrad, no add pass
        dres = None
        if ctx.needs_input_grad[2]:
            dres = dout if ctx.join is None else ctx.join.add(k, dout)
        return dy, None, dres, None


def scale_residual(y, gamma, res, join: Optional[GradJoin] = None):
    """res + gamma[c] * y (ConvNeXt's layer scale and residual add); ``join``: res's gradient is
    summed with its other consumers' (GradJoin)."""
    if torch.is_grad_enabled() and (gamma.requires_grad or y.requires_grad or res.requires_grad):
        return _ScaleResidual.apply(y, gamma, res, join)
    return K(y).scale_add_fwd(y, gamma, res)


# ============================================ multi-head attention and ViT tokens (attn.hip)
class _Attention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, heads):
        o, lse = K(qkv).attn_fwd(qkv, heads)
        ctx.heads = heads
        ctx.save_for_backward(qkv, o, lse)
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, o, lse = ctx.saved_tensors
        return K(do).attn_bwd(do.contiguous(), qkv, o, lse, ctx.heads), None


def attention(qkv, heads: int):
    """Self-attention over the packed in-projection output ``qkv`` [B, S, 3 * heads * 64] (q, k, v
    row blocks, heads of 64 inside each): [B, S, heads * 64], scale 1/8, no mask, no dropout."""
    if torch.is_grad_enabled() and qkv.requires_grad:
        return _Attention.apply(qkv, heads)
    return K(qkv).attn_fwd(qkv, heads)[0]


class _CrossAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, kv, heads):
        o, lse = K(q).xattn_fwd(q, kv, heads)
        ctx.heads = heads
        ctx.save_for_backward(q, kv, o, lse)
        return o

    @staticmethod
    def backward(ctx, do):
        q, kv, o, lse = ctx.saved_tensors
        dq, dkv = K(do).xattn_bwd(do.contiguous(), q, kv, o, lse, ctx.heads)
        return dq, dkv, None


def cross_attention(q, kv, heads: int):
    """Attention of the queries ``q`` [B, Sq, heads * 64] over a short key set ``kv`` [B, Sk, 2 *
    heads * 64] (k, then v row blocks, heads of 64 inside each), Sk <= 64: [B, Sq, heads * 64],
    scale 1/8, no mask, no dropout (PVT v2's spatial-reduction attention)."""
    if torch.is_grad_enabled() and (q.requires_grad or kv.requires_grad):
        return _CrossAttention.apply(q, kv, heads)
    return K(q).xattn_fwd(q, kv, heads)[0]


class _BiasGelu(torch.autograd.Function):
    """gelu(h + b): h is kept, and the GELU backward reduces b's gradient from the dh it stores."""

    @staticmethod
    def forward(ctx, h, b):
        ctx.b = b
        ctx.save_for_backward(h)
        return K(h).gelu_fwd(h, b)

    @staticmethod
    def backward(ctx, da):
        (h,) = ctx.saved_tensors
        b = ctx.b
        dh = K(da).gelu_bwd(da.contiguous(), h, _sink(b, da), b)
        _done(b)
        return dh, None


def dwconv_gelu(x, conv):
    """gelu(dwconv(x) + conv.bias): the conv runs bias-free and the GELU kernel adds the bias in
    fp32 (PVT v2's MLP)."""
    if not conv.depthwise or conv.bias is None:
        raise ValueError("dwconv_gelu: a depthwise Conv2d (groups == channels) with a bias expected")
    if torch.is_grad_enabled() and (conv.weight.requires_grad or x.requires_grad):
        return _BiasGelu.apply(_DwConv.apply(x, conv.weight, conv, None, None, None), conv.bias)
    sh, sw, ph, pw = conv.kgeom
    k = K(x)
    return k.gelu_fwd(k.dwconv_fwd(x, weight_of(conv.weight), sh, sw, ph, pw, _empty(x), _empty(x)),
                      conv.bias)


class _Tokens(torch.autograd.Function):
    @staticmethod
    def forward(ctx, patch, cls, pos):
        ctx.params = (cls, pos)
        return K(patch).tokens_fwd(patch, cls, pos)

    @staticmethod
    def backward(ctx, dx):
        cls, pos = ctx.params
        k = K(dx)
        dx = dx.contiguous()
        if not (cls.requires_grad and pos.requires_grad):  # frozen: sums into scratch
            tmp = torch.empty(cls.numel() + pos.numel(), device=dx.device, dtype=torch.float32)
            return k.tokens_bwd(dx, tmp[:cls.numel()], tmp[cls.numel():], True), None, None
        fresh = [_fresh(cls), _fresh(pos)]
        dpatch = k.tokens_bwd(dx, grad_sink(cls), grad_sink(pos), all(fresh))
        _done(cls, pos)
        return dpatch, None, None


def patch_tokens(x, embed, cls, pos):
    """ViT's front end: the NHWC image cut into ``embed.patch``-square patch rows, the patch
    embedding as a rows GEMM, then [cls | patches] + pos: [B, 1 + Np, D]."""
    rows = K(x).patchify(x, embed.patch)
    pr = linear_act(rows, embed)
    if not pr.is_contiguous():
        pr = pr.contiguous()
    if torch.is_grad_enabled() and (pr.requires_grad or cls.requires_grad or pos.requires_grad):
        return _Tokens.apply(pr, cls, pos)
    return K(pr).tokens_fwd(pr, cls, pos)


# ======================================= shifted-window attention and patch merging (Swin)
class _WindowAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, bias, heads, Hf, Wf, ws, shift):
        o, lse = K(qkv).wattn_fwd(qkv, bias, heads, Hf, Wf, ws, shift)
        ctx.bias, ctx.geom = bias, (heads, Hf, Wf, ws, shift)
        ctx.save_for_backward(qkv, lse)
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, lse = ctx.saved_tensors
        bias, k = ctx.bias, K(do)
        do = do.contiguous()
        if not bias.requires_grad:  # frozen: the bias gradient into scratch
            tmp = torch.empty(bias.numel(), device=do.device, dtype=torch.float32)
            return _grads(_WindowAttention, k.wattn_bwd(do, qkv, lse, bias, tmp, *ctx.geom, True))
        dqkv = k.wattn_bwd(do, qkv, lse, bias, grad_sink(bias), *ctx.geom, _fresh(bias))
        _done(bias)
        return _grads(_WindowAttention, dqkv)


def window_attention(qkv, bias, heads: int, Hf: int, Wf: int, ws: int, shift: int):
    """Swin's attention over the in-projection's rows ``qkv`` [B Hf Wf, 3 * heads * 32] in natural
    token order: softmax(q k^T / sqrt(32) + bias[h][rel] + shift mask) v inside every ws x ws
    window of the map rolled by ``shift``; ``bias`` holds heads * (2 ws - 1)^2 floats.  Returns
    rows [B Hf Wf, heads * 32] in the same order: no roll, partition or reverse pass exists."""
    if torch.is_grad_enabled() and (qkv.requires_grad or bias.requires_grad):
        return _WindowAttention.apply(qkv, bias, heads, Hf, Wf, ws, shift)
    return K(qkv).wattn_fwd(qkv, bias, heads, Hf, Wf, ws, shift)[0]


class _NeighborhoodAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, rpb, heads, Hf, Wf):
        o, lse = K(qkv).na_fwd(qkv, rpb, heads, Hf, Wf)
        ctx.rpb, ctx.geom = rpb, (heads, Hf, Wf)
        ctx.save_for_backward(qkv, lse)
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, lse = ctx.saved_tensors
        rpb, k = ctx.rpb, K(do)
        do = do.contiguous()
        if not rpb.requires_grad:  # frozen: the bias gradient into scratch
            tmp = torch.empty(rpb.numel(), device=do.device, dtype=torch.float32)
            return _grads(_NeighborhoodAttention, k.na_bwd(do, qkv, lse, rpb, tmp, *ctx.geom, True))
        dqkv = k.na_bwd(do, qkv, lse, rpb, grad_sink(rpb), *ctx.geom, _fresh(rpb))
        _done(rpb)
        return _grads(_NeighborhoodAttention, dqkv)


def neighborhood_attention(qkv, rpb, heads: int, Hf: int, Wf: int):
    """NAT's attention over the in-projection's rows ``qkv`` [B Hf Wf, 3 * heads * 32] in natural
    token order: every pixel attends the 7 x 7 neighbourhood centred on it (clamped to the map, so
    always 49 keys), softmax(q k^T / sqrt(32) + rpb[h][dy + 6][dx + 6]) v; ``rpb`` holds heads * 169
    floats.  Returns rows [B Hf Wf, heads * 32]: no gathered key or value tensor exists."""
    if torch.is_grad_enabled() and (qkv.requires_grad or rpb.requires_grad):
        return _NeighborhoodAttention.apply(qkv, rpb, heads, Hf, Wf)
    return K(qkv).na_fwd(qkv, rpb, heads, Hf, Wf)[0]


class _WindowAttentionCos(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, bias, logit_scale, heads, Hf, Wf, ws, shift):
        o, lse = K(qkv).wattn_cos_fwd(qkv, logit_scale, bias, heads, Hf, Wf, ws, shift)
        ctx.logit_scale, ctx.geom = logit_scale, (heads, Hf, Wf, ws, shift)
        ctx.save_for_backward(qkv, bias, lse)
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, bias, lse = ctx.saved_tensors
        ls, k = ctx.logit_scale, K(do)
        do = do.contiguous()
        # bias is an activation (cpb_bias's output): its gradient is returned, under the one
        # overwrite flag it shares with the logit-scale gradient
        if not ls.requires_grad:  # frozen: the logit-scale gradient into scratch
            dls, fresh = torch.empty(ls.numel(), device=do.device, dtype=torch.float32), True
        else:
            dls, fresh = grad_sink(ls), _fresh(ls)
        dbias = torch.empty_like(bias) if fresh else torch.zeros_like(bias)
        dqkv = k.wattn_cos_bwd(do, qkv, lse, ls, bias, dbias, dls, *ctx.geom, fresh)
        _done(ls)
        return _grads(_WindowAttentionCos, dqkv, dbias)


def window_attention_cos(qkv, logit_scale, bias, heads: int, Hf: int, Wf: int, ws: int, shift: int):
    """Swin V2's attention over the rows ``qkv`` [B Hf Wf, 3 * heads * 32] in natural token order:
    softmax(tau_h cos(q, k) + bias[h][rel] + shift mask) v inside every ws x ws window of the map
    rolled by ``shift``, tau_h = exp(min(logit_scale[h], ln 100)).  ``logit_scale`` is a [heads] fp32
    parameter, ``bias`` heads * (2 ws - 1)^2 fp32 (``cpb_bias``), differentiated through."""
    if torch.is_grad_enabled() and (qkv.requires_grad or bias.requires_grad or logit_scale.requires_grad):
        return _WindowAttentionCos.apply(qkv, bias, logit_scale, heads, Hf, Wf, ws, shift)
    return K(qkv).wattn_cos_fwd(qkv, logit_scale, bias, heads, Hf, Wf, ws, shift)[0]


class _CpbBias(torch.autograd.Function):
    @staticmethod
    def forward(ctx, w1, b1, w2, heads, ws):
        bias = K(w1).cpb_fwd(w1, b1, w2, heads, ws)
        ctx.params, ctx.geom = (w1, b1, w2), (heads, ws)
        ctx.save_for_backward(bias)
        return bias

    @staticmethod
    def backward(ctx, dbias):
        (bias,) = ctx.saved_tensors
        w1, b1, w2 = ctx.params
        k = K(dbias)
        dbias = dbias.contiguous()
        if not (w1.requires_grad and b1.requires_grad and w2.requires_grad):  # frozen: into scratch
            tmp = [torch.empty_like(p, dtype=torch.float32) for p in ctx.params]
            k.cpb_bwd(dbias, bias, w1, b1, w2, *tmp, *ctx.geom, True)
            return _grads(_CpbBias)
        fresh = [_fresh(p) for p in ctx.params]
        k.cpb_bwd(dbias, bias, w1, b1, w2, grad_sink(w1), grad_sink(b1), grad_sink(w2), *ctx.geom, all(fresh))
        _done(w1, b1, w2)
        return _grads(_CpbBias)


def cpb_bias(w1, b1, w2, heads: int, ws: int):
    """Swin V2's continuous position bias, [heads * (2 ws - 1)^2] fp32 head-major:
    16 sigmoid(w2 relu(w1 coord + b1)) over the log-spaced relative coordinates of a ws x ws window
    (``w1`` [512, 2], ``b1`` [512], ``w2`` [heads, 512], fp32 parameters)."""
    if torch.is_grad_enabled() and (w1.requires_grad or b1.requires_grad or w2.requires_grad):
        return _CpbBias.apply(w1, b1, w2, heads, ws)
    return K(w1).cpb_fwd(w1, b1, w2, heads, ws)


class _PatchMerge(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, P=2):
        ctx.hw, ctx.P = (x.shape[1], x.shape[2]), P
        return K(x).patchify(x, P)

    @staticmethod
    def backward(ctx, drows):
        return K(drows).unpatchify(drows.contiguous(), ctx.hw[0], ctx.hw[1], ctx.P), None


def patch_rows(x, P: int):
    """NHWC [B, Hf, Wf, C] -> rows [B Hf/P Wf/P, P P C], each P x P cell in (ky, kx, c) order: the
    rows GEMM over them is the conv with kernel = stride = P (PVT's spatial reduction)."""
    if torch.is_grad_enabled() and x.requires_grad:
        return _PatchMerge.apply(x, P)
    return K(x).patchify(x, P)


def patch_merge_rows(x):
    """Swin's patch merging gather: NHWC [B, Hf, Wf, C] -> rows [B Hf/2 Wf/2, 4 C], each 2 x 2 cell
    in (ky, kx, c) order (``patchify`` forward, ``unpatchify`` backward)."""
    if torch.is_grad_enabled() and x.requires_grad:
        return _PatchMerge.apply(x)
    return K(x).patchify(x, 2)


class _JoinInput(torch.autograd.Function):
    """Identity in front of one consumer of an activation whose gradient contributions meet in
    ``join``: its backward hands the consumer's gradient in."""

    @staticmethod
    def forward(ctx, x, join):
        ctx.join = join
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return ctx.join.add(K(g), g.contiguous()), None


class _ResidualAdd(torch.autograd.Function):
    """y += x in place (``add_bf16_``: fp32 add, one rounding).  dout goes to y's branch as it
    is and to x through the join, where it meets the gradient of x's other consumer."""

    @staticmethod
    def forward(ctx, y, x, join):
        ctx.join = join
        K(y).add_bf16_(y, x)
        ctx.mark_dirty(y)
        return y

    @staticmethod
    def backward(ctx, dout):
        dout = dout.contiguous()
        dres = None
        if ctx.needs_input_grad[1]:
            dres = dout if ctx.join is None else ctx.join.add(K(dout), dout)
        return dout, dres, None


def residual_branch(x):
    """(x for the branch, join) of a pre-norm residual block ``x + f(x)``: the branch's input
    gradient and the skip's meet in the join with one ``add_bf16_``, no autograd add."""
    if torch.is_grad_enabled() and x.requires_grad:
        join = GradJoin(2)
        return _JoinInput.apply(x, join), join
    return x, None


def fan_out(x, n: int = 2):
    """``n`` views of an activation that feeds ``n`` ops (PVT's normalised tokens: the query
    projection and the key / value path): their input gradients meet in one join."""
    if torch.is_grad_enabled() and x.requires_grad:
        join = GradJoin(n)
        return tuple(_JoinInput.apply(x, join) for _ in range(n))
    return (x,) * n


def residual_add(y, x, join: Optional[GradJoin] = None):
    """x + y, written into ``y`` (a fresh branch output, contiguous, same shape)."""
    if not y.is_contiguous():
        y = y.contiguous()
    if torch.is_grad_enabled() and (y.requires_grad or x.requires_grad):
        if y.is_leaf:
            y = y.clone()
        return _ResidualAdd.apply(y, x.contiguous(), join)
    K(y).add_bf16_(y, x.contiguous())
    return y


# ================================================== BN -> activation -> squeeze-excite gate
ACT_NONE, ACT_RELU, ACT_HARDSWISH = 0, 1, 2


def _se_params(se):
    if se is None:
        return None, None, None, None
    return se.fc1.weight, se.fc1.bias, se.fc2.weight, se.fc2.bias


class _BNActGate(torch.autograd.Function):
    """u = act(bn(z)) * gate, train mode, on the se.hip kernels: bn_stats_affine, then (with an
    SE layer) act_pool -> se_gate, then act_gate_fwd.  act(bn(z)) is never stored: the backward
    recomputes it from z.  Saved: z and per-channel / per-(image, channel) vectors."""

    @staticmethod
    def forward(ctx, z, gamma, beta, bn, act, stats, w1, b1, w2, b2):
        k = K(z)
        if stats is None:
            stats = k.bn_stats(z, bn.running_mean)
        mean, rstd, aff = k.bn_stats_affine(z, stats, gamma, beta, bn.running_mean,
                                            bn.running_var, bn.momentum_value(), bn.eps,
                                            bn.num_batches_tracked)
        pooled = h = gate = None
        if w1 is not None:
            pooled = k.act_pool(z, aff, act)
            h, gate = k.se_gate(pooled, weight_of(w1), b1, weight_of(w2), b2)
        ctx.act = act
        ctx.params = (gamma, beta, w1, b1, w2, b2)
        ctx.save_for_backward(z, mean, rstd, aff, pooled, h, gate)
        return k.act_gate_fwd(z, aff, act, _or_empty(gate, z))

    @staticmethod
    def backward(ctx, du):
        z, mean, rstd, aff, pooled, h, gate = ctx.saved_tensors
        gamma, beta, w1, b1, w2, b2 = ctx.params
        k = K(du)
        du = du.contiguous()
        act = ctx.act
        dpool = None
        if gate is not None:
            dgate = k.act_gate_bwd_pool(du, z, aff, act)
            dpre2, dpre1, dpool = k.se_gate_bwd(dgate, h, gate, weight_of(w1), weight_of(w2),
                                                1.0 / (z.shape[1] * z.shape[2]))

            def wgrad():
                for w, b, dpre, inp in ((w2, b2, dpre2, h), (w1, b1, dpre1, pooled)):
                    if w.requires_grad:
                        bs = _sink(b, du)
                        fresh = _fresh(w)  # (both flags are consumed)
                        fresh = (_fresh(b) if bs.numel() else True) and fresh
                        k.se_fc_wgrad(dpre, inp, grad_sink(w), bs, overwrite=fresh)
                        _done(w, b)
            _run_wgrad(wgrad, dpre2, h, dpre1, pooled)
        sums = k.act_gate_bwd_sums(du, z, aff, act, _or_empty(gate, du), _or_empty(dpool, du),
                                   mean, rstd)
        for p, row in ((gamma, 1), (beta, 0)):  # dgamma = sum g xhat, dbeta = sum g
            sink = _sink(p, du)
            if sink.numel():
                k.add_f32_(sink, sums[row])
        _done(gamma, beta)
        dz = None
        if ctx.needs_input_grad[0]:
            dz = k.act_gate_bwd_dx(du, z, aff, act, _or_empty(gate, du), _or_empty(dpool, du),
                                   mean, rstd, gamma, sums)
        return _grads(_BNActGate, dz)


def _eval_affine(bn):
    """An eval-mode BN as the [2, C] affine the se.hip kernels apply."""
    sc = bn.weight.float() * torch.rsqrt(bn.running_var + bn.eps)
    return torch.stack([sc, bn.bias.float() - bn.running_mean * sc]).contiguous()


def bn_act_gate(z, bn, act: int, se=None, stats: Optional[torch.Tensor] = None):
    """act(bn(z)) * gate with act in (ACT_NONE, ACT_RELU, ACT_HARDSWISH); ``se``: a
    SqueezeExcitation layer, whose per-(image, channel) gate is hardsigmoid(fc2(relu(fc1(mean
    over H x W of act(bn(z)))))), or None (no gate); ``stats`` (train mode): z's [mean | var]
    from its producer's epilogue."""
    w1, b1, w2, b2 = _se_params(se)
    if bn.training:
        return _BNActGate.apply(z, bn.weight, bn.bias, bn, act, stats, w1, b1, w2, b2)
    k = K(z)
    aff = _eval_affine(bn)
    gate = _empty(z)
    if se is not None:
        _h, gate = k.se_gate(k.act_pool(z, aff, act), weight_of(w1), b1, weight_of(w2), b2)
    return k.act_gate_fwd(z, aff, act, gate)


def dwconv_bn_act_gate(x, conv, bn, act: int, se=None):
    """bn_act_gate(dwconv(x)): train mode takes the BN statistics from the conv's epilogue.
    ReLU without a gate is ``dwconv_bn_act``."""
    if act == ACT_RELU and se is None:
        return dwconv_bn_act(x, conv, bn, relu=True)
    if bn.training:
        stats = torch.empty(2, conv.out_channels, device=x.device, dtype=torch.float32)
        z = dwconv(x, conv, stats, None if _NO_SHIFT else bn.running_mean)
        return bn_act_gate(z, bn, act, se, stats)
    return bn_act_gate(dwconv(x, conv), bn, act, se)


def conv_bn_act_gate(x, conv, bn, act: int):
    """act(bn(conv(x))) for a bias-free conv; ReLU and identity are ``conv_bn_act``."""
    if act != ACT_HARDSWISH:
        return conv_bn_act(x, conv, bn, relu=act == ACT_RELU)
    if bn.training:
        stats = torch.empty(2, conv.cout_store, device=x.device, dtype=torch.float32)
        z = conv_act(x, conv, False, stats=stats, shift=None if _NO_SHIFT else bn.running_mean)
        return bn_act_gate(z, bn, act, None, stats)
    return bn_act_gate(conv_act(x, conv, False), bn, act)


class _Hardswish(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, aff):
        ctx.save_for_backward(x, aff)
        return K(x).act_gate_fwd(x, aff, ACT_HARDSWISH, _empty(x))

    @staticmethod
    def backward(ctx, dy):
        x, aff = ctx.saved_tensors
        e = _empty(dy)
        return K(dy).act_gate_bwd_dx(dy.contiguous(), x, aff, ACT_HARDSWISH, e, e, e, e, e, e), None


def hardswish(x):
    """x * relu6(x + 3) / 6 (act_gate_fwd with the unit affine [1 | 0], no gate)."""
    C = x.shape[-1]
    key = ("hswish", C, x.device)
    aff = _UNIT.get(key)
    if aff is None:
        aff = _UNIT[key] = torch.stack([torch.ones(C, device=x.device),
                                        torch.zeros(C, device=x.device)])
    x = x.contiguous()
    if torch.is_grad_enabled() and x.requires_grad:
        return _Hardswish.apply(x, aff)
    return K(x).act_gate_fwd(x, aff, ACT_HARDSWISH, _empty(x))


# ========================================================================== grouped conv
class _GConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, conv, stats=None, shift=None):
        k = K(x)
        sh, sw, ph, pw = conv.kgeom
        z = k.gconv_fwd(x, weight_of(w), sh, sw, ph, pw, _or_empty(stats, x),
                        _or_empty(shift, x))
        ctx.conv, ctx.w = conv, w
        ctx.in_hw = (x.shape[1], x.shape[2])
        ctx.save_for_backward(x)
        return z

    @staticmethod
    def backward(ctx, dz):
        (x,) = ctx.saved_tensors
        w, conv = ctx.w, ctx.conv
        k = K(dz)
        dz = dz.contiguous()
        sh, sw, ph, pw = conv.kgeom
        if w.requires_grad:
            def wgrad():
                k.gconv_wgrad(dz, x, w.grad, sh, sw, ph, pw, overwrite=_fresh(w))
                _done(w)
            _run_wgrad(wgrad, dz, x)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = k.gconv_dgrad(dz, weight_of(w), *ctx.in_hw, sh, sw, ph, pw)
        return _grads(_GConv, dx)


def gconv(x, conv, stats: Optional[torch.Tensor] = None, shift: Optional[torch.Tensor] = None):
    """Grouped 3x3 conv (``conv.grouped``, no bias); ``stats`` ([2, C] fp32): receives the
    output's per-channel [mean | var] from the kernel's epilogue (sums shifted by ``shift``) in
    the format ``bn_act(stats=)`` takes."""
    if not conv.grouped or conv.bias is not None:
        raise ValueError("gconv: a bias-free grouped 3x3 Conv2d expected")
    if torch.is_grad_enabled() and (conv.weight.requires_grad or x.requires_grad):
        return _GConv.apply(x, conv.weight, conv, stats, shift)
    sh, sw, ph, pw = conv.kgeom
    return K(x).gconv_fwd(x, weight_of(conv.weight), sh, sw, ph, pw, _or_empty(stats, x),
                          _or_empty(shift, x))


def gconv_bn_act(x, conv, bn, relu: bool = True):
    """relu?(bn(gconv(x))): train mode takes the BN statistics from the conv's epilogue."""
    if bn.training:
        stats = torch.empty(2, conv.out_channels, device=x.device, dtype=torch.float32)
        z = gconv(x, conv, stats, None if _NO_SHIFT else bn.running_mean)
        return bn_act(z, bn, relu=relu, stats=stats)
    return bn_act(gconv(x, conv), bn, relu=relu)


# =========================================================================== standalone BN
class _BNAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, bn, relu, stats=None, out=None):
        k = K(x)
        y, mean, rstd = k.bn_fwd_train(x, _or_empty(stats, x), gamma, beta, bn.running_mean,
                                       bn.running_var, bn.momentum_value(), bn.eps, _empty(x),
                                       relu, bn.num_batches_tracked, out=out)
        ctx.params = (gamma, beta)
        # relu(bn(x)) with an affine BN recomputes its mask from x: y is not kept
        zmask = relu and beta is not None and gamma is not None
        ctx.zmask = zmask
        ctx.save_for_backward(x, y if (relu and not zmask) else None, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, mean, rstd = ctx.saved_tensors
        gamma, beta = ctx.params
        k = K(dy)
        dy = _rows(dy)
        dx, _g = k.bn_bwd(dy, x, _or_empty(y, dy), mean, rstd, gamma, _sink(gamma, dy),
                          _sink(beta, dy), bool(ctx.needs_input_grad[0]), False,
                          beta if ctx.zmask else None)
        _done(gamma, beta)
        return dx, None, None, None, None, None, None


def bn_act(x, bn, relu: bool = True, stats: Optional[torch.Tensor] = None,
           out: Optional[torch.Tensor] = None):
    """relu?(bn(x)); ``stats`` (train mode): x's [mean | var] [2, C] when already known
    (a DenseNet block's per-feature statistics), saving the statistics pass; ``out`` (train
    mode): a channel window of a wider buffer to write the result into."""
    if bn.training:
        return _BNAct.apply(x, bn.weight, bn.bias, bn, relu, stats, out)
    return K(x).bn_fwd_eval(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps,
                            _empty(x), relu)


class _BNReluAvgPool2(torch.autograd.Function):
    """avg_pool2d(relu(bn(x)), 2, 2), train mode, the BN output never written: the
    statistics half (bn_stats_affine) then one pass that applies BN + ReLU while pooling.
    Backward: avgpool_bwd, then the BN backward with the mask recomputed from x."""

    @staticmethod
    def forward(ctx, x, gamma, beta, bn, stats=None):
        k = K(x)
        if stats is None:
            stats = k.bn_stats(x, bn.running_mean)
        mean, rstd, aff = k.bn_stats_affine(x, stats, gamma, beta, bn.running_mean,
                                            bn.running_var, bn.momentum_value(), bn.eps,
                                            bn.num_batches_tracked)
        ctx.params = (gamma, beta)
        ctx.hw = (x.shape[1], x.shape[2])
        ctx.save_for_backward(x, mean, rstd)
        return k.bn_relu_avgpool2_fwd(x, aff)

    @staticmethod
    def backward(ctx, dp):
        x, mean, rstd = ctx.saved_tensors
        gamma, beta = ctx.params
        k = K(dp)
        dy = k.avgpool_bwd(dp.contiguous(), ctx.hw[0], ctx.hw[1], 2, 2, 2, 2, 0, 0, False, True)
        dx, _g = k.bn_bwd(dy, x, _empty(dy), mean, rstd, gamma, _sink(gamma, dy),
                          _sink(beta, dy), bool(ctx.needs_input_grad[0]), False, beta)
        _done(gamma, beta)
        return dx, None, None, None, None


def bn_relu_avgpool2(x, bn, stats: Optional[torch.Tensor] = None):
    """avg_pool2d(relu(bn(x)), 2, 2) (DenseNet transitions with the pool ahead of the conv);
    train mode with an affine BN, even H and W; other cases compose the two ops."""
    if (bn.training and bn.weight is not None and bn.bias is not None and x.shape[1] % 2 == 0
            and x.shape[2] % 2 == 0 and x.shape[3] % 8 == 0):
        return _BNReluAvgPool2.apply(x, bn.weight, bn.bias, bn, stats)
    return avg_pool2d(bn_act(x, bn, True, stats), (2, 2), (2, 2))


# ================================================================================ linear
class _LinearAct(torch.autograd.Function):
    """y = act(x W^T + b) over the layer's padded output width; returns the first
    ``nout`` columns (a view) when the layer stores padded rows (layers.Linear).  ``dead``: a
    (begin, end) range of the bias that the model holds at zero (Swin V2's k bias): its
    gradient is cleared before the bias is reported done."""

    @staticmethod
    def forward(ctx, x, w, b, relu, nout, dead=None):
        ctx.dead = dead
        k = K(x)
        y = k.linear_fwd(x, weight_of(w), _or_empty(b, x), relu)
        ctx.relu = relu
        ctx.params = (w, b)
        ctx.nout = nout
        ctx.save_for_backward(x, y if relu else None)
        return y if nout == y.shape[1] else y[:, :nout]

    @staticmethod
    def backward(ctx, dy):
        x, y = ctx.saved_tensors
        w, b = ctx.params
        k = K(dy)
        dy = _padded_grad(dy, w.shape[0])
        g = k.act_bwd(dy, _or_empty(y, dy), _sink(b, dy))
        # dgrad before the weight gradient: the rest of the backward chain waits for dx,
        # nothing waits for w.grad before its bucket closes
        dx = (k.linear_dgrad(g, weight_of(w), weight_t_of(w)) if ctx.needs_input_grad[0]
              else None)
        if ctx.dead is not None and b is not None and b.requires_grad:
            k.zero_f32(grad_sink(b)[ctx.dead[0]:ctx.dead[1]])
        _done(b)
        if w.requires_grad:
            k.linear_wgrad(g, x, w.grad, overwrite=_fresh(w))
            _done(w)
        return dx, None, None, None, None, None


def _padded_grad(dy, width: int):
    """Gradient of a padded layer's output view as a contiguous [B, width] tensor.  The
    cross-entropy backward already returns a view of a [B, width] buffer with zero padding
    columns - use that buffer (ce_bwd wrote its zeros:
    tests/test_kernels_gpu.py::test_cross_entropy_padded_rows); anything else is
    zero-padded by a copy."""
    if dy.shape[1] == width:
        return dy.contiguous()
    base = dy._base
    if (base is not None and base.dim() == 2 and tuple(base.shape) == (dy.shape[0], width)
            and base.is_contiguous() and dy.data_ptr() == base.data_ptr()
            and dy.stride() == base.stride()):
        return base  # (ce_bwd wrote zeros into the padding columns)
    return torch.nn.functional.pad(dy, (0, width - dy.shape[1])).contiguous()


def linear_act(x, lin, relu: bool = False, dead_bias=None):
    nout = getattr(lin, "out_features", lin.weight.shape[0])
    if torch.is_grad_enabled() and (lin.weight.requires_grad or x.requires_grad):
        return _LinearAct.apply(x, lin.weight, lin.bias, relu, nout, dead_bias)
    y = K(x).linear_fwd(x, weight_of(lin.weight), _or_empty(lin.bias, x), relu)
    return y if nout == y.shape[1] else y[:, :nout]


# ================================================================================= pools
class _MaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cfg, join=None, link_in=None):
        y, idx = K(x).maxpool_fwd(x, *cfg)
        ctx.cfg = cfg
        ctx.join = join
        ctx.link_in = link_in
        ctx.hw = (x.shape[1], x.shape[2])
        ctx.save_for_backward(idx, y if link_in is not None else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        idx, y = ctx.saved_tensors
        k = K(dy)
        dy = dy.contiguous()
        li = ctx.link_in
        if li is not None and ctx.join is None:
            # the input is a ReLU output whose producer handed its backward over (BNLink):
            # route only where the pooled value is > 0 and return the producer's bias sums
            r = k.maxpool_bwd_relu(dy, idx, y, ctx.hw[0], ctx.hw[1], *ctx.cfg[:6])
            if r is not None:
                li.sums = r[1]
                return _grads(_MaxPool, r[0])
        dx = k.maxpool_bwd(dy, idx, ctx.hw[0], ctx.hw[1], *ctx.cfg)
        return _grads(_MaxPool, dx if ctx.join is None else ctx.join.add(k, dx))


def max_pool2d(x, kernel, stride, padding=(0, 0), ceil_mode=False,
               join: Optional[GradJoin] = None, link_in: Optional[BNLink] = None):
    """``join``: the input's other consumers share it (see GradJoin); ``link_in``: the input
    is a conv -> ReLU output that feeds only this pool, and the pool's backward applies the
    ReLU mask and reduces the conv's bias gradient (Fn.BNLink; 2x2/s2 pools)."""
    cfg = (kernel[0], kernel[1], stride[0], stride[1], padding[0], padding[1], bool(ceil_mode))
    if torch.is_grad_enabled() and x.requires_grad:
        return _MaxPool.apply(x, cfg, join, link_in)
    return K(x).maxpool_fwd(x, *cfg)[0]


class _AvgPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cfg, join=None):
        ctx.cfg = cfg
        ctx.join = join
        ctx.hw = (x.shape[1], x.shape[2])
        return K(x).avgpool_fwd(x, *cfg)

    @staticmethod
    def backward(ctx, dy):
        k = K(dy)
        dx = k.avgpool_bwd(dy.contiguous(), ctx.hw[0], ctx.hw[1], *ctx.cfg)
        return _grads(_AvgPool, dx if ctx.join is None else ctx.join.add(k, dx))


def avg_pool2d(x, kernel, stride, padding=(0, 0), ceil_mode=False, count_include_pad=True,
               join: Optional[GradJoin] = None):
    cfg = (kernel[0], kernel[1], stride[0], stride[1], padding[0], padding[1], bool(ceil_mode),
           bool(count_include_pad))
    if torch.is_grad_enabled() and x.requires_grad:
        return _AvgPool.apply(x, cfg, join)
    return K(x).avgpool_fwd(x, *cfg)


class _AdaptiveAvgPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, oh, ow):
        ctx.hw = (x.shape[1], x.shape[2])
        return K(x).adaptive_avgpool_fwd(x, oh, ow)

    @staticmethod
    def backward(ctx, dy):
        return K(dy).adaptive_avgpool_bwd(dy.contiguous(), ctx.hw[0], ctx.hw[1]), None, None


def adaptive_avg_pool2d(x, out_hw):
    oh, ow = out_hw
    if torch.is_grad_enabled() and x.requires_grad:
        return _AdaptiveAvgPool.apply(x, oh, ow)
    return K(x).adaptive_avgpool_fwd(x, oh, ow)


# ============================================================ concat at channel offsets
class _ChannelBuffer(torch.autograd.Function):
    """The channel concat of ``parts`` that their producers already wrote into their
    windows of ``buf`` (``out=`` of conv_bn_act / bn_act / conv1x1_group): forward returns
    the buffer (a part NOT at its window is copied in), backward hands each part its
    window of the gradient - a row-strided view, which the BN backward kernels read in
    place.  SURVEY K13: torchvision's ``torch.cat`` of Inception branch outputs
    (``/root/reference/models.py:83-95``) without the copy kernels."""

    @staticmethod
    def forward(ctx, buf, *parts):
        k = K(buf)
        o = 0
        ctx.sizes = []
        for t in parts:
            n = t.shape[-1]
            win = buf[..., o:o + n]
            if t.data_ptr() != win.data_ptr() or t.stride() != win.stride():
                k.chan_insert(buf, o, t.contiguous())
            ctx.sizes.append(n)
            o += n
        return buf.view(buf.shape)

    @staticmethod
    def backward(ctx, dy):
        s = _BR["stream"] if _BR["on"] else None
        if s is not None and dy.is_cuda:
            dy.record_stream(s)  # (a window may be read by a side-branch chain)
        outs, o = [], 0
        for n in ctx.sizes:
            outs.append(dy[..., o:o + n])
            o += n
        return (None,) + tuple(outs)


class ChannelBuffer:
    """An NHWC block output [N, H, W, sum(widths)] whose branches write their results at
    their channel offsets: ``window(i)`` is branch i's destination (pass it as ``out=``),
    ``gather(parts)`` the concat (no copy for parts already in place)."""

    def __init__(self, like: torch.Tensor, hw, widths):
        self.widths = list(widths)
        self.offs = [sum(self.widths[:i]) for i in range(len(self.widths))]
        self.buf = torch.empty((like.shape[0], hw[0], hw[1], sum(self.widths)),
                               device=like.device, dtype=like.dtype)

    def window(self, i: int) -> torch.Tensor:
        o = self.offs[i]
        return self.buf[..., o:o + self.widths[i]]

    def gather(self, parts):
        if torch.is_grad_enabled() and any(t.requires_grad for t in parts):
            return _ChannelBuffer.apply(self.buf, *parts)
        k = K(self.buf)
        for i, t in enumerate(parts):
            w = self.window(i)
            if t.data_ptr() != w.data_ptr():
                k.chan_insert(self.buf, self.offs[i], t.contiguous())
        return self.buf


# ======================================================================== channel concat
class _Concat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *xs):
        ctx.sizes = [x.shape[-1] for x in xs]
        return K(xs[0]).concat_channels(list(xs))

    @staticmethod
    def backward(ctx, dy):
        return tuple(K(dy).split_channels(dy.contiguous(), ctx.sizes))


def cat_channels(xs):
    """NHWC channel concat (torchvision's ``torch.cat(dim=1)`` on NCHW) [K13]: one native
    strided-copy kernel forward, the matching split kernel backward."""
    xs = [x.contiguous() for x in xs]
    if len(xs) == 1:
        return xs[0]
    if torch.is_grad_enabled() and any(x.requires_grad for x in xs):
        return _Concat.apply(*xs)
    return K(xs[0]).concat_channels(xs)


# =============================================================================== dropout
class DropoutRNG:
    """Stream position of the dropout masks, so every call draws a fresh mask.

    GPU: a device int32 counter per device, read by the dropout kernel as its offset and
    advanced on the stream after every call.  A HIP graph replays both, so each replay of a
    captured step draws new masks (a host-side offset would be frozen into the graph at
    capture, and every replay would reuse one mask).  CPU: a host counter.  The seed is a
    host constant.  ``state()`` / ``set_state()`` snapshot both (TrainStep.capture)."""
    seed = 0
    offset = 0
    _counters = {}

    @classmethod
    def counter(cls, device: torch.device) -> torch.Tensor:
        c = cls._counters.get(device)
        if c is None:
            c = cls._counters[device] = torch.zeros(1, dtype=torch.int32, device=device)
        return c

    @classmethod
    def state(cls):
        # (the current GPU's counter is created here if no dropout ran yet: a snapshot taken
        # before the first dropout call must still pin the position that call will start
        # from - otherwise set_state() cannot rewind it, e.g. TrainStep.capture's warm-up
        # steps in a process whose first dropout they are)
        if torch.cuda.is_available():
            cls.counter(torch.device("cuda", torch.cuda.current_device()))
        return cls.offset, {d: c.clone() for d, c in cls._counters.items()}

    @classmethod
    def set_state(cls, st) -> None:
        cls.offset = st[0]
        for d, c in st[1].items():
            cls.counter(d).copy_(c)


def _dropout_fwd(x, p):
    if x.is_cuda:  # offset = the device counter (advanced by the kernel launch pair)
        return K(x).dropout_fwd(x, p, DropoutRNG.seed, 0, DropoutRNG.counter(x.device))
    DropoutRNG.offset += 1
    return K(x).dropout_fwd(x, p, DropoutRNG.seed, DropoutRNG.offset)


class _Dropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p):
        y, mask = _dropout_fwd(x, p)
        ctx.p = p
        ctx.save_for_backward(mask)
        return y

    @staticmethod
    def backward(ctx, dy):
        (mask,) = ctx.saved_tensors
        return K(dy).dropout_bwd(dy.contiguous(), mask, ctx.p), None


def dropout(x, p: float, training: bool):
    if not training or p == 0.0:
        return x
    if torch.is_grad_enabled() and x.requires_grad:
        return _Dropout.apply(x, p)
    return _dropout_fwd(x, p)[0]


# ========================================================================= cross-entropy
class _CrossEntropy(torch.autograd.Function):
    """sum_h weight_h * CE(logits_h, labels) as ONE native op: each head's fused
    log-softmax + NLL kernel adds its weighted mean into the loss scalar (and into the
    trainer's running loss sum ``acc``), the backward scales each head's softmax gradient
    by its weight - no elementwise ATen ops for Inception's ``loss + 0.4 * aux_loss``."""

    @staticmethod
    def forward(ctx, labels, weights, acc, smoothing, mix, bias, *logits):
        k = K(logits[0])
        out = torch.empty(1, device=logits[0].device, dtype=torch.float32)
        adj = {} if bias is None else {"bias": bias}  # (off: the call it always was)
        lses = [k.ce_fwd_weighted(lg, labels, out, _or_empty(acc, lg), float(w), i > 0, smoothing,
                                  *mix, **adj)
                for i, (lg, w) in enumerate(zip(logits, weights))]
        ctx.weights = weights
        ctx.smoothing = smoothing  # one eps for every head, as a torch criterion applies it
        ctx.mixed = bool(mix)      # ... and one (labels2, lam): the aux head mixes the same way
        ctx.adjusted = bias is not None  # ... and one bias: the aux head has the same classes
        ctx.save_for_backward(labels, *mix, *([] if bias is None else [bias]), *logits, *lses)
        return out.reshape(())

    @staticmethod
    def backward(ctx, go):
        saved = ctx.saved_tensors
        labels, rest, n = saved[0], saved[1:], len(ctx.weights)
        mix = rest[:2] if ctx.mixed else ()
        rest = rest[len(mix):]
        adj = {}
        if ctx.adjusted:
            adj, rest = {"bias": rest[0]}, rest[1:]
        logits, lses = rest[:n], rest[n:]
        go = go.reshape(1).float().contiguous()
        gs = [K(lg).ce_bwd(lg, labels, lse, go, float(w), ctx.smoothing, *mix, **adj)
              for lg, lse, w in zip(logits, lses, ctx.weights)]
        return (None, None, None, None, None, None) + tuple(gs)


def cross_entropy(logits, labels, weight: float = 1.0, acc: Optional[torch.Tensor] = None,
                  heads=None, label_smoothing: float = 0.0, labels2=None, lam=None,
                  logit_bias=None):
    """Mean softmax cross-entropy (``nn.CrossEntropyLoss()`` at main.py:134,150).

    ``heads``: extra (logits, weight) terms summed into the same loss (Inception aux);
    ``acc``: a float32 device scalar the loss is also added to (no host sync);
    ``label_smoothing``: torch's ``label_smoothing`` in [0, 1], applied to every head;
    ``labels2`` / ``lam`` (int64 / float32 [B] on the logits' device; Mixup / CutMix): row
    r's target is lam[r] * onehot(labels[r]) + (1 - lam[r]) * onehot(labels2[r]), for every
    head; lam is read on the device, so a captured graph replays with new weights;
    ``logit_bias`` (float32 [>= NC] on the logits' device; logit adjustment, Menon et al.
    2021): the loss is that of ``float(logits) + logit_bias[:NC]``, for every head - the
    add happens in fp32 inside the loss kernels, the logits themselves are not changed."""
    eps = float(label_smoothing)
    if not 0.0 <= eps <= 1.0:
        raise ValueError("label_smoothing must be in [0, 1], got %r" % (label_smoothing,))
    if (labels2 is None) != (lam is None):
        raise ValueError("cross_entropy: labels2 and lam go together")
    mix = () if labels2 is None else (labels2, lam)
    lg = [logits] + [h[0] for h in (heads or [])]
    ws = (float(weight),) + tuple(float(h[1]) for h in (heads or []))
    if torch.is_grad_enabled() and any(t.requires_grad for t in lg):
        return _CrossEntropy.apply(labels, ws, acc, eps, mix, logit_bias, *lg)
    k = K(logits)
    out = torch.empty(1, device=logits.device, dtype=torch.float32)
    adj = {} if logit_bias is None else {"bias": logit_bias}
    for i, (t, w) in enumerate(zip(lg, ws)):
        k.ce_fwd_weighted(t, labels, out, _or_empty(acc, t), w, i > 0, eps, *mix, **adj)
    return out.reshape(())


def count_correct(logits, labels, count: torch.Tensor) -> None:
    """count += #(argmax(logits) == labels)  (main.py:182-183)."""
    K(logits).argmax_correct(logits, labels, count)


def count_class_stats(logits, labels, count: torch.Tensor, stats: torch.Tensor) -> None:
    """``count_correct`` and, in the same pass over the logits, per-class counters:
    ``stats`` int64 [3, NC] += (support, predicted, true positives) of the rows whose label
    is in [0, NC) (``metrics.macro_scores`` turns them into macro-F1 / balanced accuracy)."""
    K(logits).argmax_stats(logits, labels, count, stats)


def count_topk(logits, labels, k: int, count: torch.Tensor) -> None:
    """count += #(labels among the k largest logits), ties to the lower index."""
    K(logits).topk_correct(logits, labels, int(k), count)


def predict_topk(logits, k: int, idx: Optional[torch.Tensor] = None,
                 prob: Optional[torch.Tensor] = None):
    """The k (1..16) best classes of every row and their softmax probabilities, in one pass
    over the logits: ``idx`` int32 [B, k] in ``count_topk``'s order (ties to the lower index,
    -1 past the last class that is neither NaN nor -inf) and ``prob`` float32 [B, k].  Given
    tensors (row windows of larger buffers, say) are written; missing ones are allocated.
    Returns (idx, prob)."""
    k = int(k)
    B = logits.shape[0]
    if idx is None:
        idx = torch.empty(B, max(k, 0), dtype=torch.int32, device=logits.device)
    if prob is None:
        prob = torch.empty(B, max(k, 0), dtype=torch.float32, device=logits.device)
    K(logits).topk_predict(logits, k, idx, prob)
    return idx, prob


def preprocess(img_u8, out_hw, mean, std, mode: int = 0, cpad: int = 3,
               out_dtype=torch.bfloat16, pad=None, extents=None, boxes=None, mix=None, lam=None):
    """u8 [B,H,W,3] -> resized, normalized NHWC with ``cpad`` channels, optionally on a
    zero-bordered canvas ``pad`` = (top, bottom, left, right) (the pre-padded input layout
    of a pixel-pair stem, ``models.layers.Conv2d.input_spec``).

    mode 0: bilinear, no antialias (the train transform, main.py:62-65); mode 1: PIL-exact
    bicubic (the eval transform, evaluation_pipeline.py:89, data/pil_resize.py); mode 2:
    float antialiased bicubic (torch ``F.interpolate(antialias=True)`` semantics).
    ``extents`` (host int [B, 2]): image b occupies rows [0, h_b) and columns [0, w_b) of
    its slot (real images of different sizes decoded into one padded batch).
    ``boxes`` (host int [B, 5], mode 0): rows (y0, x0, h, w, flip) - image b is resized
    from that crop of its slot instead of its whole extent (same arithmetic as resizing
    the contiguous crop) and the result is mirrored along W when flip is 1: random-resized
    crop + horizontal flip in the same launch (``data/augment.py`` samples the rows).  A
    box outside its image's extent raises ``ValueError`` here; the kernel does not check.
    ``mix`` (host int [B, 5]) and ``lam`` (host float [B]), mode 0, both or neither - Mixup /
    CutMix in the same launch: rows (partner, y0, x0, h, w) name an image of the same batch
    and a rectangle in output pixels (inside the canvas border; h or w 0: none).  With P
    the launch's result without them, image b becomes P[partner] inside its rectangle and
    bf16(lam * P[b] + (1 - lam) * P[partner]) outside it, bitwise that fp32 expression of the
    bf16 values (``data/augment.py::sample_mix`` draws the rows).  Bad rows raise
    ``ValueError`` here; the kernel does not check."""
    k = K(img_u8)
    pad = list(pad) if pad else []
    if extents is not None:
        extents = np.asarray(extents, dtype=np.int64).reshape(-1, 2)
        B, Hp, Wp = img_u8.shape[:3]
        if extents.shape[0] != B or (extents < 1).any() or (extents[:, 0] > Hp).any() \
                or (extents[:, 1] > Wp).any():
            raise ValueError("preprocess: extents %s do not fit the [%d, %d] slot pitch"
                             % (extents.tolist(), Hp, Wp))
    if boxes is not None:
        boxes = _check_boxes(boxes, extents, img_u8.shape, mode)
    if mix is not None or lam is not None:
        mix, lam = _check_mix(mix, lam, img_u8.shape[0], out_hw, mode)
    if img_u8.is_cuda:
        if mode == 1:  # PIL-exact bicubic (the eval transform)
            tc = _PIL_TABLES.get(img_u8.device)
            if tc is None:
                from ..data.pil_resize import TableCache
                tc = _PIL_TABLES[img_u8.device] = TableCache(img_u8.device)
            B, Hp, Wp = img_u8.shape[:3]
            ext = extents if extents is not None else np.tile([[Hp, Wp]], (B, 1))
            e, sel, hb, hk, kh, vb, vk, kv = tc.tables(ext, tuple(out_hw), (Hp, Wp))
            return k.preprocess_pil(img_u8, e if extents is not None else _empty_i32(img_u8),
                                    sel, hb, hk, kh, vb, vk, kv, out_hw[0], out_hw[1],
                                    list(mean), list(std), cpad, pad)
        ext = None
        if extents is not None:
            ext = torch.from_numpy(extents.astype(np.int32)).to(img_u8.device, non_blocking=True)
        if mix is not None:
            if boxes is None:  # the mixed kernel takes boxes: the full extents
                B, Hp, Wp = img_u8.shape[:3]
                boxes = np.zeros((B, 5), np.int32)
                boxes[:, 2:4] = extents if extents is not None else (Hp, Wp)
            dev = img_u8.device
            return k.preprocess(img_u8, out_hw[0], out_hw[1], list(mean), list(std), mode, cpad,
                                pad, ext, box=torch.from_numpy(boxes).to(dev, non_blocking=True),
                                mix=torch.from_numpy(mix).to(dev, non_blocking=True),
                                lam=torch.from_numpy(lam).to(dev, non_blocking=True))
        if boxes is not None:
            box = torch.from_numpy(boxes).to(img_u8.device, non_blocking=True)
            return k.preprocess(img_u8, out_hw[0], out_hw[1], list(mean), list(std), mode, cpad,
                                pad, ext, box=box)
        return k.preprocess(img_u8, out_hw[0], out_hw[1], list(mean), list(std), mode, cpad, pad,
                            ext)
    if mix is not None:
        return k.preprocess(img_u8, out_hw[0], out_hw[1], list(mean), list(std), mode, cpad,
                            out_dtype, pad, extents, boxes, mix, lam)
    if boxes is not None:
        return k.preprocess(img_u8, out_hw[0], out_hw[1], list(mean), list(std), mode, cpad,
                            out_dtype, pad, extents, boxes)
    return k.preprocess(img_u8, out_hw[0], out_hw[1], list(mean), list(std), mode, cpad,
                        out_dtype, pad, extents)


def _check_mix(mix, lam, B, out_hw, mode):
    """Mixing rows (partner, y0, x0, h, w) as a contiguous int32 [B, 5] array and the weights
    as float32 [B], or ``ValueError``: partners in [0, B), rectangles inside [0, OH] x [0, OW]
    with non-negative sides, weights finite and in [0, 1].  This host check is all that keeps
    the kernel's reads inside the batch."""
    if mode != 0:
        raise ValueError("preprocess: mixing needs mode 0 (the bilinear train transform)")
    if mix is None or lam is None:
        raise ValueError("preprocess: mix and lam go together")
    B, (OH, OW) = int(B), (int(v) for v in out_hw)
    mx, lm = np.asarray(mix), np.asarray(lam)
    if mx.dtype.kind not in "iu" or mx.shape != (B, 5):
        raise ValueError("preprocess: mix must be an integer [%d, 5] array, got %s %s"
                         % (B, mx.dtype, mx.shape))
    if lm.dtype.kind != "f" or lm.shape != (B,):
        raise ValueError("preprocess: lam must be a float [%d] array, got %s %s"
                         % (B, lm.dtype, lm.shape))
    mx = mx.astype(np.int64)
    p, y0, x0, h, w = (mx[:, i] for i in range(5))
    bad = (p < 0) | (p >= B) | (h < 0) | (w < 0) | (y0 < 0) | (x0 < 0) | (y0 + h > OH) \
        | (x0 + w > OW)
    if bad.any():
        b = int(np.argmax(bad))
        raise ValueError("preprocess: mix row %s of image %d: partner outside [0, %d) or "
                         "rectangle outside the (%d, %d) output (rows are partner, y0, x0, h, w)"
                         % (mx[b].tolist(), b, B, OH, OW))
    if not (np.isfinite(lm).all() and (lm >= 0.0).all() and (lm <= 1.0).all()):
        raise ValueError("preprocess: lam must be finite and in [0, 1]")
    return np.ascontiguousarray(mx.astype(np.int32)), np.ascontiguousarray(lm.astype(np.float32))


def _check_boxes(boxes, extents, shape, mode) -> np.ndarray:
    """Crop boxes (y0, x0, h, w, flip) as a contiguous int32 [B, 5] array, or ``ValueError``:
    every box must lie inside its image's extent (the slot when ``extents`` is None).  This
    host check is all that keeps the kernel's reads inside the slot."""
    if mode != 0:
        raise ValueError("preprocess: boxes need mode 0 (the bilinear train transform)")
    B, Hp, Wp = (int(v) for v in shape[:3])
    bx = np.asarray(boxes)
    if bx.dtype.kind not in "iu" or bx.ndim != 2 or bx.shape != (B, 5):
        raise ValueError("preprocess: boxes must be an integer [%d, 5] array, got %s %s"
                         % (B, bx.dtype, bx.shape))
    bx = bx.astype(np.int64)
    eh = extents[:, 0] if extents is not None else np.full(B, Hp, np.int64)
    ew = extents[:, 1] if extents is not None else np.full(B, Wp, np.int64)
    y0, x0, h, w, flip = (bx[:, i] for i in range(5))
    bad = (h < 1) | (w < 1) | (y0 < 0) | (x0 < 0) | (y0 + h > eh) | (x0 + w > ew) \
        | ((flip != 0) & (flip != 1))
    if bad.any():
        b = int(np.argmax(bad))
        raise ValueError("preprocess: box %s of image %d does not fit its extent (%d, %d) "
                         "(rows are y0, x0, h, w, flip)" % (bx[b].tolist(), b, eh[b], ew[b]))
    return np.ascontiguousarray(bx.astype(np.int32))


_PIL_TABLES = {}


def _empty_i32(t: torch.Tensor) -> torch.Tensor:
    key = (t.device, torch.int32)
    e = _EMPTY.get(key)
    if e is None:
        e = _EMPTY[key] = torch.empty(0, device=t.device, dtype=torch.int32)
    return e
