"""Plain-PyTorch implementation of the native kernel API (NHWC layout).

Two roles:
1. CPU execution path.  The reference framework is CPU-only (``main.py:50-51``), and
   BASELINE.json config 1 is a single-process CPU plumbing run, so CPU tensors run here.
2. Test oracle for every HIP kernel: the GPU tests call the same function here on the
   same inputs (computed in fp32) and compare.

It is NEVER used as a runtime fallback for GPU tensors (see ``ops/_ext.py``).

Every function mirrors a function of ``mpi_pytorch_amd._C`` with the same signature and
output dtypes: activations keep the input dtype (bf16 on GPU, fp32 on CPU), statistics
and gradient sinks are fp32.  Layouts: activations NHWC ``[N,H,W,C]``; conv weights
``[K,R,S,C]`` ("KRSC"); linear weights ``[out,in]``.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

Tensor = torch.Tensor


def _f(x: Tensor) -> Tensor:
    return x.float()


def _nchw(x: Tensor) -> Tensor:
    return x.permute(0, 3, 1, 2)


def _nhwc(x: Tensor) -> Tensor:
    return x.permute(0, 2, 3, 1).contiguous()


def _opt(t: Optional[Tensor]) -> Optional[Tensor]:
    if t is None or t.numel() == 0:
        return None
    return t


# ----------------------------------------------------------------------------------- conv
def conv_out_hw(H, W, R, S, sh, sw, ph, pw):
    return (H + 2 * ph - R) // sh + 1, (W + 2 * pw - S) // sw + 1


def affine_act(x, aff, relu):
    """relu?(x * aff[0] + aff[1]) per channel, in x's dtype (aff: bn_stats_affine's [2, C])."""
    y = _f(x) * aff[0].float() + aff[1].float()
    if relu:
        y = torch.relu(y)
    return y.to(x.dtype)


def conv_fwd(x, w, bias, sh, sw, ph, pw, relu, stats, shift=None):
    y = F.conv2d(_nchw(_f(x)), _f(w).permute(0, 3, 1, 2), None if _opt(bias) is None else _f(bias),
                 (sh, sw), (ph, pw))
    y = _nhwc(y)
    if relu:
        y = torch.relu(y)
    y = y.to(x.dtype)
    st = _opt(stats)
    if st is not None:  # finalized (mean, biased var) of the output, like the native kernel
        yf = y.float().reshape(-1, y.shape[-1])
        st[0].copy_(yf.mean(0))
        st[1].copy_(yf.var(0, unbiased=False))
    return y


def conv_dgrad(dy, w, H, W, sh, sw, ph, pw, wt=None, accum=None):
    """wt: transposed weight copy (unused here); accum: add the result into this tensor
    (in place, one rounding of the fp32 sum) and return it."""
    N, P, Q, K = dy.shape
    Kw, R, S, C = w.shape
    gi = torch.ops.aten.convolution_backward(
        _nchw(_f(dy)).contiguous(), torch.empty(N, C, H, W, device=dy.device),
        _f(w).permute(0, 3, 1, 2).contiguous(), None, [sh, sw], [ph, pw], [1, 1], False,
        [0, 0], 1, [True, False, False])[0]
    if accum is not None:
        accum.copy_((_f(accum) + _nhwc(gi)).to(accum.dtype))
        return accum
    return _nhwc(gi).to(dy.dtype)


def conv_dgrad_res(dy, w, wt, H, W, ph, pw, res, rmask):
    """Stride-1 dgrad + the residual gradient res * (y > 0) (y's ReLU bit mask), summed in
    fp32 and rounded once."""
    d = _f(conv_dgrad(dy, w, H, W, 1, 1, ph, pw))
    g = _f(res) * bitmask_unpack(rmask, res.shape)
    return (d + g).to(dy.dtype)


def conv_dgrad_pair(dy, w, wt, H, W, sh, sw, ph, pw, dy2, w2, wt2, ph2, pw2, accum=None):
    """dx of two convs reading the same input with the same stride (3x3/s2 conv1 + its
    1x1/s2 shortcut), summed in fp32 and rounded once; None if the grids differ."""
    if sh == 1 and sw == 1:
        return None
    P2 = (H + 2 * ph2 - w2.shape[1]) // sh + 1
    Q2 = (W + 2 * pw2 - w2.shape[2]) // sw + 1
    if (P2, Q2) != tuple(dy.shape[1:3]):
        return None

    def gi(d, ww, p_h, p_w):
        N = d.shape[0]
        C = ww.shape[3]
        return torch.ops.aten.convolution_backward(
            _nchw(_f(d)).contiguous(), torch.empty(N, C, H, W, device=d.device),
            _f(ww).permute(0, 3, 1, 2).contiguous(), None, [sh, sw], [p_h, p_w], [1, 1],
            False, [0, 0], 1, [True, False, False])[0]

    tot = _nhwc(gi(dy, w, ph, pw) + gi(dy2, w2, ph2, pw2))
    if accum is not None:
        accum.copy_((_f(accum) + tot).to(accum.dtype))
        return accum
    return tot.to(dy.dtype)


def conv_wgrad(dy, x, dw, sh, sw, ph, pw, overwrite=False):
    K, R, S, C = dw.shape
    gw = torch.ops.aten.convolution_backward(
        _nchw(_f(dy)).contiguous(), _nchw(_f(x)).contiguous(),
        torch.empty(K, C, R, S, device=dy.device), None, [sh, sw], [ph, pw], [1, 1], False,
        [0, 0], 1, [False, True, False])[1]
    if overwrite:
        dw.copy_(gw.permute(0, 2, 3, 1))
    else:
        dw.add_(gw.permute(0, 2, 3, 1))


def act_bwd(dy, y, dbias):
    """g = dy * (y > 0) if y given else dy; dbias += sum_rows(g)."""
    g = dy if _opt(y) is None else (_f(dy) * (_f(y) > 0)).to(dy.dtype)
    db = _opt(dbias)
    if db is not None:
        db.add_(_f(g).reshape(-1, g.shape[-1]).sum(0))
    return g


# ------------------------------------------------------------------------------------ BN
def relu_bitmask(y):
    """uint8 [numel / 8]: bit j of byte i = (element 8 i + j of y, flattened) > 0."""
    b = (y.reshape(-1, 8) > 0).to(torch.int32)
    w = torch.tensor([1 << j for j in range(8)], dtype=torch.int32, device=y.device)
    return (b * w).sum(1).to(torch.uint8)


def bitmask_unpack(m, shape):
    """Inverse of relu_bitmask: bool tensor of ``shape``."""
    bits = torch.arange(8, device=m.device, dtype=torch.int32)
    return ((m.to(torch.int32).unsqueeze(1) >> bits) & 1).bool().reshape(shape)


def bn_stats_affine(x, stats, gamma, beta, rmean, rvar, momentum, eps, counter=None):
    """Statistics half of a train-mode BN whose apply runs in its consumer: (mean, rstd,
    [2, C] affine = [gamma rstd | beta - mean gamma rstd]); updates the running stats."""
    C = x.shape[-1]
    xf = _f(x).reshape(-1, C)
    M = xf.shape[0]
    mean = xf.mean(0)
    var = xf.var(0, unbiased=False)
    rstd = torch.rsqrt(var + eps)
    sc = gamma.float() * rstd
    with torch.no_grad():
        unbiased = var * (M / max(M - 1, 1))
        rmean.mul_(1 - momentum).add_(mean, alpha=momentum)
        rvar.mul_(1 - momentum).add_(unbiased, alpha=momentum)
        if _opt(counter) is not None:
            counter.add_(1)
    return mean, rstd, torch.stack([sc, beta.float() - mean * sc])


def bn_fwd_train(x, stats, gamma, beta, rmean, rvar, momentum, eps, residual, relu,
                 counter=None, mask=None, channels=0, res_affine=None, out=None):
    # the oracle always uses exact two-pass statistics (``stats`` from a fused producer
    # epilogue is accepted for API parity but not needed); channels > 0: BN of the first
    # ``channels`` channels of a wider buffer
    if channels:
        x = x[..., :channels]
    C = x.shape[-1]
    xf = _f(x).reshape(-1, C)
    M = xf.shape[0]
    mean = xf.mean(0)
    var = xf.var(0, unbiased=False)
    rstd = torch.rsqrt(var + eps)
    y = (xf - mean) * (rstd * gamma) + beta
    if _opt(residual) is not None:
        r = _f(residual).reshape(-1, C)
        if _opt(res_affine) is not None:  # the residual's deferred BN
            r = r * res_affine[0] + res_affine[1]
        y = y + r
    if relu:
        y = torch.relu(y)
    with torch.no_grad():
        unbiased = var * (M / max(M - 1, 1))
        rmean.mul_(1 - momentum).add_(mean, alpha=momentum)
        rvar.mul_(1 - momentum).add_(unbiased, alpha=momentum)
        if _opt(counter) is not None:
            counter.add_(1)
    y = y.reshape(x.shape).to(x.dtype)
    if _opt(mask) is not None:
        mask.copy_(relu_bitmask(y))
    if _opt(out) is not None:  # a channel window of a wider buffer
        # (through .data, like a native kernel's store: no autograd version bump of the
        # buffer the other branches' outputs are views of)
        out.data.copy_(y)
        y = out
    return y, mean.contiguous(), rstd.contiguous()


def bn_stats(x, shift=None):
    xf = _f(x).reshape(-1, x.shape[-1])
    return torch.stack([xf.mean(0), xf.var(0, unbiased=False)])


def bn_fwd_eval(x, gamma, beta, rmean, rvar, eps, residual, relu, channels=0):
    if channels:
        x = x[..., :channels]
    C = x.shape[-1]
    xf = _f(x).reshape(-1, C)
    rstd = torch.rsqrt(rvar + eps)
    y = (xf - rmean) * (rstd * gamma) + beta
    if _opt(residual) is not None:
        y = y + _f(residual).reshape(-1, C)
    if relu:
        y = torch.relu(y)
    return y.reshape(x.shape).to(x.dtype)


def bn_bwd(dy, x, y, mean, rstd, gamma, dgamma, dbeta, want_dx, want_g=True, zmask_beta=None,
           ymask=None, gacc=None, dx_out=None):
    """Returns (dx, g) where g = dy masked by ReLU (the residual-branch gradient).  The mask
    comes from ``ymask`` (bn_fwd_train's bit mask) if given, else from ``y``, else - with
    ``zmask_beta`` - is recomputed from x for y = relu(bn(x)).  x may be wider than dy (a
    channel prefix); ``gacc`` (fp32): dx is added into its first C channels instead."""
    C = dy.shape[-1]
    x = x[..., :C]
    g = _f(dy).reshape(-1, C)
    if _opt(ymask) is not None:
        g = g * bitmask_unpack(ymask, g.shape)
    elif _opt(y) is not None:
        g = g * (_f(y).reshape(-1, C) > 0)
    elif _opt(zmask_beta) is not None:
        sc = gamma * rstd
        t = (_f(x).reshape(-1, C) * sc + (zmask_beta - mean * sc)).to(torch.bfloat16).float()
        g = g * (t > 0)
    M = g.shape[0]
    xhat = (_f(x).reshape(-1, C) - mean) * rstd
    sg = g.sum(0)
    sgx = (g * xhat).sum(0)
    if _opt(dgamma) is not None:
        dgamma.add_(sgx)
    if _opt(dbeta) is not None:
        dbeta.add_(sg)
    dx = None
    if gacc is not None:
        d = (gamma * rstd) * (g - sg / M - xhat * (sgx / M))
        gacc[..., :C] += d.reshape(dy.shape)
    elif want_dx:
        dx = (gamma * rstd) * (g - sg / M - xhat * (sgx / M))
        dx = dx.reshape(dy.shape).to(dy.dtype)
        if dx_out is not None:
            dx_out.copy_(dx)
            dx = dx_out
    return dx, g.reshape(dy.shape).to(dy.dtype)


def bn_bwd_pair(dy, x, ymask, mean, rstd, gamma, dgamma, dbeta, x2, mean2, rstd2, gamma2,
                dgamma2, dbeta2):
    """Backward of relu(bn(x) + bn2(x2)), both BNs train-mode: [dx, dx2] from the shared
    g = dy * mask (kept in fp32, as the fused kernel does)."""
    C = dy.shape[-1]
    g = _f(dy).reshape(-1, C) * bitmask_unpack(ymask, (dy.numel() // C, C))
    M = g.shape[0]
    sg = g.sum(0)
    out = []
    for xx, mu, rs, ga, dga, dbe in ((x, mean, rstd, gamma, dgamma, dbeta),
                                     (x2, mean2, rstd2, gamma2, dgamma2, dbeta2)):
        xhat = (_f(xx).reshape(-1, C) - mu) * rs
        sgx = (g * xhat).sum(0)
        if _opt(dga) is not None:
            dga.add_(sgx)
        if _opt(dbe) is not None:
            dbe.add_(sg)
        d = (ga * rs) * (g - sg / M - xhat * (sgx / M))
        out.append(d.reshape(dy.shape).to(dy.dtype))
    return out


def bn_bwd_apply(dy, x, y, mean, rstd, gamma, dgamma, dbeta, sums, want_dx, want_g=True):
    """bn_bwd's apply pass with precomputed sums = [sum g | sum g*xhat]."""
    C = x.shape[-1]
    g = _f(dy).reshape(-1, C)
    if _opt(y) is not None:
        g = g * (_f(y).reshape(-1, C) > 0)
    M = g.shape[0]
    xhat = (_f(x).reshape(-1, C) - mean) * rstd
    sg, sgx = sums[:C], sums[C:]
    if _opt(dgamma) is not None:
        dgamma.add_(sgx)
    if _opt(dbeta) is not None:
        dbeta.add_(sg)
    dx = None
    if want_dx:
        dx = ((gamma * rstd) * (g - sg / M - xhat * (sgx / M))).reshape(x.shape).to(dy.dtype)
    return dx, g.reshape(x.shape).to(dy.dtype)


def conv_bnred_ok(K, C):
    return True


def conv_dgrad_bnred(dy, w, H, W, sh, sw, ph, pw, wt, z, y, mean, rstd, gamma=None, beta=None):
    """dgrad fused with the backward reduction of the ReLU(BN) that produced the conv
    input: returns (g = dx * (y > 0), [sum g | sum g * xhat]).  Without y, the mask is
    recomputed from z with the forward's affine (gamma, beta) - the halo kernel's form
    (y is the same mask when it is the forward's output)."""
    dx = conv_dgrad(dy, w, H, W, sh, sw, ph, pw)
    C = dx.shape[-1]
    g = _f(dx).reshape(-1, C)
    if _opt(y) is not None:
        g = g * (_f(y).reshape(-1, C) > 0)
    elif gamma is not None and beta is not None:
        sc = gamma.float() * rstd
        sh_ = beta.float() - mean * sc
        live = (_f(z).reshape(-1, C) * sc + sh_).to(torch.bfloat16).float() > 0
        g = g * live
    xhat = (_f(z).reshape(-1, C) - mean) * rstd
    sums = torch.cat([g.sum(0), (g * xhat).sum(0)])
    return g.reshape(dx.shape).to(dx.dtype), sums


def conv_dgrad_bnred_gacc(dz, w, wt, zbuf, mean, rstd, gamma, beta, G):
    """1x1 / stride-1 dgrad fused with the backward of the ReLU(BN) that produced its input
    (a DenseNet norm1 over the block buffer's first Ci channels): G[..., :Ci] += gamma*rstd *
    g with g the masked dgrad (no dy tensor); returns [sum g | sum g * xhat].  The rest of
    the BN backward is deferred to bn_defer_step."""
    Ci = w.shape[-1]
    N, H, W_ = dz.shape[:3]
    dx = conv_dgrad(dz, w, H, W_, 1, 1, 0, 0)
    g = _f(dx).to(dz.dtype).float().reshape(-1, Ci)  # the kernel rounds dy to bf16 first
    z = _f(zbuf[..., :Ci]).reshape(-1, Ci)
    sc = gamma.float()[:Ci] * rstd[:Ci]
    sh_ = beta.float()[:Ci] - mean[:Ci] * sc
    g = g * ((z * sc + sh_).to(torch.bfloat16).float() > 0)
    xhat = (z - mean[:Ci]) * rstd[:Ci]
    Gv = G[..., :Ci]
    Gv.copy_((Gv.float() + (sc * g).reshape(Gv.shape)).to(G.dtype))
    return torch.cat([g.sum(0), (g * xhat).sum(0)])


def bn_defer_step(sums, gamma, mean, rstd, s0, k12, dgamma, dbeta, G, x, out=None):
    """Fold a dense layer's norm1 sums into the block's deferred corrections k12 [2, Ctot]
    (channels < s0) and the (gamma, beta) gradients, and apply the final correction
    G += K1 + K2 * xhat to the channels [s0, Ci)."""
    Ci = sums.numel() // 2
    M = x.numel() // x.shape[-1]
    sg, sgx = sums[:Ci], sums[Ci:]
    if _opt(dgamma) is not None:
        dgamma.add_(sgx)
    if _opt(dbeta) is not None:
        dbeta.add_(sg)
    a = gamma.float()[:Ci] * rstd[:Ci]
    t1, t2 = -a * sg / M, -a * sgx / M
    k1 = k12[0, s0:Ci] + t1[s0:]
    k2 = k12[1, s0:Ci] + t2[s0:]
    k12[0, :s0] += t1[:s0]
    k12[1, :s0] += t2[:s0]
    xs = _f(x[..., s0:Ci])
    xhat = (xs - mean[s0:Ci]) * rstd[s0:Ci]
    Gv = G[..., s0:Ci]
    fin = (Gv.float() + k1 + k2 * xhat).to(G.dtype)
    if out is not None and out.numel():  # the consumer's copy only (G's is never read again)
        out.copy_(fin.to(out.dtype))
    else:
        Gv.copy_(fin)


def conv_fwd_into(x, w, bias, sh, sw, ph, pw, relu, stats, shift, out):
    """conv_fwd writing into ``out`` (a channel window of a wider buffer); ``stats`` may be
    a [2, K] window of a wider table."""
    st = _opt(stats)
    tmp = torch.empty(2, w.shape[0], dtype=torch.float32) if st is not None else stats
    y = conv_fwd(x, w, bias, sh, sw, ph, pw, relu, tmp, shift)
    out.copy_(y)
    if st is not None:
        st.copy_(tmp)


# ---------------------------------------------------------------------------------- pool
def _pool_out(H, k, s, p, ceil):
    if ceil:
        o = -(-(H + 2 * p - k) // s) + 1
        if (o - 1) * s >= H + p:
            o -= 1
    else:
        o = (H + 2 * p - k) // s + 1
    return o


def maxpool_fwd(x, kh, kw, sh, sw, ph, pw, ceil):
    y, idx = F.max_pool2d(_nchw(_f(x)), (kh, kw), (sh, sw), (ph, pw), ceil_mode=ceil,
                          return_indices=True)
    return _nhwc(y).to(x.dtype), _nhwc(idx.to(torch.int32))


def maxpool_bwd(dy, idx, H, W, kh, kw, sh, sw, ph, pw, ceil):
    N, P, Q, C = dy.shape
    out = torch.zeros(N, C, H * W, device=dy.device, dtype=torch.float32)
    out.scatter_add_(2, _nchw(idx).reshape(N, C, -1).long(), _nchw(_f(dy)).reshape(N, C, -1))
    return _nhwc(out.reshape(N, C, H, W)).to(dy.dtype)


def maxpool_bwd_relu(dy, idx, y, H, W, kh, kw, sh, sw, ph, pw):
    """Max-pool backward of a ReLU output handed over by its producer: the gradient routes
    only where the pooled value is > 0; returns (dx, per-channel sum of the routed
    gradient), or None when the fused kernel would not apply (not a 2x2/s2/p0 pool)."""
    if not (kh == kw == sh == sw == 2 and ph == pw == 0 and H % 2 == 0 and W % 2 == 0):
        return None
    g = _f(dy) * (_f(y) > 0)
    dx = maxpool_bwd(g, idx, H, W, kh, kw, sh, sw, ph, pw, False).to(dy.dtype)
    return dx, g.reshape(-1, g.shape[-1]).sum(0)


def bn_relu_maxpool_fwd(z, stats, gamma, beta, rmean, rvar, momentum, eps, kh, kw, sh, sw, ph,
                        pw, ceil, counter=None, zsel_out=None):
    y, mean, rstd = bn_fwd_train(z, stats, gamma, beta, rmean, rvar, momentum, eps, None, True,
                                 counter)
    p, idx = maxpool_fwd(y, kh, kw, sh, sw, ph, pw, ceil)
    if zsel_out is not None:  # raw z at each window's argmax
        N, H, W, C = z.shape
        flat = _nchw(idx).reshape(N, C, -1).long()  # ATen's flat h * W + w argmax
        zs = _nchw(z).reshape(N, C, -1).gather(2, flat)
        zsel_out.copy_(_nhwc(zs.reshape(N, C, p.shape[1], p.shape[2])))
    return p, idx, mean, rstd


def maxpool_bn_bwd(dp, idx, z, mean, rstd, gamma, beta, dgamma, dbeta, kh, kw, sh, sw, ph, pw,
                   zsel=None):
    N, H, W, C = z.shape
    g = maxpool_bwd(dp, idx, H, W, kh, kw, sh, sw, ph, pw, False)
    # ReLU mask recomputed from z: bn(z) > 0
    y = (_f(z) - mean) * (rstd * gamma) + beta
    dz, _ = bn_bwd(g, z, y, mean, rstd, gamma, dgamma, dbeta, True, False)
    return dz


def maxpool_bn_bwd_sums(dp, zsel, mean, rstd, gamma, beta, dgamma, dbeta):
    """Pooled-only half of the fused stem backward: [sum g | sum g xhat] with g the pooled
    gradient masked by bn(zsel) > 0 (zsel = raw z at each argmax); adds dgamma / dbeta."""
    C = dp.shape[-1]
    z = _f(zsel).reshape(-1, C)
    g = _f(dp).reshape(-1, C) * ((z - mean) * (rstd * gamma) + beta > 0)
    sg, sgx = g.sum(0), (g * ((z - mean) * rstd)).sum(0)
    if _opt(dgamma) is not None:
        dgamma.add_(sgx)
    if _opt(dbeta) is not None:
        dbeta.add_(sg)
    return torch.cat([sg, sgx])


def stem_pool_wgrad_ok(dp, idx, z, x, dw, sh, sw, ph, pw):
    return True


def stem_pool_wgrad(dp, idx, z, mean, rstd, gamma, beta, sums, x, dw, sh, sw, ph, pw,
                    overwrite=False):
    """Weight gradient of conv -> BN -> ReLU -> 3x3/s2/p1 max-pool from the pooled gradient:
    dz = a g + b + cco z (the BN backward with the pooled ``sums``), rounded to the
    activation dtype as the two-pass form stores it, then the conv weight gradient."""
    N, H, W, C = z.shape
    g = _f(maxpool_bwd(dp, idx, H, W, 3, 3, 2, 2, 1, 1, False)).reshape(-1, C)
    zf = _f(z).reshape(-1, C)
    g = g * ((zf - mean) * (rstd * gamma) + beta > 0)
    M = g.shape[0]
    a = gamma * rstd
    cco = -a * rstd * sums[C:] / M
    b = -a * sums[:C] / M - cco * mean
    dz = (a * g + b + cco * zf).reshape(z.shape).to(z.dtype)
    conv_wgrad(dz, x, dw, sh, sw, ph, pw, overwrite)


def avgpool_fwd(x, kh, kw, sh, sw, ph, pw, ceil, count_include_pad):
    y = F.avg_pool2d(_nchw(_f(x)), (kh, kw), (sh, sw), (ph, pw), ceil_mode=ceil,
                     count_include_pad=count_include_pad)
    return _nhwc(y).to(x.dtype)


def avgpool_bwd(dy, H, W, kh, kw, sh, sw, ph, pw, ceil, count_include_pad, dx_out=None):
    N, P, Q, C = dy.shape
    xin = torch.zeros(N, C, H, W, device=dy.device, requires_grad=True)
    with torch.enable_grad():
        y = F.avg_pool2d(xin, (kh, kw), (sh, sw), (ph, pw), ceil_mode=ceil,
                         count_include_pad=count_include_pad)
        (gx,) = torch.autograd.grad(y, xin, _nchw(_f(dy)))
    gx = _nhwc(gx).to(dy.dtype)
    if dx_out is not None:
        dx_out.copy_(gx)
        return dx_out
    return gx


def bn_relu_avgpool2_fwd(z, aff):
    """avg_pool2d(relu(z * aff[0] + aff[1]), 2, 2) over NHWC z."""
    y = torch.relu(_f(z) * aff[0] + aff[1])
    return _nhwc(F.avg_pool2d(_nchw(y), 2, 2)).to(z.dtype)


def adaptive_avgpool_fwd(x, oh, ow):
    return _nhwc(F.adaptive_avg_pool2d(_nchw(_f(x)), (oh, ow))).to(x.dtype)


def adaptive_avgpool_bwd(dy, H, W):
    N, P, Q, C = dy.shape
    xin = torch.zeros(N, C, H, W, device=dy.device, requires_grad=True)
    with torch.enable_grad():
        y = F.adaptive_avg_pool2d(xin, (P, Q))
        (gx,) = torch.autograd.grad(y, xin, _nchw(_f(dy)))
    return _nhwc(gx).to(dy.dtype)


# ------------------------------------------------------------------------------- linear
def linear_fwd(x, w, bias, relu):
    y = _f(x) @ _f(w).t()
    if _opt(bias) is not None:
        y = y + _f(bias)
    if relu:
        y = torch.relu(y)
    return y.to(x.dtype)


def linear_dgrad(dy, w, wt=None):
    return (_f(dy) @ _f(w)).to(dy.dtype)


def linear_wgrad(dy, x, dw, overwrite=False):
    if overwrite:
        dw.copy_(_f(dy).t() @ _f(x))
    else:
        dw.add_(_f(dy).t() @ _f(x))


# --------------------------------------------------------------------------- loss / acc
def _adjusted(logits, bias):
    """fp32 logits, plus the logit adjustment's per-class term ``bias[:NC]`` when given."""
    lf = _f(logits)
    return lf if bias is None else lf + _f(bias)[:lf.shape[1]]


def ce_fwd(logits, labels, smoothing=0.0, labels2=None, lam=None, bias=None):
    """``smoothing``: torch's ``label_smoothing`` - the target is (1 - eps) * onehot + eps / NC.
    ``labels2`` / ``lam`` [B] (Mixup / CutMix): onehot is lam * onehot(labels) + (1 - lam) *
    onehot(labels2).  ``bias`` fp32 [>= NC] (logit adjustment): the loss and the returned lse
    are those of ``float(logits) + bias[:NC]``."""
    lf = _adjusted(logits, bias)
    lse = torch.logsumexp(lf, dim=1)
    picked = lf.gather(1, labels.view(-1, 1).long()).squeeze(1)
    if labels2 is not None:
        lam = _f(lam)
        picked = lam * picked + (1.0 - lam) * lf.gather(1, labels2.view(-1, 1).long()).squeeze(1)
    if smoothing:
        rows = lse - (1.0 - smoothing) * picked - (smoothing / lf.shape[1]) * lf.sum(1)
    else:
        rows = lse - picked
    return rows.mean().reshape(1), lse


def ce_bwd(logits, labels, lse, grad_out, weight=1.0, smoothing=0.0, labels2=None, lam=None,
           bias=None):
    B, NC = logits.shape
    p = torch.exp(_adjusted(logits, bias) - lse[:, None])
    if smoothing:
        p -= smoothing / NC
    rows = torch.arange(B, device=logits.device)
    if labels2 is not None:  # the two weights are added first: right, and the same under a
        lam = _f(lam)        # swap of the labels, when both name one column
        w = torch.zeros_like(p)
        w[rows, labels.long()] += lam
        w[rows, labels2.long()] += 1.0 - lam
        p -= (1.0 - smoothing) * w
    else:
        p[rows, labels.long()] -= 1.0 - smoothing
    return (p * (_f(grad_out).reshape(()) * weight / B)).to(logits.dtype)


def ce_fwd_weighted(logits, labels, out, acc, weight, accumulate, smoothing=0.0, labels2=None,
                    lam=None, bias=None):
    loss, lse = ce_fwd(logits, labels, smoothing, labels2, lam, bias)
    v = loss.reshape(1) * weight
    if accumulate:
        out[:1] += v
    else:
        out[:1] = v
    if acc is not None and acc.numel() > 0:
        acc[:1] += v
    return lse


def zero_f32(t):
    t.zero_()


def step_inc(step):
    step.add_(1.0)


def argmax_correct(logits, labels, count):
    pred = _f(logits).argmax(1)
    count.add_((pred == labels.long()).sum().to(count.dtype))


def argmax_stats(logits, labels, count, stats):
    """``argmax_correct``'s count, and per-class counters ``stats`` int64 [3, NC] (support,
    predicted, true positives).  The prediction is the first index of the row's largest
    non-NaN logit; a row without one (all NaN or -inf) predicts nothing.  For a row with a
    label in [0, NC): stats[0][label] += 1, stats[1][pred] += 1 (when there is a prediction),
    stats[2][label] += 1 (when pred == label).  Other rows touch no counter; count gains the
    rows with pred == label."""
    lf = _f(logits)
    NC = lf.shape[1]
    lab = labels.long()
    v = torch.where(torch.isnan(lf), torch.full_like(lf, float("-inf")), lf)
    best = v.max(1, keepdim=True).values
    idx = torch.arange(NC, device=lf.device).view(1, -1)
    first = torch.where(v == best, idx, NC).min(1).values
    pred = torch.where(best.squeeze(1) > float("-inf"), first, torch.full_like(first, 0x7fffffff))
    count.add_((pred == lab).sum().to(count.dtype))
    valid = (lab >= 0) & (lab < NC)
    one = lambda sel: torch.bincount(sel, minlength=NC).to(stats.dtype)
    stats[0] += one(lab[valid])
    stats[1] += one(pred[valid & (pred < NC)])
    stats[2] += one(lab[valid & (pred == lab)])


def topk_correct(logits, labels, k, count):
    """count += #{rows whose label is among the k largest logits}.  No sort: the label's
    rank is the number of columns that beat it, a tie going to the lower index (argmax's
    rule, so k = 1 is ``argmax_correct``).  Rows whose label is outside [0, NC) or whose
    label logit is NaN are not counted; NaNs elsewhere compare false."""
    if k < 1:
        raise ValueError("topk_correct: k must be >= 1, got %r" % (k,))
    lf = _f(logits)
    NC = lf.shape[1]
    lab = labels.long()
    valid = (lab >= 0) & (lab < NC)
    safe = lab.clamp(0, NC - 1).view(-1, 1)
    xl = lf.gather(1, safe)
    idx = torch.arange(NC, device=lf.device).view(1, -1)
    rank = ((lf > xl) | ((lf == xl) & (idx < safe))).sum(1)
    ok = valid & ~torch.isnan(xl.squeeze(1)) & (rank < k)
    count.add_(ok.sum().to(count.dtype))


def topk_predict(logits, k, idx, prob):
    """The k best classes of every row and their softmax probabilities, written into ``idx``
    int32 [B, k] and ``prob`` float32 [B, k].  Candidates are the columns whose logit is
    neither NaN nor -inf; c outranks d when x[c] > x[d], or x[c] == x[d] and c < d
    (``topk_correct``'s order), and idx[r, j] is the candidate that exactly j candidates
    outrank.  prob[r, j] = exp(x[idx] - logsumexp(x[r])); slots past the last candidate get
    idx = -1 and prob = 0.  (With a NaN or +inf in the row its probabilities are unspecified.)"""
    if not 1 <= k <= 16:
        raise ValueError("topk_predict: k must be in [1, 16], got %r" % (k,))
    B, NC = logits.shape
    for t, dt, what in ((idx, torch.int32, "idx"), (prob, torch.float32, "prob")):
        if (t.dtype != dt or tuple(t.shape) != (B, k) or not t.is_contiguous()
                or t.device != logits.device):
            raise ValueError("topk_predict: %s must be a contiguous %s [B, k] tensor on the "
                             "logits' device" % (what, dt))
    lf = _f(logits)
    ninf = torch.full_like(lf, float("-inf"))
    v, order = torch.sort(torch.where(torch.isnan(lf), ninf, lf), dim=1, descending=True,
                          stable=True)  # stable: equal logits keep their column order
    n = min(k, NC)
    v, order = v[:, :n], order[:, :n]
    some = v > float("-inf")
    # row by row: a batched reduction may split a long row differently from batch to batch,
    # and a row's outputs depend on that row alone
    lse = torch.stack([torch.logsumexp(row, 0) for row in lf]) if B else lf.new_zeros(0)
    p = torch.exp(v - lse[:, None]).clamp(max=1.0)
    idx.fill_(-1)
    prob.zero_()
    idx[:, :n] = torch.where(some, order, torch.full_like(order, -1)).to(torch.int32)
    prob[:, :n] = torch.where(some, p, torch.zeros_like(p))


# ----------------------------------------------------------------------------- optimizer
def adam_step(master, grad, m, v, shadow, step_t, lr, b1, b2, eps, wd, grad_scale):
    step = float(step_t.item()) + 1.0
    g = grad * grad_scale
    if wd != 0.0:
        g = g + wd * master
    m.mul_(b1).add_(g, alpha=1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    bc1 = 1 - b1 ** step
    bc2 = 1 - b2 ** step
    denom = (v.sqrt() / math.sqrt(bc2)).add_(eps)
    master.addcdiv_(m, denom, value=-lr / bc1)
    if _opt(shadow) is not None:
        shadow.copy_(master)


def sgd_step(master, grad, buf, shadow, step_t, lr, momentum, dampening, wd, nesterov, grad_scale):
    first = float(step_t.item()) == 0.0
    g = grad * grad_scale
    if wd != 0.0:
        g = g + wd * master
    if momentum != 0.0:
        if first:
            buf.copy_(g)
        else:
            buf.mul_(momentum).add_(g, alpha=1 - dampening)
        g = g + momentum * buf if nesterov else buf
    master.add_(g, alpha=-lr)
    if _opt(shadow) is not None:
        shadow.copy_(master)


# ---- per-step recipe (LR schedule + global-norm clipping); csrc/kernels/optim.hip
# hyper record slots (csrc/kernels/api.h HYPER_*)
HYPER_LR, HYPER_SCALE, HYPER_NORM, HYPER_COEF, HYPER_SKIP, HYPER_NONFINITE, HYPER_SUMSQ = range(7)
HYPER_N = 8
SCHEDULE_KINDS = ("constant", "cosine", "step")


def grad_sqnorm_grid_cap():
    return 1


def grad_sqnorm(grad, part):
    """Sum of squares of the gradient arena, accumulated in float64; one partial."""
    part[0] = float(grad.double().pow(2).sum())
    return 1


def grad_sqnorm_sum(part, nparts, out):
    out[0] = float(part[:nparts].double().sum())


def hyper_update(step_t, hyper, part, nparts, kind, base_lr, warmup, total, min_ratio, gamma,
                 decay_steps, max_norm, grad_scale):
    """fp32 mirror of hyper_kernel: k = step_t (the 0-based index of this update)."""
    f = np.float32
    k, base, W, T, r = f(float(step_t.item())), f(base_lr), f(warmup), f(total), f(min_ratio)
    lr = base
    if k < W:
        lr = base * (k + f(1)) / W
    elif kind == 1:
        if k < T:
            p = (k - W) / max(f(1), T - W)
            lr = base * (r + (f(1) - r) * f(0.5) * (f(1) + f(math.cos(math.pi * float(p)))))
        else:
            lr = base * r
    elif kind == 2:
        lr = base * f(float(gamma) ** math.floor(float(k / f(decay_steps))))
    gs = f(grad_scale)
    norm, coef, skip, bad = f(0), f(1), f(0), f(float(hyper[HYPER_NONFINITE]))
    sumsq = f(0)
    if nparts > 0:
        with np.errstate(over="ignore", invalid="ignore"):
            sumsq = f(float(part[:nparts].double().sum()))
            norm = gs * np.sqrt(sumsq)
        if not np.isfinite(sumsq):
            skip, coef, bad = f(1), f(0), bad + f(1)
        elif norm > f(max_norm):
            coef = min(f(1), f(max_norm) / (norm + f(1e-6)))
    hyper[HYPER_LR] = float(lr)
    hyper[HYPER_SCALE] = float(gs * coef)
    hyper[HYPER_NORM] = float(norm)
    hyper[HYPER_COEF] = float(coef)
    hyper[HYPER_SKIP] = float(skip)
    hyper[HYPER_NONFINITE] = float(bad)
    hyper[HYPER_SUMSQ] = float(sumsq)


def adam_step_dev(master, grad, m, v, shadow, step_t, hyper, b1, b2, eps, wd):
    if float(hyper[HYPER_SKIP]) != 0.0:
        return
    adam_step(master, grad, m, v, shadow, step_t, float(hyper[HYPER_LR]), b1, b2, eps, wd,
              float(hyper[HYPER_SCALE]))


def sgd_step_dev(master, grad, buf, shadow, step_t, hyper, momentum, dampening, wd, nesterov):
    if float(hyper[HYPER_SKIP]) != 0.0:
        return
    sgd_step(master, grad, buf, shadow, step_t, float(hyper[HYPER_LR]), momentum, dampening, wd,
             nesterov, float(hyper[HYPER_SCALE]))


# ---- weight EMA; csrc/kernels/optim.hip
EMA_SRC, EMA_OFF, EMA_LEN = range(3)
EMA_COLS = 3


def ema_weight(step_t, decay, warmup):
    """fp32 mirror of the kernels' ``w = 1 - d_t``, ``d_t = min(decay, (1 + t) / (10 + t))``
    with warm-up (``t = step_t``, the updates completed), else ``decay``."""
    f = np.float32
    d = f(decay)
    if warmup:
        t = f(float(step_t.item()))
        d = min(d, (f(1) + t) / (f(10) + t))
    return f(1) - d


def _ema_into(ema, p, w):
    diff = p - ema       # three separately rounded fp32 tensor ops, like ema_elem
    prod = diff * float(w)
    ema.add_(prod)


def ema_update(ema, p, step_t, decay, warmup):
    """ema += w * (p - ema) over a flat fp32 arena; bit for bit the kernel."""
    if not 0.0 <= decay < 1.0:
        raise ValueError("ema_update: decay must be in [0, 1), got %r" % (decay,))
    _ema_into(ema, p, ema_weight(step_t, decay, warmup))


def ema_update_multi(ema_buf, table, table_host, srcs, step_t, decay, warmup):
    """The same update for the small fp32 tensors ``srcs``: source ``i`` averages into
    ``ema_buf[off:off + len]`` of row ``i`` of ``table_host`` [nbuf][EMA_COLS] int64 =
    (source address, offset, length).  ``table`` is the kernel's device copy."""
    if not 0.0 <= decay < 1.0:
        raise ValueError("ema_update_multi: decay must be in [0, 1), got %r" % (decay,))
    rows = table_host.tolist()
    if len(rows) != len(srcs):
        raise ValueError("ema_update_multi: one table row per source")
    w = ema_weight(step_t, decay, warmup)
    for (_addr, off, ln), s in zip(rows, srcs):
        if ln != s.numel() or off < 0 or off + ln > ema_buf.numel():
            raise ValueError("ema_update_multi: a table row does not describe its source")
        _ema_into(ema_buf[off:off + ln], s.reshape(-1), w)


# ---- layer-wise optimizers on the segment plan (AdamW / LAMB / LARS); csrc/kernels/optim.hip
# seg [nseg][SEG_COLS] int64 rows (csrc/kernels/api.h SEG_*); the segments tile [0, n)
SEG_OFF, SEG_LEN, SEG_FIRST, SEG_NCHUNK, SEG_FLAGS = range(5)
SEG_COLS = 5
SEG_DECAY, SEG_ADAPT = 1, 2
TRUST_LAMB, TRUST_LARS = 0, 1


def seg_chunk():
    return 16384


def _seg_total(seg):
    rows = seg.tolist()
    off = 0
    for r in rows:  # (the twins expand per-segment values over a gap-free tiling)
        assert r[SEG_OFF] == off and r[SEG_LEN] > 0, "segments must tile [0, n)"
        off += r[SEG_LEN]
    return rows, off


def _per_element(seg, vals, like):
    """vals[s] repeated over segment s: one value per arena element."""
    return torch.repeat_interleave(torch.as_tensor(vals, dtype=like.dtype, device=like.device),
                                   seg[:, SEG_LEN].to(like.device))


def _chunk_sums(sq, rows, part):
    """part[c] = float64 sum of the per-element values ``sq`` over chunk c."""
    CH = seg_chunk()
    for off, ln, first, nch, _flags in rows:
        t = sq[off:off + ln]
        if ln % CH:
            t = torch.nn.functional.pad(t, (0, CH - ln % CH))
        part[first:first + nch] = t.view(-1, CH).sum(1).to(part.dtype)


def seg_sqnorm(x, seg, chunk_seg, hyper, scaled, part):
    """Per-chunk sum of squares of an arena-shaped buffer, accumulated in float64."""
    if float(hyper[HYPER_SKIP]) != 0.0:
        return
    rows, n = _seg_total(seg)
    xs = x[:n].double()
    if scaled:
        xs = xs * float(hyper[HYPER_SCALE])
    _chunk_sums(xs * xs, rows, part)


def _lamb_u(p, g, m, v, step_t, gs, b1, b2, eps, wd_e):
    """New moments and LAMB's update direction u = m^ / (sqrt(v^) + eps) + wd * p, in the
    dtype of the inputs (``wd_e``: per-element decay or None)."""
    step = float(step_t.item()) + 1.0
    gr = g * gs
    m2 = m.mul(b1).add_(gr, alpha=1 - b1)  # (adam_step's operations: the same moments)
    v2 = v.mul(b2).addcmul_(gr, gr, value=1 - b2)
    u = (m2 / (1 - b1 ** step)) / (v2.sqrt() / math.sqrt(1 - b2 ** step) + eps)
    if wd_e is not None:
        u = u + wd_e * p
    return m2, v2, u


def _decay_per_element(seg, rows, wd, like):
    if wd == 0.0:
        return None
    return _per_element(seg, [wd if r[SEG_FLAGS] & SEG_DECAY else 0.0 for r in rows], like)


def lamb_norms(master, grad, m, v, step_t, hyper, seg, chunk_seg, part_p, part_u, b1, b2, eps,
               wd):
    """LAMB stage 1: per-chunk sums of p^2 and of u^2 (float64 accumulation); reads only."""
    if float(hyper[HYPER_SKIP]) != 0.0:
        return
    rows, n = _seg_total(seg)
    p = master[:n]
    _m, _v, u = _lamb_u(p, grad[:n], m[:n], v[:n], step_t, float(hyper[HYPER_SCALE]), b1, b2,
                        eps, _decay_per_element(seg, rows, wd, p))
    _chunk_sums(p.double() ** 2, rows, part_p)
    _chunk_sums(u.double() ** 2, rows, part_u)


def trust_ratio(seg, chunk_seg, part_p, part_b, hyper, mode, trust_coef, wd, ratio, norms):
    if float(hyper[HYPER_SKIP]) != 0.0:
        return
    nv = norms.view(-1)
    for s, (_off, _ln, first, nch, flags) in enumerate(seg.tolist()):
        pn = math.sqrt(float(part_p[first:first + nch].double().sum()))
        bn = math.sqrt(float(part_b[first:first + nch].double().sum()))
        r = 1.0
        if flags & SEG_ADAPT and pn > 0.0 and bn > 0.0:
            if mode == TRUST_LARS:
                r = trust_coef * pn / (bn + (wd if flags & SEG_DECAY else 0.0) * pn + 1e-8)
            else:
                r = pn / bn
        ratio[s] = r
        nv[2 * s] = pn
        nv[2 * s + 1] = bn


def lamb_step_dev(master, grad, m, v, shadow, step_t, hyper, seg, chunk_seg, ratio, b1, b2, eps,
                  wd, adamw):
    """LAMB stage 2, or torch.optim.AdamW's rule with a per-segment decay (``adamw``)."""
    if float(hyper[HYPER_SKIP]) != 0.0:
        return
    rows, n = _seg_total(seg)
    lr, gs = float(hyper[HYPER_LR]), float(hyper[HYPER_SCALE])
    p = master[:n]
    wd_e = _decay_per_element(seg, rows, wd, p)
    if adamw:
        if wd_e is not None:
            p.mul_(1 - lr * wd_e)
        adam_step(p, grad[:n], m[:n], v[:n], None, step_t, lr, b1, b2, eps, 0.0, gs)
    else:
        m2, v2, u = _lamb_u(p, grad[:n], m[:n], v[:n], step_t, gs, b1, b2, eps, wd_e)
        m[:n].copy_(m2)
        v[:n].copy_(v2)
        p.sub_(_per_element(seg, ratio[:len(rows)].tolist(), p) * lr * u)
    if _opt(shadow) is not None:
        shadow[:n].copy_(p)


def lars_step_dev(master, grad, buf, shadow, step_t, hyper, seg, chunk_seg, ratio, momentum,
                  dampening, wd, nesterov):
    """g' = ratio[s] * (g^ + wd_s * p), then sgd_step's momentum rule with wd = 0."""
    if float(hyper[HYPER_SKIP]) != 0.0:
        return
    rows, n = _seg_total(seg)
    p = master[:n]
    g = grad[:n] * float(hyper[HYPER_SCALE])
    wd_e = _decay_per_element(seg, rows, wd, p)
    if wd_e is not None:
        g = g + wd_e * p
    g = g * _per_element(seg, ratio[:len(rows)].tolist(), p)
    sgd_step(p, g, buf[:n], None, step_t, float(hyper[HYPER_LR]), momentum, dampening, 0.0,
             nesterov, 1.0)
    if _opt(shadow) is not None:
        shadow[:n].copy_(p)


# ------------------------------------------------------------------------ preprocessing
def preprocess(img_u8, oh, ow, mean, std, mode, cpad, out_dtype, pad=None, extents=None,
               boxes=None, mix=None, lam=None):
    """u8 NHWC [B,H,W,3] -> normalized NHWC [B,oh,ow,cpad] (zero padded channels), on a
    zero-bordered canvas when pad = (top, bottom, left, right).

    mode 0: bilinear, no antialias  (train path: ToTensor -> Resize on tensor, main.py:62-65)
    mode 1: PIL bicubic (antialiased, 8-bit fixed point) -> u8 -> ToTensor -> Normalize
            (eval path, evaluation_pipeline.py:89,116-122): data/pil_resize.py, bit-exact
            with PIL.Image.resize
    mode 2: float bicubic with antialias (F.interpolate semantics)
    extents: image b occupies [:h_b, :w_b] of its slot.
    boxes (mode 0): rows (y0, x0, h, w, flip); image b is the resize of its crop
    [y0:y0+h, x0:x0+w], mirrored along W when flip is set (RandomResizedCrop ->
    RandomHorizontalFlip: the mirror of the resize's result, inside the canvas border).
    mix / lam (mode 0; Mixup / CutMix): rows (partner, y0, x0, h, w) and weights [B].  With
    P the un-mixed result in ``out_dtype``, image b is P[partner] inside its rectangle (output
    pixels, inside the canvas border) and lam * P[b] + (1 - lam) * P[partner] outside it,
    evaluated in fp32 (P[b] / P[partner] themselves at lam 1 / 0), then cast to ``out_dtype``.
    """
    if mix is not None:
        assert mode == 0 and lam is not None, "mix: mode 0 only, with lam"
        P = preprocess(img_u8, oh, ow, mean, std, mode, cpad, out_dtype, pad, extents, boxes)
        t, _bo, l, _r = pad if pad else (0, 0, 0, 0)
        out = P.clone()
        lam_h = torch.as_tensor(lam).detach().cpu().float()  # (float32 weights, as the kernel's)
        for b, (pb, y0, x0, h, w) in enumerate(torch.as_tensor(mix).tolist()):
            own, other = P[b].float(), P[pb].float()
            lb = lam_h[b]
            if float(lb) == 1.0:
                v = own.clone()
            elif float(lb) == 0.0:
                v = other.clone()
            else:
                v = lb * own + (1.0 - lb) * other
            if h > 0 and w > 0:
                v[t + y0:t + y0 + h, l + x0:l + x0 + w] = other[t + y0:t + y0 + h,
                                                                l + x0:l + x0 + w]
            out[b] = v.to(out_dtype)
        return out
    if boxes is not None:
        assert mode == 0, "boxes: mode 0 only"
        parts = []
        for b, (y0, x0, h, w, flip) in enumerate(np.asarray(boxes).tolist()):
            x = preprocess(img_u8[b:b + 1, y0:y0 + h, x0:x0 + w], oh, ow, mean, std, mode, cpad,
                           out_dtype)
            parts.append(torch.flip(x, dims=(2,)) if flip else x)
        x = torch.cat(parts, 0)
        if pad:
            t, bo, l, r = pad
            x = F.pad(x, (0, 0, l, r, t, bo))
        return x
    if extents is not None:
        parts = [preprocess(img_u8[b:b + 1, :int(h), :int(w)], oh, ow, mean, std, mode, cpad,
                            out_dtype, pad) for b, (h, w) in enumerate(extents)]
        return torch.cat(parts, 0)
    if mode == 1:
        from ..data import pil_resize
        x = torch.from_numpy(pil_resize.reference(img_u8.cpu().numpy(), (oh, ow), mean, std))
        x = x.to(img_u8.device)
    else:
        x = _nchw(img_u8.float() / 255.0)
        if (oh, ow) != tuple(x.shape[-2:]):
            if mode == 0:
                x = F.interpolate(x, size=(oh, ow), mode="bilinear", align_corners=False)
            else:
                x = F.interpolate(x, size=(oh, ow), mode="bicubic", align_corners=False,
                                  antialias=True)
        m = torch.tensor(mean, device=x.device).view(1, 3, 1, 1)
        s = torch.tensor(std, device=x.device).view(1, 3, 1, 1)
        x = _nhwc((x - m) / s)
    if cpad > 3:
        x = F.pad(x, (0, cpad - 3))
    if pad:
        t, b, l, r = pad
        x = F.pad(x, (0, 0, l, r, t, b))
    return x.to(out_dtype)


# ---------------------------------------------------------------------------- dropout
def dropout_fwd(x, p, seed, offset):
    g = torch.Generator(device=x.device)
    g.manual_seed(int(seed) * 1000003 + int(offset))
    keep = (torch.rand(x.shape, generator=g, device=x.device) >= p)
    y = (_f(x) * keep / (1 - p)).to(x.dtype)
    return y, keep.to(torch.uint8)


def dropout_bwd(dy, mask, p):
    return (_f(dy) * mask.float() / (1 - p)).to(dy.dtype)


def concat_channels(xs):
    return torch.cat(list(xs), dim=-1)


def split_channels(dy, sizes):
    return [t.contiguous() for t in torch.split(dy, list(sizes), dim=-1)]


def chan_accum(g, off, src, assign):
    cs = src.shape[-1]
    if assign:
        g[..., off:off + cs] = src.float()
    else:
        g[..., off:off + cs] += src.float()


def zero_cols_f32(t, period, first, count):
    t.view(-1, period)[:, first:first + count] = 0


def add_bf16_(a, b):
    a.add_(b)


def add_f32_(dst, src):
    dst.add_(src)


def chan_slice(src, off, cs):
    return src[..., off:off + cs].clone()


def chan_insert(dst, off, src):
    dst.data[..., off:off + src.shape[-1]] = src


def chan_extract(g, off, cs):
    return g[..., off:off + cs].clone()


def relu_fwd(x):
    return torch.relu(x)
