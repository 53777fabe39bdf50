"""Geometry-sized halo fetch of the linear-tile 3x3 kernels (``igemm_set_halo_trim``): the
producers of the 256-pixel forward / dgrad tiles and the 4-wave 128-pixel weight gradient
fetch only the halo slots a tile of the launch's geometry reads.  Every output tile is
computed from the same operands in the same order, so the results are bitwise those of the
whole-stage fetch; the planned DMA counts are the ones the geometry gives."""
import functools
import math

import pytest
import torch

from mpi_pytorch_amd.ops import ref

pytestmark = pytest.mark.gpu

# N, H, W: each spans more than one 256-pixel tile (two or more 128-pixel weight-gradient
# tiles), crosses image separators (but the one 56 x 56 image) and ends in a partial tile
IMAGES = [(6, 7, 7), (3, 14, 14), (2, 28, 28), (1, 56, 56)]
# C, K: resident weights / streamed weights in 4 chunks
CHANNELS = [(64, 64), (128, 64)]

# planned halo DMAs per wave: width -> (forward / dgrad of 9, weight gradient of 7)
TABLE = {56: (9, 7), 28: (7, 5), 14: (6, 4), 7: (6, 7)}


def C():
    from mpi_pytorch_amd.ops import _ext
    return _ext.ext()


def rel(a, b):
    a = a.float()
    b = b.float()
    return float((a - b).abs().max() / (b.abs().max() + 1e-6))


def bf(*shape, dev, scale=1.0):
    return (torch.randn(*shape, device=dev) * scale).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _inputs(N, H, W, Cc, K):
    dev = torch.device("cuda", 0)
    torch.manual_seed(61)
    x = bf(N, H, W, Cc, dev=dev)
    w = bf(K, 3, 3, Cc, dev=dev, scale=1.0 / math.sqrt(9 * Cc))
    dy = bf(N, H, W, K, dev=dev)
    shift = torch.randn(K, device=dev) * 0.1
    return x, w, dy, shift


def _on_off(fn):
    """fn() with the halo kernels on, geometry-sized fetch on and off, deterministic mode."""
    c = C()
    old = c.deterministic()
    out = []
    try:
        c.set_deterministic(1)
        c.igemm_set_halo(1)
        for trim in (1, 0):
            c.igemm_set_halo_trim(trim)
            out.append(fn())
        torch.cuda.synchronize()
    finally:
        c.igemm_set_halo_trim(1)
        c.igemm_set_halo(0)
        c.set_deterministic(int(old))
    return out


@pytest.mark.parametrize("chan", CHANNELS)
@pytest.mark.parametrize("img", IMAGES)
def test_halo_trim_fwd_dgrad(gpu, img, chan):
    """Forward (BN statistics, the training path) and stride-1 dgrad (plain and
    accumulating): trim on == trim off bitwise, and the oracle at test_kernels_gpu's bound."""
    N, H, W = img
    Cc, K = chan
    x, w, dy, shift = _inputs(N, H, W, Cc, K)
    e = torch.empty(0, device=gpu)

    def fwd():
        st = torch.zeros(2, K, device=gpu)
        return C().conv_fwd(x, w, e, 1, 1, 1, 1, False, st, shift), st

    (y, st), (y0, st0) = _on_off(fwd)
    assert torch.equal(y, y0) and torch.equal(st, st0)
    str_ = torch.zeros(2, K, device=gpu)
    yr = ref.conv_fwd(x, w, e, 1, 1, 1, 1, False, str_, shift)
    assert rel(y, yr) < 2e-2 and rel(st, str_) < 2e-2

    # dgrad of the same conv: dy [N, H, W, K] -> dx [N, H, W, C] from the transposed weight
    wt = w.permute(3, 1, 2, 0).reshape(Cc, 9, K).contiguous()
    dx, dx0 = _on_off(lambda: C().conv_dgrad(dy, w, H, W, 1, 1, 1, 1, wt))
    assert torch.equal(dx, dx0)
    dxr = ref.conv_dgrad(dy, w, H, W, 1, 1, 1, 1)
    assert rel(dx, dxr) < 2e-2
    acc0 = x  # (any [N, H, W, C] bf16 tensor: the GradJoin accumulate operand)
    acc, acc1 = _on_off(lambda: C().conv_dgrad(dy, w, H, W, 1, 1, 1, 1, wt, acc0.clone()))
    assert torch.equal(acc, acc1)
    assert rel(acc, acc0.float() + dxr.float()) < 2e-2


@pytest.mark.parametrize("kout", [64, 32])
@pytest.mark.parametrize("img", IMAGES)
def test_halo_trim_wgrad_bitwise(gpu, img, kout):
    """4-wave halo weight gradient: trim on == trim off bitwise in deterministic mode (the
    producer-wave form, which fetches whole stages, against itself as well), and the oracle
    at test_conv_halo_wgrad's bound."""
    N, H, W = img
    Cc = 64
    x, _, dy, _ = _inputs(N, H, W, Cc, kout)
    dw0 = torch.randn(kout, 3, 3, Cc, device=gpu)
    dwr = dw0.clone()
    ref.conv_wgrad(dy, x, dwr, 1, 1, 1, 1)

    def run():
        dw = dw0.clone()
        C().conv_wgrad(dy, x, dw, 1, 1, 1, 1)
        return dw

    try:
        for prod in (0, 1):
            C().igemm_set_halo_wprod(prod)
            dw, dw1 = _on_off(run)
            assert torch.equal(dw, dw1)
            assert rel(dw - dw0, dwr - dw0) < 1e-2
    finally:
        C().igemm_set_halo_wprod(1)


def test_halo_trim_dma_counts(gpu):
    """The planned DMA count per shape: the slots a tile's taps reach, in 16-slot
    instructions dealt over 4 waves; the whole stage with the trim off."""
    c = C()
    try:
        for w, (f, g) in TABLE.items():
            c.igemm_set_halo_trim(1)
            assert (c.conv3_halo_dma_count(w, w), c.conv3_halo_wgrad_dma_count(w, w)) == (f, g)
            c.igemm_set_halo_trim(0)
            assert (c.conv3_halo_dma_count(w, w), c.conv3_halo_wgrad_dma_count(w, w)) == (9, 7)
    finally:
        c.igemm_set_halo_trim(1)
