"""Mixup / CutMix on the device: the mixed preprocess launch (``Fn.preprocess(mix=, lam=)``,
``csrc/kernels/preprocess.hip``) and the two-label cross-entropy (``csrc/kernels/loss.hip``).

The preprocess identity is the definition: with P the output of the same launch without
``mix`` / ``lam``, image b of the mixed launch is P[partner] inside its rectangle and, outside
it, BITWISE the fp32 expression ``(lam * P[b].float() + (1 - lam) * P[partner].float())
.bfloat16()`` (P[b] / P[partner] themselves at lam 1 / 0), over the whole canvas.  The
cross-entropy checks reuse the shapes, inputs and bounds of ``test_loss_head_gpu.py``.

Every check takes the implementation and the device, so ``test_mix_cpu.py`` runs them with
the oracle (``ops/ref.py``) on the CPU: a GPU failure is then the kernel's."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_loss_head_gpu as lh
from mpi_pytorch_amd.ops import functional as Fn
from mpi_pytorch_amd.ops import ref

pytestmark = pytest.mark.gpu
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

# ----------------------------------------------------------------------------- preprocess
B = 10
PARTNERS = [1, 0, 2, 4, 5, 3, 7, 8, 9, 6]        # a 2-cycle, a self-partner, a 3- and a 4-cycle
LAM = [1, 0, 0.5, 0.25, 0.3, 0.7, 1, 1, 0.123, 0.999]
# 16-B, 4-B and byte staging, global taps, and one slot on each side of the widest slot a
# mixed launch stages (PP_MIX_MAXW = 672 pixels)
SLOTS = [(24, 64), (17, 20), (19, 21), (12, 1400), (9, 672), (9, 673)]
DSTS = [(16, 16), (37, 91)]
LAYOUTS = [(3, None), (8, None), (4, (3, 3, 3, 3))]
CASES = [(s, d, l) for s in SLOTS for d in DSTS for l in LAYOUTS]
VARIANTS = ["plain", "boxes", "extents", "all"]


def rectangles(OH, OW, n=B):
    """(y0, x0, h, w) per image, cycled: empty, the whole image, 1x1 at (0, 0), flush with the
    bottom-right corner, one full row, one full column, an interior box."""
    kinds = [(0, 0, 0, 0), (0, 0, OH, OW), (0, 0, 1, 1), (OH - 5, OW - 7, 5, 7), (3, 0, 1, OW),
             (0, 4, OH, 1), (2, 3, OH // 2, OW // 3)]
    return [kinds[i % len(kinds)] for i in range(n)]


def mix_rows(dst, partners=PARTNERS):
    return np.array([[p] + list(r) for p, r in zip(partners, rectangles(*dst, len(partners)))],
                    dtype=np.int32)


def boxes_for(H, W):
    """Ten crop boxes of an [H][W] image (the shapes of test_augment_gpu.py)."""
    return np.array([[0, 0, H, W, 0], [H // 2, W // 3, 1, 1, 0], [0, 0, H - 3, W - 5, 0],
                     [3, 5, H - 3, W - 5, 0], [0, 7, H, W - 7, 0], [H - 1, 0, 1, W, 0],
                     [0, W - 1, H, 1, 0], [2, 1, H - 4, W - 2, 0], [1, 3, 5, 7, 0],
                     [H - 2, W - 9, 2, 9, 0]], dtype=np.int32)


def geometry(variant, H, W):
    """(extents, boxes) of a variant.  extents: partners differ in extent; boxes: every other
    image flipped; all: each image's box lies inside its own extent."""
    ext = boxes = None
    if variant in ("extents", "all"):
        ext = np.array([[H - b % 3, W - b % 4] for b in range(B)])
    if variant == "boxes":
        boxes = boxes_for(H, W)
    if variant == "all":
        boxes = np.stack([boxes_for(int(h), int(w))[b] for b, (h, w) in enumerate(ext)])
    if boxes is not None:
        boxes[::2, 4] = 1
    return ext, boxes


def blend_of(P, mix, lam, pad):
    """The definition, from the un-mixed result P (any float dtype; evaluated in fp32 on the
    CPU with one rounding per operation, cast back to P's dtype)."""
    t, _b, l, _r = pad or (0, 0, 0, 0)
    Pf = P.detach().cpu().float()
    out = torch.empty_like(Pf)
    for b, (p, y0, x0, h, w) in enumerate(np.asarray(mix).tolist()):
        lb = torch.tensor(float(lam[b]), dtype=torch.float32)
        own, other = Pf[b], Pf[p]
        if float(lb) == 1.0:
            v = own.clone()
        elif float(lb) == 0.0:
            v = other.clone()
        else:
            v = lb * own + (1.0 - lb) * other
        if h > 0 and w > 0:
            v[t + y0:t + y0 + h, l + x0:l + x0 + w] = other[t + y0:t + y0 + h, l + x0:l + x0 + w]
        out[b] = v
    return out.to(P.dtype)


def pre(dev, img, dst, cpad, pad, **kw):
    """``Fn.preprocess`` to bf16 on ``dev`` (the kernel on the GPU, the oracle on the CPU)."""
    return Fn.preprocess(img.to(dev), dst, MEAN, STD, 0, cpad, out_dtype=torch.bfloat16, pad=pad,
                         **kw)


def images(n, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, H, W, 3), generator=g, dtype=torch.uint8)


def check_blend(dev, case):
    (H, W), dst, (cpad, pad) = case
    img = images(B, H, W, H * 1000 + W + dst[1])
    mix, lam = mix_rows(dst), np.array(LAM, dtype=np.float32)
    for variant in VARIANTS:
        ext, boxes = geometry(variant, H, W)
        P = pre(dev, img, dst, cpad, pad, extents=ext, boxes=boxes)
        out = pre(dev, img, dst, cpad, pad, extents=ext, boxes=boxes, mix=mix, lam=lam)
        assert out.dtype == torch.bfloat16 and out.shape == P.shape
        exp = blend_of(P, mix, lam, pad)
        same = torch.equal(out.cpu(), exp)
        if not same:
            bad = (out.cpu().float() != exp.float()).flatten(1).any(1).nonzero().flatten().tolist()
            print("mixed launch differs", case, variant, "images", bad)
        assert same, (case, variant)
        assert not torch.equal(out.cpu(), P.cpu())      # (and it did mix)
        rest = out.clone()                               # canvas border + padding channels
        t, _b, l, _r = pad or (0, 0, 0, 0)
        rest[:, t:t + dst[0], l:l + dst[1], :3] = 0
        assert not rest.any()


def check_inert(dev, case):
    """Source pixels outside the crop boxes do not matter, for an image's own pixels and for
    the ones its partner reads; lam = 1 with empty rectangles is P whatever the partners."""
    (H, W), dst, (cpad, pad) = case
    img = images(B, H, W, 77 + W)
    _ext, boxes = geometry("boxes", H, W)
    mix, lam = mix_rows(dst), np.array(LAM, dtype=np.float32)
    out = pre(dev, img, dst, cpad, pad, boxes=boxes, mix=mix, lam=lam)
    other = 255 - img
    for b, (y0, x0, h, w, _f) in enumerate(boxes.tolist()):
        other[b, y0:y0 + h, x0:x0 + w] = img[b, y0:y0 + h, x0:x0 + w]
    assert torch.equal(pre(dev, other, dst, cpad, pad, boxes=boxes, mix=mix, lam=lam), out)
    P = pre(dev, img, dst, cpad, pad, boxes=boxes)
    none = mix.copy()
    none[:, 1:] = 0
    ones = np.ones(B, dtype=np.float32)
    assert torch.equal(pre(dev, img, dst, cpad, pad, boxes=boxes, mix=none, lam=ones), P)


def check_against_oracle(dev, case):
    (H, W), dst, (cpad, pad) = case
    img = images(B, H, W, 5 + H)
    _ext, boxes = geometry("boxes", H, W)
    mix, lam = mix_rows(dst), np.array(LAM, dtype=np.float32)
    out = pre(dev, img, dst, cpad, pad, boxes=boxes, mix=mix, lam=lam)
    exp = ref.preprocess(img, dst[0], dst[1], MEAN, STD, 0, cpad, torch.float32, pad,
                         boxes=boxes, mix=mix, lam=lam)
    assert out.shape == exp.shape
    err = float((out.float().cpu() - exp).abs().max())
    print("max abs err", err)
    assert err < 0.05        # test_augment_gpu.py::test_boxed_kernel_against_oracle's bound


def check_rejections(dev):
    """Every host-side ``ValueError``; none of them launches."""
    img = torch.zeros(3, 12, 10, 3, dtype=torch.uint8, device=dev)
    ok = [[1, 0, 0, 0, 0], [2, 1, 1, 3, 3], [0, 0, 0, 4, 4]]
    lam = [0.5, 1.0, 0.0]
    call = lambda m, l, mode=0: Fn.preprocess(img, (4, 4), MEAN, STD, mode, 3,
                                              out_dtype=torch.bfloat16, mix=m, lam=l)
    call(ok, lam)
    bad_rows = [[3, 0, 0, 0, 0], [-1, 0, 0, 0, 0],          # partner outside [0, B)
                [0, 0, 0, 5, 1], [0, 0, 0, 1, 5], [0, 3, 0, 2, 1], [0, 0, 3, 1, 2],   # outside
                [0, -1, 0, 1, 1], [0, 0, -1, 1, 1], [0, 1, 1, -1, 1], [0, 1, 1, 1, -1]]
    for row in bad_rows:
        with pytest.raises(ValueError):
            call([ok[0], row, ok[2]], lam)
    for bad_lam in ([0.5, 1.5, 0.0], [0.5, -0.1, 0.0], [0.5, float("nan"), 0.0],
                    [0.5, float("inf"), 0.0], [0.5, 1.0], [1, 1, 0]):     # range, shape, dtype
        with pytest.raises(ValueError):
            call(ok, bad_lam)
    for bad_mix in (ok[:2], [r[:4] for r in ok], np.array(ok, dtype=np.float32)):
        with pytest.raises(ValueError):
            call(bad_mix, lam)
    for m, l in ((ok, None), (None, lam)):                   # one without the other
        with pytest.raises(ValueError):
            call(m, l)
    for mode in (1, 2):
        with pytest.raises(ValueError):
            call(ok, lam, mode)


# --------------------------------------------------------------------------- cross-entropy
CE_EPS = [0.0, 0.1]
GO, WEIGHT = lh.GO, lh.WEIGHT


def mixed_labels(Bn, NC, dev, dyadic=False):
    labels = torch.randint(0, NC, (Bn,), device=dev)
    labels2 = torch.randint(0, NC, (Bn,), device=dev)
    labels2[0] = labels[0]
    if dyadic:
        lam = torch.tensor([0.25, 0.5, 0.75], device=dev)[torch.randint(0, 3, (Bn,), device=dev)]
    else:
        lam = torch.rand(Bn, device=dev) * 0.98 + 0.01
        lam[1], lam[2] = 1.0, 0.0
    return labels, labels2, lam.float().contiguous()


def check_ce_random(impl, dev, Bn, NC, ld, eps):
    torch.manual_seed(90)
    logits = lh.padded(torch.randn(Bn, NC, device=dev) * 3 + 2, ld)
    y, y2, lam = mixed_labels(Bn, NC, dev)
    loss, lse = impl.ce_fwd(logits, y, eps, y2, lam)
    lossr, lser = ref.ce_fwd(logits, y, eps, y2, lam)
    go = torch.full((1,), GO, device=dev)
    d = impl.ce_bwd(logits, y, lse, go, WEIGHT, eps, y2, lam)
    dr = ref.ce_bwd(logits, y, lser, go, WEIGHT, eps, y2, lam)
    print("mixed ce", (Bn, NC, ld), eps, float(loss), float(lossr), lh.rel(lse, lser),
          lh.rel(d, dr))
    assert lh.loss_close(loss, lossr)
    assert lh.rel(lse, lser) < 1e-4
    assert d.shape == (Bn, NC) and lh.rel(d, dr) < 2e-2
    assert lh.pad_is_zero(impl, d, ld)


def check_ce_flat(impl, dev, Bn, NC, ld, eps):
    """Every valid logit 2.0: closed forms by position (the max-norm bound cannot see a
    small second-label term), with check_smoothed_flat's error forms."""
    torch.manual_seed(91)
    logits = lh.padded(torch.full((Bn, NC), 2.0, device=dev), ld)
    y, y2, lam = mixed_labels(Bn, NC, dev)
    loss, lse = impl.ce_fwd(logits, y, eps, y2, lam)
    assert lh.loss_close(loss, math.log(NC)), (float(loss), math.log(NC))
    go = torch.full((1,), GO, device=dev)
    dv = impl.ce_bwd(logits, y, lse, go, WEIGHT, eps, y2, lam)
    d = dv.float()
    s = GO * WEIGHT
    onw, unif, unit = 1.0 - eps, eps / NC, s / (Bn * NC)
    rows = torch.arange(Bn, device=dev)
    want = torch.full((Bn, NC), (1.0 / NC - unif) * s / Bn, device=dev, dtype=torch.float64)
    lam64 = lam.double()
    same = y == y2
    want[rows, y] = (1.0 / NC - onw * lam64 - unif) * s / Bn
    want[rows, y2] = torch.where(same, (1.0 / NC - onw - unif) * s / Bn,
                                 (1.0 / NC - onw * (1.0 - lam64) - unif) * s / Bn)
    is_label = torch.zeros(Bn, NC, dtype=torch.bool, device=dev)
    is_label[rows, y] = True
    is_label[rows, y2] = True
    err = (d.double() - want).abs()
    other = (1.0 / NC - unif) * s / Bn
    err_other = float(err[~is_label].max())
    print("mixed flat", (Bn, NC, ld), eps, float(loss), err_other,
          float((err[is_label] / (want[is_label].abs() + 1e-30)).max()))
    assert err_other <= max(1e-2 * abs(other), 1e-3 * unit), (err_other, other)
    assert bool((err[is_label] <= 1e-2 * want[is_label].abs() + 1e-3 * unit).all())
    assert bool(same[0]) and float(lam[1]) == 1.0 and float(lam[2]) == 0.0
    assert lh.pad_is_zero(impl, dv, ld)


def check_ce_bitwise(impl, dev, Bn, NC, ld):
    """lam = 1 / 0 everywhere is the plain call on labels / labels2; dyadic lam: swapping the
    labels and lam -> 1 - lam changes nothing; a mixed forward repeats; labels2 = None is the
    plain call."""
    torch.manual_seed(92)
    logits = lh.padded(torch.randn(Bn, NC, device=dev) * 3 + 2, ld)
    y, y2, lam = mixed_labels(Bn, NC, dev, dyadic=True)
    go = torch.full((1,), GO, device=dev)
    one, zero = torch.ones_like(lam), torch.zeros_like(lam)
    for eps in CE_EPS:
        lp, sp = impl.ce_fwd(logits, y, eps)
        dp = impl.ce_bwd(logits, y, sp, go, WEIGHT, eps)
        lq, sq = impl.ce_fwd(logits, y2, eps)
        dq = impl.ce_bwd(logits, y2, sq, go, WEIGHT, eps)
        for lm, (lw, sw, dw) in ((one, (lp, sp, dp)), (zero, (lq, sq, dq))):
            l1, s1 = impl.ce_fwd(logits, y, eps, y2, lm)
            assert torch.equal(l1, lw) and torch.equal(s1, sw)
            assert torch.equal(impl.ce_bwd(logits, y, s1, go, WEIGHT, eps, y2, lm), dw)
        la, sa = impl.ce_fwd(logits, y, eps, y2, lam)
        lb, sb = impl.ce_fwd(logits, y2, eps, y, 1.0 - lam)
        assert torch.equal(la, lb) and torch.equal(sa, sb)
        assert torch.equal(impl.ce_bwd(logits, y, sa, go, WEIGHT, eps, y2, lam),
                           impl.ce_bwd(logits, y2, sb, go, WEIGHT, eps, y, 1.0 - lam))
        lc, sc = impl.ce_fwd(logits, y, eps, y2, lam)
        assert torch.equal(la, lc) and torch.equal(sa, sc)
        assert not torch.equal(la, lp)                       # (and mixing changes the loss)
        ln, sn = impl.ce_fwd(logits, y, eps, None, None)
        assert torch.equal(ln, lp) and torch.equal(sn, sp)
        assert torch.equal(impl.ce_bwd(logits, y, sn, go, WEIGHT, eps, None, None), dp)


def check_ce_weighted(impl, dev, Bn, NC, ld):
    """check_smoothed_weighted with two labels per row."""
    torch.manual_seed(93)
    out, acc = torch.full((1,), 123.0, device=dev), torch.full((1,), 5.0, device=dev)
    outr, accr = out.clone(), acc.clone()
    for accumulate in (False, True):
        logits = lh.padded(torch.randn(Bn, NC, device=dev) * 3 + 2, ld)
        y, y2, lam = mixed_labels(Bn, NC, dev)
        lse = impl.ce_fwd_weighted(logits, y, out, acc, 0.4, accumulate, 0.1, y2, lam)
        lser = ref.ce_fwd_weighted(logits, y, outr, accr, 0.4, accumulate, 0.1, y2, lam)
        print("mixed weighted", (Bn, NC, ld), accumulate, float(out), float(outr), float(acc),
              float(accr), lh.rel(lse, lser))
        assert lh.loss_close(out, outr) and lh.loss_close(acc, accr)
        assert lh.rel(lse, lser) < 1e-4


def check_ce_autograd(dev, Bn=7, NC=1000, ld=1024):
    """``Fn.cross_entropy`` with an aux head, eps = 0.1, mixed, against the fp32 CPU oracle
    lam * CE(x, y) + (1 - lam) * CE(x, y2) (per row, then the mean) from the same bf16 logits;
    check_autograd's tolerances."""
    torch.manual_seed(94)
    dt = torch.bfloat16 if dev.type == "cuda" else torch.float32
    mains = [(torch.randn(Bn, NC) * 3 + 2).to(torch.bfloat16) for _ in range(2)]
    y, y2, lam = mixed_labels(Bn, NC, torch.device("cpu"))
    fulls = []
    for v in mains:
        f_ = torch.full((Bn, ld), lh.SENTINEL, dtype=dt)
        f_[:, :NC] = v.to(dt)
        fulls.append(f_.to(dev).requires_grad_(True))
    lg, aux = fulls[0][:, :NC], fulls[1][:, :NC]
    loss = Fn.cross_entropy(lg, y.to(dev), label_smoothing=0.1, heads=[(aux, 0.4)],
                            labels2=y2.to(dev), lam=lam.to(dev))
    loss.backward()
    want_in = [v.float().requires_grad_(True) for v in mains]
    ce = lambda x, t: F.cross_entropy(x, t, reduction="none", label_smoothing=0.1)
    head = lambda x: (lam * ce(x, y) + (1.0 - lam) * ce(x, y2)).mean()
    want = head(want_in[0]) + 0.4 * head(want_in[1])
    want.backward()
    assert lh.loss_close(loss, want), (float(loss), float(want))
    for f_, w in zip(fulls, want_in):
        g = f_.grad.cpu()
        print("mixed autograd", lh.rel(g[:, :NC], w.grad))
        assert lh.rel(g[:, :NC], w.grad) < 2e-2
        assert float(g[:, NC:].float().abs().max()) == 0.0


# ------------------------------------------------------------------------------- GPU runs
def C():
    from mpi_pytorch_amd.ops import _ext
    return _ext.ext()


@pytest.mark.parametrize("case", CASES, ids=str)
def test_mixed_launch_is_the_blend_of_the_unmixed_launch(gpu, case):
    check_blend(gpu, case)


def test_identity_size_mixes_the_copy_kernels_output(gpu):
    """The un-mixed launch takes the copy fast path; the mixed one goes through the bilinear
    kernel and is still the bitwise blend of it."""
    dst, cpad, pad = (16, 32), 4, (3, 3, 3, 3)
    img = images(B, 16, 32, 1632)
    mix, lam = mix_rows(dst), np.array(LAM, dtype=np.float32)
    P = pre(gpu, img, dst, cpad, pad)
    out = pre(gpu, img, dst, cpad, pad, mix=mix, lam=lam)
    assert torch.equal(out.cpu(), blend_of(P, mix, lam, pad))
    assert not torch.equal(out, P)


def test_more_items_than_blocks(gpu):
    """520 images x 4 row groups = 2,080 work items on the 2,048-block grid: the stride loop
    re-stages both images per item."""
    n, dst = 520, (32, 16)
    img = images(n, 8, 16, 520)
    mix = np.zeros((n, 5), dtype=np.int32)
    mix[:, 0] = (np.arange(n) + 1) % n
    lam = np.full(n, 0.5, dtype=np.float32)
    P = pre(gpu, img, dst, 4, None)
    out = pre(gpu, img, dst, 4, None, mix=mix, lam=lam)
    assert torch.equal(out.cpu(), blend_of(P, mix, lam, None))


@pytest.mark.parametrize("case", CASES[::5], ids=str)
def test_pixels_outside_the_boxes_and_identity_rows_are_inert(gpu, case):
    check_inert(gpu, case)


@pytest.mark.parametrize("case", CASES[::3], ids=str)
def test_mixed_kernel_against_oracle(gpu, case):
    check_against_oracle(gpu, case)


def test_bad_mix_rows_are_rejected_on_the_host(gpu):
    check_rejections(gpu)
    # the binding's own argument checks (shape, dtype, device, mode, a missing half or box)
    k = C()
    img = torch.zeros(2, 12, 10, 3, dtype=torch.uint8, device=gpu)
    box = torch.tensor([[0, 0, 12, 10, 0]] * 2, dtype=torch.int32, device=gpu)
    mix = torch.tensor([[1, 0, 0, 2, 2], [0, 0, 0, 0, 0]], dtype=torch.int32, device=gpu)
    lam = torch.tensor([0.5, 1.0], device=gpu)
    call = lambda mode=0, **kw: k.preprocess(img, 4, 4, list(MEAN), list(STD), mode, 3, [], None,
                                             **kw)
    call(box=box, mix=mix, lam=lam)
    for kw in (dict(box=box, mix=mix.long(), lam=lam), dict(box=box, mix=mix.cpu(), lam=lam),
               dict(box=box, mix=mix[:1], lam=lam), dict(box=box, mix=mix[:, :4], lam=lam),
               dict(box=box, mix=mix, lam=lam.double()), dict(box=box, mix=mix, lam=lam[:1]),
               dict(box=box, mix=mix, lam=lam.cpu()), dict(box=box, mix=mix),
               dict(box=box, lam=lam), dict(mix=mix, lam=lam),
               dict(box=box, mix=mix.t().contiguous().t(), lam=lam)):
        with pytest.raises(RuntimeError):
            call(**kw)
    with pytest.raises(RuntimeError):
        call(2, box=box, mix=mix, lam=lam)
    logits = lh.padded(torch.zeros(2, 8, device=gpu), 8)
    y = torch.zeros(2, dtype=torch.int64, device=gpu)
    for y2, lm in ((y, None), (None, lam), (y.int(), lam), (y[:1], lam), (y, lam.double()),
                   (y.cpu(), lam), (y, lam[:1])):
        with pytest.raises(RuntimeError):
            k.ce_fwd(logits, y, 0.0, y2, lm)


@pytest.mark.parametrize("eps", CE_EPS)
@pytest.mark.parametrize("shape", lh.SHAPES)
def test_mixed_ce_random(gpu, shape, eps):
    check_ce_random(C(), gpu, *shape, eps)


@pytest.mark.parametrize("eps", CE_EPS)
@pytest.mark.parametrize("shape", lh.SHAPES)
def test_mixed_ce_flat_closed_forms(gpu, shape, eps):
    check_ce_flat(C(), gpu, *shape, eps)


@pytest.mark.parametrize("shape", lh.SHAPES)
def test_mixed_ce_bitwise_properties(gpu, shape):
    check_ce_bitwise(C(), gpu, *shape)


@pytest.mark.parametrize("shape", [(300, 33, 64), (7, 1000, 1024), (7, 1004, 1004)])
def test_mixed_ce_fwd_weighted(gpu, shape):
    check_ce_weighted(C(), gpu, *shape)


def test_mixed_cross_entropy_autograd(gpu):
    check_ce_autograd(gpu)


# ------------------------------------------------------------------------------ the step
@pytest.fixture
def det(gpu):
    k = C()
    old = k.deterministic()
    k.set_deterministic(1)
    yield gpu
    k.set_deterministic(int(old))


def _train(gpu):
    from mpi_pytorch_amd.engine import build_training
    from mpi_pytorch_amd.parallel import World
    torch.manual_seed(0)
    return build_training("resnet18", 100, gpu, World(device=gpu), 1e-3, label_smoothing=0.1)[:3]


def _batches(gpu, Bn=32, hw=64, nc=100):
    """One image batch and three different mixed label sets + one plain one."""
    from mpi_pytorch_amd.engine import MixedLabels
    g = torch.Generator(device="cpu").manual_seed(1)
    x = (torch.randn(Bn, hw, hw, 8, generator=g) * (torch.arange(8) < 3)).to(gpu, torch.bfloat16)
    ys = []
    for _ in range(3):
        y = torch.randint(0, nc, (Bn,), generator=g)
        y2 = torch.randint(0, nc, (Bn,), generator=g)
        lam = torch.rand(Bn, generator=g)
        ys.append(MixedLabels(y.to(gpu), y2.to(gpu), lam.to(gpu)))
    return x, ys, torch.randint(0, nc, (Bn,), generator=g).to(gpu)


def test_mixed_step_repeats_and_graph_replays_reread_the_labels(det):
    """ResNet-18 as in test_recipe_gpu.py's graph-replay test, deterministic mode: a mixed
    step repeats bitwise; three replays fed three different MixedLabels equal three eager
    steps (labels2 and lam are re-read, not frozen at capture); a plain-label call on the
    captured step runs eagerly and equals the uncaptured step."""
    gpu = det
    x, ys, plain = _batches(gpu)
    # eager: three mixed steps, then a plain one
    model, opt, step = _train(gpu)
    losses, masters = [], []
    for y in ys:
        losses.append(step(x, y).clone())
        masters.append(model._mpa_arena.master.clone())
    loss_sum = step.loss_sum.clone()
    losses.append(step(x, plain).clone())
    torch.cuda.synchronize()
    masters.append(model._mpa_arena.master.clone())
    assert not torch.equal(losses[0], losses[1])
    del model, opt, step
    # the first step again
    model, opt, step = _train(gpu)
    l0 = step(x, ys[0]).clone()
    torch.cuda.synchronize()
    assert torch.equal(l0, losses[0]) and torch.equal(model._mpa_arena.master, masters[0])
    del model, opt, step
    # graph
    model, opt, step = _train(gpu)
    assert step.capture(x, ys[0], warmup=2)
    got = [step(x, y).clone() for y in ys]
    torch.cuda.synchronize()
    assert torch.equal(torch.stack(got), torch.stack(losses[:3]))
    assert torch.equal(model._mpa_arena.master, masters[2])
    assert torch.equal(step.loss_sum, loss_sum)
    lp = step(x, plain).clone()                  # the other label kind: eager
    torch.cuda.synchronize()
    assert torch.equal(lp, losses[3]) and torch.equal(model._mpa_arena.master, masters[3])
    # ... and the captured kind still replays afterwards
    assert step._graph is not None and isinstance(step._static_y, tuple)
