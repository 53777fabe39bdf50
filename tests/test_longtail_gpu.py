"""The long-tail head (csrc/kernels/loss.hip): logit-adjusted cross-entropy and the per-class
counters behind macro-F1 / balanced accuracy.

Every check takes the implementation and the device, so ``test_longtail_cpu.py`` runs the
same checks with the oracle (``ops/ref.py``) on the CPU: each bound below is met by the
oracle alone, and a GPU failure is the kernel's.  Inputs are drawn on the CPU from a seeded
generator, so both runs see the same values.

Adjusted CE is ``F.cross_entropy(x.float() + bias, target, label_smoothing=eps)``:
    z        = float(x) + bias                (fp32, inside the kernels)
    loss_row = lse(z) - (1-eps) * (lam*z[y] + (1-lam)*z[y2]) - (eps/NC) * sum_c z[c]
    dx[c]    = (exp(z[c] - lse) - target[c]) * grad_out * weight / B
Bounds are ``test_loss_head_gpu.py``'s: loss 1e-3 * max(1, |ref|), rel(lse) < 1e-4, gradient
rel < 2e-2 in the max norm, gradient pad columns exactly zero.  The bias is tau * log prior
of Zipf-like counts (about [-13, -1]): dropping it moves the loss by far more than the
bound.  Pad logits carry the finite sentinel 1000.0 and the bias is allocated with ``ld``
floats whose columns NC..ld-1 hold NaN, so a read of either shows in the loss, the LSE or
the gradient."""
import pytest
import torch
import torch.nn.functional as F

import test_loss_head_gpu as lh
from mpi_pytorch_amd.ops import ref

pytestmark = pytest.mark.gpu

SHAPES = lh.SHAPES
EPS = [0.0, 0.1]
GO, WEIGHT = lh.GO, lh.WEIGHT
rel, padded, loss_close, pad_is_zero, C = lh.rel, lh.padded, lh.loss_close, lh.pad_is_zero, lh.C


def gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def zipf_log_prior(NC, g):
    """float64 log prior of counts proportional to 1 / rank, the ranks shuffled."""
    rank = torch.randperm(NC, generator=g).double() + 1.0
    p = 1.0 / rank
    return torch.log(p / p.sum())


def nan_padded(vals, ld, dev):
    """fp32 [NC] values in a buffer of ``ld`` floats whose tail is NaN."""
    NC = vals.numel()
    full = torch.full((max(ld, NC),), float("nan"), dtype=torch.float32)
    full[:NC] = vals.float()
    return full.to(dev)


def make_case(dev, B, NC, ld, seed, mixed):
    g = gen(seed)
    logits = padded((torch.randn(B, NC, generator=g) * 3 + 2).to(dev), ld)
    y = torch.randint(0, NC, (B,), generator=g).to(dev)
    bias = nan_padded(zipf_log_prior(NC, g), ld, dev)
    mix = ()
    if mixed:
        y2 = torch.randint(0, NC, (B,), generator=g)
        y2[0] = y[0]  # both labels one column
        lam = torch.rand(B, generator=g)
        lam[-1] = 1.0
        mix = (y2.to(dev), lam.float().contiguous().to(dev))
    return logits, y, bias, mix


def mix_args(mix):
    return mix if mix else (None, None)


# ------------------------------------------------------------------------- adjusted CE
def check_adjusted_random(impl, dev, B, NC, ld, eps, mixed):
    logits, y, bias, mix = make_case(dev, B, NC, ld, 90, mixed)
    assert -14.0 < float(bias[:NC].min()) < -4.0 and -4.0 < float(bias[:NC].max()) < -1.0
    loss, lse = impl.ce_fwd(logits, y, eps, *mix_args(mix), bias)
    lossr, lser = ref.ce_fwd(logits, y, eps, *mix_args(mix), bias)
    go = torch.full((1,), GO, device=dev)
    d = impl.ce_bwd(logits, y, lse, go, WEIGHT, eps, *mix_args(mix), bias)
    dr = ref.ce_bwd(logits, y, lser, go, WEIGHT, eps, *mix_args(mix), bias)
    _, lse_plain = ref.ce_fwd(logits, y, eps, *mix_args(mix))
    print("adjusted", (B, NC, ld), eps, mixed, float(loss), float(lossr), rel(lse, lser),
          rel(lse_plain, lser), rel(d, dr))
    assert rel(lse_plain, lser) > 100 * 1e-4  # (a dropped bias is a hundred bounds away)
    assert loss_close(loss, lossr)
    assert rel(lse, lser) < 1e-4
    assert d.shape == (B, NC) and rel(d, dr) < 2e-2
    assert pad_is_zero(impl, d, ld)


def check_constant_bias(impl, dev, B, NC, ld):
    """bias = k on every class: lse shifts by k, the unsmoothed loss and the gradient stay."""
    k = -3.5
    logits, y, _, mix = make_case(dev, B, NC, ld, 91, True)
    bias = nan_padded(torch.full((NC,), k), ld, dev)
    go = torch.full((1,), GO, device=dev)
    for mx in ((), mix):
        l0, s0 = impl.ce_fwd(logits, y, 0.0, *mix_args(mx))
        l1, s1 = impl.ce_fwd(logits, y, 0.0, *mix_args(mx), bias)
        d0 = impl.ce_bwd(logits, y, s0, go, WEIGHT, 0.0, *mix_args(mx))
        d1 = impl.ce_bwd(logits, y, s1, go, WEIGHT, 0.0, *mix_args(mx), bias)
        print("constant", (B, NC, ld), bool(mx), float(l0), float(l1), rel(s1, s0 + k),
              rel(d1, d0))
        assert rel(s1, s0 + k) < 1e-4
        assert loss_close(l1, l0)
        assert rel(d1, d0) < 2e-2
        assert pad_is_zero(impl, d1, ld)


def check_null_and_zero_bias(impl, dev, B, NC, ld):
    """bias=None is the existing call; bias = 0 equals it bitwise (x + 0.0f is exact)."""
    logits, y, _, mix = make_case(dev, B, NC, ld, 92, True)
    zero = nan_padded(torch.zeros(NC), ld, dev)
    go = torch.full((1,), GO, device=dev)
    for eps in EPS:
        lp, sp = impl.ce_fwd(logits, y, eps)
        dp = impl.ce_bwd(logits, y, sp, go, WEIGHT, eps)
        for mx in ((), mix):
            l0, s0 = impl.ce_fwd(logits, y, eps, *mix_args(mx))
            d0 = impl.ce_bwd(logits, y, s0, go, WEIGHT, eps, *mix_args(mx))
            ln, sn = impl.ce_fwd(logits, y, eps, *mix_args(mx), None)
            dn = impl.ce_bwd(logits, y, sn, go, WEIGHT, eps, *mix_args(mx), None)
            lz, sz = impl.ce_fwd(logits, y, eps, *mix_args(mx), zero)
            dz = impl.ce_bwd(logits, y, sz, go, WEIGHT, eps, *mix_args(mx), zero)
            assert torch.equal(ln, l0) and torch.equal(sn, s0) and torch.equal(dn, d0)
            assert torch.equal(lz, l0) and torch.equal(sz, s0) and torch.equal(dz, d0)
            if not mx:
                assert torch.equal(l0, lp) and torch.equal(s0, sp) and torch.equal(d0, dp)


def check_flat_logits(impl, dev, B, NC, ld):
    """All-zero logits: lse = logsumexp(bias), loss = lse - mean bias[y], dx = (softmax(bias) -
    onehot) * scale.  A bias applied to the label only, or to the LSE only, fails."""
    g = gen(93)
    logits = padded(torch.zeros(B, NC, device=dev), ld)
    y = torch.randint(0, NC, (B,), generator=g)
    b32 = (1.5 * zipf_log_prior(NC, g)).float()  # (tau = 1: the priors' lse would be 0)
    bias = nan_padded(b32, ld, dev)
    want_lse = float(torch.logsumexp(b32.double(), 0))
    want_loss = want_lse - float(b32.double()[y].mean())
    loss, lse = impl.ce_fwd(logits, y.to(dev), 0.0, None, None, bias)
    print("flat", (B, NC, ld), float(loss), want_loss, float(lse[0]), want_lse)
    assert float((lse.double() - want_lse).abs().max()) < 1e-4 * abs(want_lse)
    assert loss_close(loss, want_loss)
    go = torch.full((1,), GO, device=dev)
    dv = impl.ce_bwd(logits, y.to(dev), lse, go, WEIGHT, 0.0, None, None, bias)
    d = dv.double().cpu()
    scale = GO * WEIGHT / B
    want = torch.softmax(b32.double(), 0).expand(B, NC).clone()
    want[torch.arange(B), y] -= 1.0
    want *= scale
    # every element on its own: the result is a bf16 (half an ulp is 2^-9) of an fp32 product
    # of a fast exp (a few 1e-6 per unit of its argument, |z - lse| < 16): 1e-2 relative
    err = ((d - want).abs() / want.abs()).max()
    print("flat grad", float(err))
    assert float(err) < 1e-2
    assert pad_is_zero(impl, dv, ld)


def check_adjusted_weighted(impl, dev, B, NC, ld):
    """``check_smoothed_weighted`` with a bias: two heads, assign then accumulate."""
    out, acc = torch.full((1,), 123.0, device=dev), torch.full((1,), 5.0, device=dev)
    outr, accr = out.clone(), acc.clone()
    for accumulate in (False, True):
        logits, y, bias, mix = make_case(dev, B, NC, ld, 94 + int(accumulate), accumulate)
        lse = impl.ce_fwd_weighted(logits, y, out, acc, 0.4, accumulate, 0.1, *mix_args(mix),
                                   bias)
        lser = ref.ce_fwd_weighted(logits, y, outr, accr, 0.4, accumulate, 0.1, *mix_args(mix),
                                   bias)
        print("weighted", (B, NC, ld), accumulate, float(out), float(outr), float(acc),
              float(accr), rel(lse, lser))
        assert loss_close(out, outr) and loss_close(acc, accr)
        assert rel(lse, lser) < 1e-4


def check_autograd(dev, B=7, NC=1000, ld=1024):
    """``Fn.cross_entropy(logit_bias=)`` with smoothing and an aux head, forward and backward,
    against ``F.cross_entropy(x.float() + bias, label_smoothing=0.1)`` on the CPU."""
    from mpi_pytorch_amd.ops import functional as Fn
    g = gen(96)
    dt = torch.bfloat16 if dev.type == "cuda" else torch.float32
    mains = [(torch.randn(B, NC, generator=g) * 3 + 2).to(torch.bfloat16) for _ in range(2)]
    labels = torch.randint(0, NC, (B,), generator=g)
    b32 = zipf_log_prior(NC, g).float()
    bias = nan_padded(b32, ld, dev)
    fulls = []
    for v in mains:
        f_ = torch.full((B, ld), lh.SENTINEL, dtype=dt)
        f_[:, :NC] = v.to(dt)
        fulls.append(f_.to(dev).requires_grad_(True))
    lg, aux = fulls[0][:, :NC], fulls[1][:, :NC]
    loss = Fn.cross_entropy(lg, labels.to(dev), label_smoothing=0.1, heads=[(aux, 0.4)],
                            logit_bias=bias)
    loss.backward()
    want_in = [v.float().requires_grad_(True) for v in mains]
    want = F.cross_entropy(want_in[0] + b32, labels, label_smoothing=0.1) + \
        0.4 * F.cross_entropy(want_in[1] + b32, labels, label_smoothing=0.1)
    want.backward()
    plain = F.cross_entropy(mains[0].float(), labels, label_smoothing=0.1) + \
        0.4 * F.cross_entropy(mains[1].float(), labels, label_smoothing=0.1)
    assert not loss_close(plain, want)
    assert loss_close(loss, want), (float(loss), float(want))
    # (without autograd: the same number)
    with torch.no_grad():
        again = Fn.cross_entropy(lg, labels.to(dev), label_smoothing=0.1, heads=[(aux, 0.4)],
                                 logit_bias=bias)
    assert torch.equal(again, loss.detach())
    for f_, w in zip(fulls, want_in):
        gr = f_.grad.cpu()
        print("autograd", rel(gr[:, :NC], w.grad))
        assert rel(gr[:, :NC], w.grad) < 2e-2
        assert float(gr[:, NC:].float().abs().max()) == 0.0


# ------------------------------------------------------------------------ argmax_stats
def run_stats(impl, logits, labels, stats=None, count=None):
    NC = logits.shape[1]
    dev = logits.device
    if stats is None:
        stats = torch.zeros(3, NC, dtype=torch.int64, device=dev)
    if count is None:
        count = torch.zeros(1, dtype=torch.int64, device=dev)
    impl.argmax_stats(logits, labels, count, stats)
    return count, stats


def check_stats_vs_ref(impl, dev, B, NC, ld):
    """Random and tie-heavy logits, every valid value below the pad sentinel; one label is -1
    and one is NC.  count is ``argmax_correct``'s; the sentinel is never predicted."""
    g = gen(97)
    for kind in ("random", "ties"):
        if kind == "random":
            vals = torch.randn(B, NC, generator=g) * 3
        else:
            vals = torch.randint(0, 3, (B, NC), generator=g).float()
        logits = padded(vals.to(dev), ld)
        pred = vals.to(torch.bfloat16).float().argmax(1)
        labels = torch.where(torch.rand(B, generator=g) < 0.5, pred,
                             torch.randint(0, NC, (B,), generator=g))
        labels[0], labels[1] = -1, NC
        labels = labels.to(dev)
        count, stats = run_stats(impl, logits, labels)
        countr, statsr = run_stats(ref, logits, labels)
        am = torch.zeros(1, dtype=torch.int64, device=dev)
        impl.argmax_correct(logits, labels, am)
        print("stats", (B, NC, ld), kind, int(count), int(countr), int(am),
              stats.sum(1).tolist())
        assert torch.equal(stats, statsr) and int(count) == int(countr) == int(am)
        assert stats.sum(1).tolist() == [B - 2, B - 2, int(count)]


def check_stats_contention(impl, dev, B=300, NC=33, ld=64):
    """Every label and every prediction one class: 3 x 300 atomics on three words."""
    vals = torch.zeros(B, NC)
    vals[:, 7] = 5.0
    logits = padded(vals.to(dev), ld)
    labels = torch.full((B,), 7, dtype=torch.int64, device=dev)
    count, stats = run_stats(impl, logits, labels)
    want = torch.zeros(3, NC, dtype=torch.int64)
    want[:, 7] = B
    assert int(count) == B and torch.equal(stats.cpu(), want)
    # two calls add up
    run_stats(impl, logits, labels, stats, count)
    assert int(count) == 2 * B and torch.equal(stats.cpu(), 2 * want)


def check_stats_rules(impl, dev):
    """Ties go to the lower index; an all-NaN row has a support and no prediction; labels -1
    and NC touch nothing; a NaN beside finite values is skipped."""
    NC = 40
    for ld in (40, 41, 48):
        vals = torch.full((6, NC), 1.5)
        vals[1, 9] = 2.0
        vals[1, 30] = 2.0          # a tie of two maxima: 9
        vals[2] = float("nan")     # no prediction
        vals[3, 0] = float("nan")  # skipped: the first finite maximum is 1
        logits = padded(vals.to(dev), ld)
        labels = torch.tensor([0, 30, 5, 1, -1, NC], device=dev)
        count, stats = run_stats(impl, logits, labels)
        want = torch.zeros(3, NC, dtype=torch.int64)
        for lab in (0, 30, 5, 1):
            want[0, lab] += 1
        for p in (0, 9, 1):
            want[1, p] += 1
        for t in (0, 1):
            want[2, t] += 1
        assert int(count) == 2 and torch.equal(stats.cpu(), want), (ld, stats.cpu().nonzero())
        if impl is not ref:  # (the oracle's argmax_correct is torch.argmax: NaN wins there)
            am = torch.zeros(1, dtype=torch.int64, device=dev)
            impl.argmax_correct(logits, labels, am)
            assert int(am) == 2


def check_stats_window(impl, dev, B=7, NC=33, ld=64):
    """stats and count as windows of larger sentinel buffers: the neighbours stay."""
    g = gen(98)
    logits = padded((torch.randn(B, NC, generator=g) * 3).to(dev), ld)
    labels = torch.randint(0, NC, (B,), generator=g).to(dev)
    big = torch.full((5, NC), -7, dtype=torch.int64, device=dev)
    big[1:4] = 0
    cbuf = torch.full((3,), -7, dtype=torch.int64, device=dev)
    cbuf[1] = 0
    impl.argmax_stats(logits, labels, cbuf[1:2], big[1:4])
    countr, statsr = run_stats(ref, logits, labels)
    assert torch.equal(big[1:4], statsr) and int(cbuf[1]) == int(countr)
    assert bool((big[0] == -7).all()) and bool((big[4] == -7).all())
    assert cbuf[0] == -7 and cbuf[2] == -7


def check_macro_scores(dev):
    """``metrics.macro_scores`` against a float64 loop over a hand-made 5-class confusion:
    class 3 is never a label but is predicted, class 4 is a label and never predicted, class
    2 does not occur at all."""
    from mpi_pytorch_amd.metrics import macro_scores
    conf = [[5, 1, 0, 2, 0],   # rows: label, columns: prediction
            [2, 3, 0, 0, 0],
            [0, 0, 0, 0, 0],
            [0, 0, 0, 0, 0],
            [1, 2, 0, 1, 0]]
    support = [sum(r) for r in conf]
    predicted = [sum(conf[r][c] for r in range(5)) for c in range(5)]
    tp = [conf[c][c] for c in range(5)]
    f1s, recalls = [], []
    for c in range(5):
        if support[c] + predicted[c] > 0:
            f1s.append(2.0 * tp[c] / (support[c] + predicted[c]))
        if support[c] > 0:
            recalls.append(tp[c] / support[c])
    assert len(f1s) == 4 and len(recalls) == 3
    stats = torch.tensor([support, predicted, tp], dtype=torch.int64, device=dev)
    got = macro_scores(stats)
    assert abs(got["macro_f1"] - sum(f1s) / len(f1s)) < 1e-12
    assert abs(got["balanced_acc"] - sum(recalls) / len(recalls)) < 1e-12
    assert got["classes_seen"] == 3
    empty = macro_scores(torch.zeros(3, 5, dtype=torch.int64, device=dev))
    assert empty == {"macro_f1": 0.0, "balanced_acc": 0.0, "classes_seen": 0}


# ---------------------------------------------------------------------------- GPU runs
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("shape", SHAPES)
def test_adjusted_ce_matches_oracle(gpu, shape, eps, mixed):
    check_adjusted_random(C(), gpu, *shape, eps, mixed)


@pytest.mark.parametrize("shape", SHAPES)
def test_adjusted_ce_constant_bias(gpu, shape):
    check_constant_bias(C(), gpu, *shape)


@pytest.mark.parametrize("shape", SHAPES)
def test_adjusted_ce_null_and_zero_bias_are_bitwise_plain(gpu, shape):
    check_null_and_zero_bias(C(), gpu, *shape)


@pytest.mark.parametrize("shape", SHAPES)
def test_adjusted_ce_flat_logits_closed_forms(gpu, shape):
    check_flat_logits(C(), gpu, *shape)


@pytest.mark.parametrize("shape", [(300, 33, 64), (7, 1000, 1024), (7, 1004, 1004)])
def test_adjusted_ce_fwd_weighted(gpu, shape):
    check_adjusted_weighted(C(), gpu, *shape)


def test_adjusted_cross_entropy_autograd(gpu):
    check_autograd(gpu)


def test_bad_bias_is_rejected(gpu):
    logits = padded(torch.zeros(2, 16, device=gpu), 16)
    labels = torch.zeros(2, dtype=torch.int64, device=gpu)
    lse = torch.zeros(2, device=gpu)
    go = torch.ones(1, device=gpu)
    out = torch.zeros(1, device=gpu)
    bads = [torch.zeros(16, dtype=torch.float64, device=gpu),   # wrong dtype
            torch.zeros(16, dtype=torch.bfloat16, device=gpu),
            torch.zeros(15, device=gpu),                        # numel < NC
            torch.zeros(16),                                    # on another device
            torch.zeros(32, device=gpu)[::2]]                   # not contiguous
    for bad in bads:
        with pytest.raises(RuntimeError):
            C().ce_fwd(logits, labels, 0.0, None, None, bad)
        with pytest.raises(RuntimeError):
            C().ce_bwd(logits, labels, lse, go, 1.0, 0.0, None, None, bad)
        with pytest.raises(RuntimeError):
            C().ce_fwd_weighted(logits, labels, out, out, 1.0, False, 0.0, None, None, bad)
    C().ce_fwd(logits, labels, 0.0, None, None, torch.zeros(16, device=gpu))  # (a good one)


@pytest.mark.parametrize("shape", SHAPES)
def test_argmax_stats_matches_oracle_and_argmax_correct(gpu, shape):
    check_stats_vs_ref(C(), gpu, *shape)


def test_argmax_stats_contention_rules_and_window(gpu):
    check_stats_contention(C(), gpu)
    check_stats_rules(C(), gpu)
    check_stats_window(C(), gpu)


def test_argmax_stats_rejects_bad_arguments(gpu):
    logits = padded(torch.zeros(2, 16, device=gpu), 16)
    labels = torch.zeros(2, dtype=torch.int64, device=gpu)
    count = torch.zeros(1, dtype=torch.int64, device=gpu)
    good = torch.zeros(3, 16, dtype=torch.int64, device=gpu)
    bads = [(labels, count, torch.zeros(3, 16, dtype=torch.int32, device=gpu)),
            (labels, count, torch.zeros(3, 15, dtype=torch.int64, device=gpu)),
            (labels, count, torch.zeros(2, 16, dtype=torch.int64, device=gpu)),
            (labels, count, torch.zeros(3, 32, dtype=torch.int64, device=gpu)[:, ::2]),
            (labels, count, torch.zeros(3, 16, dtype=torch.int64)),
            (labels, torch.zeros(1, dtype=torch.int32, device=gpu), good),
            (labels[:1], count, good)]
    for lab, cnt, st in bads:
        with pytest.raises(RuntimeError):
            C().argmax_stats(logits, lab, cnt, st)
    C().argmax_stats(logits, labels, count, good)
    assert int(count) == 2 and int(good[0, 0]) == 2


def test_count_class_stats_and_macro_scores_on_the_device(gpu):
    from mpi_pytorch_amd.ops import functional as Fn
    from mpi_pytorch_amd.metrics import macro_scores
    check_macro_scores(gpu)
    g = gen(99)
    vals = torch.randn(64, 33, generator=g) * 3
    logits = padded(vals.to(gpu), 64)
    labels = torch.randint(0, 33, (64,), generator=g)
    count = torch.zeros(1, dtype=torch.int64, device=gpu)
    stats = torch.zeros(3, 33, dtype=torch.int64, device=gpu)
    Fn.count_class_stats(logits, labels.to(gpu), count, stats)
    countr, statsr = run_stats(ref, padded(vals, 64), labels)
    assert torch.equal(stats.cpu(), statsr) and int(count) == int(countr)
    assert macro_scores(stats) == macro_scores(statsr)


# -------------------------------------------------------------------------- end to end
NCLS = lh.NCLS  # 40: the head is stored padded to 64
det = lh.det    # (the deterministic-mode fixture)


def step_bias(dev=None):
    from mpi_pytorch_amd.data.longtail import logit_bias
    counts = [max(1, 400 // (c + 1)) for c in range(NCLS)]
    labels = [c for c, n in enumerate(counts) for _ in range(n)]
    return logit_bias(labels, NCLS, 1.0, dev)


def _train(gpu, **kw):
    from mpi_pytorch_amd.engine import build_training
    from mpi_pytorch_amd.parallel import World
    torch.manual_seed(0)  # one snapshot: every build starts from the same parameters
    return build_training("resnet18", NCLS, gpu, World(device=gpu), 1e-3, **kw)[:3]


def _one_step(gpu, x, y, **kw):
    model, opt, step = _train(gpu, **kw)
    seen = []
    hook = model.register_forward_hook(lambda m, i, o: seen.append(o.detach().clone()))
    loss = step(x, y).clone()
    torch.cuda.synchronize()
    hook.remove()
    return loss, model._mpa_arena.master.clone(), seen[0]


def test_adjusted_step_repeats_and_tau0_is_the_plain_step(det):
    gpu = det
    x, y = lh._batch(gpu)
    bias = step_bias(gpu)
    la, pa, xa = _one_step(gpu, x, y, logit_bias=bias)
    lb, pb, _ = _one_step(gpu, x, y, logit_bias=bias)
    l0, p0, x0 = _one_step(gpu, x, y, logit_bias=None)  # what tau = 0 builds
    lp, pp, _ = _one_step(gpu, x, y)                    # a build without the option
    assert torch.equal(la, lb) and torch.equal(pa, pb)
    assert torch.equal(l0, lp) and torch.equal(p0, pp)
    assert torch.equal(xa, x0) and xa.shape == (8, NCLS)
    assert not torch.equal(la, l0) and not torch.equal(pa, p0)
    want = float(F.cross_entropy(xa.float() + bias[:NCLS], y))
    print("adjusted step", float(la), want, float(l0))
    assert abs(float(la) - want) <= 1e-3 * max(1.0, abs(want))


def test_adjusted_step_graph_replays_bitwise_equal_eager(det):
    gpu = det
    x, y = lh._batch(gpu)
    bias = step_bias(gpu)
    model, opt, step = _train(gpu, logit_bias=bias)
    want = torch.stack([step(x, y).clone() for _ in range(3)])
    torch.cuda.synchronize()
    want_master = model._mpa_arena.master.clone()
    del model, opt, step
    model, opt, step = _train(gpu, logit_bias=bias)
    assert step.capture(x, y, warmup=2)
    got = torch.stack([step(x, y).clone() for _ in range(3)])
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert torch.equal(model._mpa_arena.master, want_master)

