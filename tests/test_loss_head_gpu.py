"""The loss head (csrc/kernels/loss.hip): label-smoothed cross-entropy and top-k accuracy.

Every check takes the implementation and the device, so ``test_loss_head_cpu.py`` runs the
same checks with the oracle (``ops/ref.py``) on the CPU: each bound below is met by the
oracle alone, and a GPU failure is the kernel's.

Smoothing follows ``torch.nn.functional.cross_entropy(label_smoothing=eps)``:
    loss_row = lse - (1-eps) * x[label] - (eps/NC) * sum_c x[c]
    dx[c]    = (softmax[c] - (1-eps) * [c == label] - eps/NC) * grad_out * weight / B
Top-k counts the rows whose label's rank #{c: x[c] > x[label] or (x[c] == x[label] and
c < label)} is below k (ties to the lower index, argmax's rule).

Bounds are ``test_kernels_gpu.py::test_cross_entropy``'s: loss 1e-3 * max(1, |ref|),
rel(lse) < 1e-4, gradient rel < 2e-2 in the max norm.  Padded inputs carry the finite
sentinel 1000.0 in their pad columns, so a kernel that reads them into the logit sum, the
LSE or the rank fails visibly."""
import math

import pytest
import torch
import torch.nn.functional as F

from mpi_pytorch_amd.ops import ref

pytestmark = pytest.mark.gpu

# (B, NC, ld): the smallest shape that reaches each code path
SHAPES = [
    (5, 33, 33),            # scalar V = 1
    (7, 1004, 1004),        # V = 4
    (5, 33, 64),            # padded; NC ends inside a 16-byte vector
    (7, 1000, 1024),        # padded; whole pad vectors
    (3, 8200, 8224),        # padded; ld/8 = 1028 > 256 * 4: a second loop trip, most lanes idle
    (300, 33, 64),          # B > 256: the loss sum strides rows
    (4, 64500, 64512),      # the production head
]
EPS = [0.1, 1.0]
SENTINEL = 1000.0
GO, WEIGHT = 0.7, 0.4


def C():
    from mpi_pytorch_amd.ops import _ext
    return _ext.ext()


def rel(a, b):
    a = a.float()
    b = b.float()
    return float((a - b).abs().max() / (b.abs().max() + 1e-6))


def padded(vals, ld):
    """[B, NC] values as the ``[:, :NC]`` view of a [B, ld] bf16 buffer whose pad columns hold
    the sentinel."""
    B, NC = vals.shape
    full = torch.full((B, ld), SENTINEL, dtype=torch.bfloat16, device=vals.device)
    full[:, :NC] = vals.to(torch.bfloat16)
    return full[:, :NC] if ld > NC else full


def loss_close(got, want):
    got, want = (float(v.detach()) if torch.is_tensor(v) else v for v in (got, want))
    return abs(float(got) - float(want)) <= 1e-3 * max(1.0, abs(float(want)))


def pad_is_zero(impl, d, ld):
    """The gradient's pad columns (the native op returns a view of a [B, ld] buffer)."""
    B, NC = d.shape
    if impl is ref or ld == NC:
        return True
    assert d.stride(0) == ld
    base = d.as_strided((B, ld), (ld, 1), d.storage_offset())
    return float(base[:, NC:].float().abs().max()) == 0.0


# ----------------------------------------------------------------------- smoothed CE
def check_smoothed_random(impl, dev, B, NC, ld, eps):
    torch.manual_seed(60)
    vals = torch.randn(B, NC, device=dev) * 3 + 2  # nonzero mean: the sum term is visible
    logits = padded(vals, ld)
    assert abs(float(logits.float().mean())) > 1.0
    labels = torch.randint(0, NC, (B,), device=dev)
    loss, lse = impl.ce_fwd(logits, labels, eps)
    lossr, lser = ref.ce_fwd(logits, labels, eps)
    go = torch.full((1,), GO, device=dev)
    d = impl.ce_bwd(logits, labels, lse, go, WEIGHT, eps)
    dr = ref.ce_bwd(logits, labels, lser, go, WEIGHT, eps)
    print("smoothed", (B, NC, ld), eps, float(loss), float(lossr), rel(lse, lser), rel(d, dr))
    assert loss_close(loss, lossr)
    assert rel(lse, lser) < 1e-4
    assert d.shape == (B, NC) and rel(d, dr) < 2e-2
    assert pad_is_zero(impl, d, ld)


def check_smoothed_flat(impl, dev, B, NC, ld, eps):
    """Every valid logit 2.0 (exact in bf16): closed forms, which see a dropped sum or a
    dropped eps/NC term that the max-norm gradient bound cannot."""
    torch.manual_seed(61)
    logits = padded(torch.full((B, NC), 2.0, device=dev), ld)
    labels = torch.randint(0, NC, (B,), device=dev)
    loss, lse = impl.ce_fwd(logits, labels, eps)
    assert loss_close(loss, math.log(NC)), (float(loss), math.log(NC))
    go = torch.full((1,), GO, device=dev)
    d = impl.ce_bwd(logits, labels, lse, go, WEIGHT, eps).float()
    s = GO * WEIGHT
    unit = s / (B * NC)
    other = (1.0 - eps) / NC * s / B
    at_label = (1.0 - eps) * (1.0 / NC - 1.0) * s / B
    is_label = torch.zeros(B, NC, dtype=torch.bool, device=dev)
    is_label[torch.arange(B, device=dev), labels] = True
    err_other = float((d[~is_label] - other).abs().max())
    err_label = float((d[is_label] - at_label).abs().max())
    print("flat", (B, NC, ld), eps, float(loss), err_other, err_label)
    assert err_other <= max(1e-2 * abs(other), 1e-3 * unit), (err_other, other)
    assert err_label <= 1e-2 * abs(at_label) + 1e-3 * unit, (err_label, at_label)
    assert pad_is_zero(impl, impl.ce_bwd(logits, labels, lse, go, WEIGHT, eps), ld)


def check_smoothed_bitwise(impl, dev, B, NC, ld):
    """eps = 1 does not see the label; an explicit eps = 0 is the plain call; a smoothed
    forward repeats bitwise."""
    torch.manual_seed(62)
    logits = padded(torch.randn(B, NC, device=dev) * 3 + 2, ld)
    la = torch.randint(0, NC, (B,), device=dev)
    lb = (la + 1 + torch.randint(0, NC - 1, (B,), device=dev)) % NC
    assert bool((la != lb).all())
    go = torch.full((1,), GO, device=dev)
    (l1, s1), (l2, s2) = impl.ce_fwd(logits, la, 1.0), impl.ce_fwd(logits, lb, 1.0)
    assert torch.equal(l1, l2) and torch.equal(s1, s2)
    assert torch.equal(impl.ce_bwd(logits, la, s1, go, WEIGHT, 1.0),
                       impl.ce_bwd(logits, lb, s2, go, WEIGHT, 1.0))
    (l0, s0), (lp, sp) = impl.ce_fwd(logits, la, 0.0), impl.ce_fwd(logits, la)
    assert torch.equal(l0, lp) and torch.equal(s0, sp)
    assert torch.equal(impl.ce_bwd(logits, la, s0, go, WEIGHT, 0.0),
                       impl.ce_bwd(logits, la, sp, go, WEIGHT))
    (la1, sa1), (la2, sa2) = impl.ce_fwd(logits, la, 0.1), impl.ce_fwd(logits, la, 0.1)
    assert torch.equal(la1, la2) and torch.equal(sa1, sa2)
    assert not torch.equal(la1, lp)  # (and smoothing does change the loss)


def check_smoothed_weighted(impl, dev, B, NC, ld):
    """``check_ce_fwd_weighted`` of test_kernels_gpu.py with eps = 0.1: two heads, assign then
    accumulate with weight 0.4, both into the running acc."""
    torch.manual_seed(63)
    out, acc = torch.full((1,), 123.0, device=dev), torch.full((1,), 5.0, device=dev)
    outr, accr = out.clone(), acc.clone()
    for accumulate in (False, True):
        logits = padded(torch.randn(B, NC, device=dev) * 3 + 2, ld)
        labels = torch.randint(0, NC, (B,), device=dev)
        lse = impl.ce_fwd_weighted(logits, labels, out, acc, 0.4, accumulate, 0.1)
        lser = ref.ce_fwd_weighted(logits, labels, outr, accr, 0.4, accumulate, 0.1)
        print("weighted", (B, NC, ld), accumulate, float(out), float(outr), float(acc),
              float(accr), rel(lse, lser))
        assert loss_close(out, outr) and loss_close(acc, accr)
        assert rel(lse, lser) < 1e-4


def check_autograd(dev, B=7, NC=1000, ld=1024):
    """``Fn.cross_entropy`` with smoothing and an aux head, forward and backward, against
    ``F.cross_entropy(label_smoothing=0.1)`` in fp32 on the CPU from the same bf16 logits."""
    from mpi_pytorch_amd.ops import functional as Fn
    torch.manual_seed(64)
    dt = torch.bfloat16 if dev.type == "cuda" else torch.float32
    mains = [(torch.randn(B, NC) * 3 + 2).to(torch.bfloat16) for _ in range(2)]
    labels = torch.randint(0, NC, (B,))
    fulls = []
    for v in mains:
        f_ = torch.full((B, ld), SENTINEL, dtype=dt)
        f_[:, :NC] = v.to(dt)
        fulls.append(f_.to(dev).requires_grad_(True))
    lg, aux = fulls[0][:, :NC], fulls[1][:, :NC]
    loss = Fn.cross_entropy(lg, labels.to(dev), label_smoothing=0.1, heads=[(aux, 0.4)])
    loss.backward()
    want_in = [v.float().requires_grad_(True) for v in mains]
    want = F.cross_entropy(want_in[0], labels, label_smoothing=0.1) + \
        0.4 * F.cross_entropy(want_in[1], labels, label_smoothing=0.1)
    want.backward()
    assert loss_close(loss, want), (float(loss), float(want))
    for f_, w in zip(fulls, want_in):
        g = f_.grad.cpu()
        print("autograd", rel(g[:, :NC], w.grad))
        assert rel(g[:, :NC], w.grad) < 2e-2
        assert float(g[:, NC:].float().abs().max()) == 0.0


# ------------------------------------------------------------------------------ top-k
def _count(impl, logits, labels, k, start=0):
    cnt = torch.full((1,), start, dtype=torch.int64, device=logits.device)
    impl.topk_correct(logits, labels, k, cnt)
    return int(cnt)


def check_topk_vs_ref(impl, dev, B, NC, ld):
    """Tie-heavy random logits; one label is -1 and one is NC (where the pad sentinel, or the
    next row, sits for an unguarded read)."""
    torch.manual_seed(70)
    logits = padded(torch.randn(B, NC, device=dev) * 3, ld)
    labels = torch.randint(0, NC, (B,), device=dev)
    labels[0], labels[1] = -1, NC
    for k in (1, 5, NC, NC + 3):
        got, want = _count(impl, logits, labels, k), _count(ref, logits, labels, k)
        print("topk", (B, NC, ld), k, got, want)
        assert got == want
        if k >= NC:
            assert got == B - 2


def check_topk_vs_argmax(impl, dev, B, NC, ld):
    """Logits from {0, 1, 2}: ties dominate.  k = 1 counts what argmax_correct counts: the
    first maximum (even rows) and not the second one (odd rows)."""
    torch.manual_seed(71)
    vals = torch.randint(0, 3, (B, NC), device=dev).float()
    logits = padded(vals, ld)
    cols = torch.arange(NC, device=dev).expand(B, NC)
    is_max = vals == vals.max(1, keepdim=True).values
    first = torch.where(is_max, cols, NC).min(1).values
    is_max[torch.arange(B, device=dev), first] = False
    second = torch.where(is_max, cols, NC).min(1).values
    assert int(second.max()) < NC
    labels = torch.where(torch.arange(B, device=dev) % 2 == 0, first, second)
    am = torch.zeros(1, dtype=torch.int64, device=dev)
    impl.argmax_correct(logits, labels, am)
    assert _count(impl, logits, labels, 1) == int(am) == (B + 1) // 2


def distinct_rows(B, NC, dev):
    """Rows of NC distinct finite normal bf16 values (65,024 bit patterns: two signs x 254
    exponents x 128 mantissas)."""
    rows = []
    for _ in range(B):
        p = torch.randperm(65024)[:NC]
        bits = (p // 32512) * 32768 + (p % 32512) + 128
        rows.append((bits - (bits >= 32768) * 65536).to(torch.int16))
    return torch.stack(rows).view(torch.bfloat16).to(dev)


def check_topk_tie_free(impl, dev, B, NC, ld, ks=(1, 5)):
    """No ties: the label sits at sorted position k-1 in even rows (counted) and k in odd
    rows (not counted), so the count is the number of even rows and is torch.topk's."""
    torch.manual_seed(72)
    vals = distinct_rows(B, NC, dev)
    assert bool(torch.isfinite(vals.float()).all())
    logits = padded(vals, ld)
    order = vals.float().argsort(1, descending=True)
    rows = torch.arange(B, device=dev)
    for k in ks:
        assert k < NC
        labels = order[rows, k - 1 + rows % 2]
        want = int((vals.float().topk(k, 1).indices == labels[:, None]).any(1).sum())
        got = _count(impl, logits, labels, k)
        print("tie-free", (B, NC, ld), k, got, want)
        assert got == want == (B + 1) // 2


def check_topk_tie_rule(impl, dev):
    """An all-equal row with label L has rank L."""
    for ld in (40, 41, 48):  # 16-byte path unpadded, scalar path, 16-byte path padded
        logits = padded(torch.full((8, 40), 1.5, device=dev), ld)
        labels = torch.arange(8, device=dev)
        got = [_count(impl, logits, labels, k) for k in (1, 3, 5, 8, 9)]
        assert got == [1, 3, 5, 8, 8], (ld, got)


def check_topk_nan_and_accumulate(impl, dev):
    torch.manual_seed(73)
    for ld in (40, 41, 48):
        vals = torch.randn(4, 40, device=dev) * 3
        labels = torch.tensor([3, 17, 39, 0], device=dev)
        vals[torch.arange(4, device=dev), labels] = 50.0  # every label is its row's maximum
        vals[0, 3] = float("nan")    # NaN at the label: never counted
        vals[1, 20] = float("nan")   # NaN elsewhere: ignored
        vals[1, 5] = 60.0            # ... and the rest decides: one column beats the label
        logits = padded(vals, ld)
        assert _count(impl, logits, labels, 1) == 2
        assert _count(impl, logits, labels, 2) == 3
        assert _count(impl, logits, labels, 43) == 3
        cnt = torch.full((1,), 10, dtype=torch.int64, device=dev)
        impl.topk_correct(logits, labels, 2, cnt)
        impl.topk_correct(logits, labels, 1, cnt)
        assert int(cnt) == 15  # count accumulates across calls


# ---------------------------------------------------------------------------- GPU runs
@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("shape", SHAPES)
def test_smoothed_ce_random(gpu, shape, eps):
    check_smoothed_random(C(), gpu, *shape, eps)


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("shape", SHAPES)
def test_smoothed_ce_flat_closed_forms(gpu, shape, eps):
    check_smoothed_flat(C(), gpu, *shape, eps)


@pytest.mark.parametrize("shape", SHAPES)
def test_smoothed_ce_bitwise_properties(gpu, shape):
    check_smoothed_bitwise(C(), gpu, *shape)


@pytest.mark.parametrize("shape", [(300, 33, 64), (7, 1000, 1024), (7, 1004, 1004)])
def test_smoothed_ce_fwd_weighted(gpu, shape):
    check_smoothed_weighted(C(), gpu, *shape)


def test_smoothing_out_of_range_is_rejected(gpu):
    logits = padded(torch.zeros(2, 8, device=gpu), 8)
    labels = torch.zeros(2, dtype=torch.int64, device=gpu)
    for bad in (-0.1, 1.5):
        with pytest.raises(RuntimeError):
            C().ce_fwd(logits, labels, bad)


def test_smoothed_cross_entropy_autograd(gpu):
    check_autograd(gpu)


@pytest.mark.parametrize("shape", SHAPES)
def test_topk_matches_oracle(gpu, shape):
    check_topk_vs_ref(C(), gpu, *shape)


@pytest.mark.parametrize("shape", SHAPES)
def test_topk_k1_is_argmax_correct(gpu, shape):
    check_topk_vs_argmax(C(), gpu, *shape)


@pytest.mark.parametrize("shape", SHAPES)
def test_topk_tie_free_rows(gpu, shape):
    check_topk_tie_free(C(), gpu, *shape)


def test_topk_tie_rule_nan_and_accumulation(gpu):
    check_topk_tie_rule(C(), gpu)
    check_topk_nan_and_accumulate(C(), gpu)
    cnt = torch.zeros(1, dtype=torch.int64, device=gpu)
    with pytest.raises(RuntimeError):
        C().topk_correct(padded(torch.zeros(2, 8, device=gpu), 8),
                         torch.zeros(2, dtype=torch.int64, device=gpu), 0, cnt)


# -------------------------------------------------------------------------- end to end
NCLS = 40  # the head is stored padded to 64


@pytest.fixture
def det(gpu):
    k = C()
    old = k.deterministic()
    k.set_deterministic(1)
    yield gpu
    k.set_deterministic(int(old))


def _train(gpu, eps):
    from mpi_pytorch_amd.engine import build_training
    from mpi_pytorch_amd.parallel import World
    torch.manual_seed(0)  # one snapshot: every build starts from the same parameters
    return build_training("resnet18", NCLS, gpu, World(device=gpu), 1e-3,
                          label_smoothing=eps)[:3]


def _batch(gpu, B=8, hw=32):
    g = torch.Generator(device="cpu").manual_seed(1)
    x = (torch.randn(B, hw, hw, 8, generator=g) * (torch.arange(8) < 3)).to(gpu, torch.bfloat16)
    y = torch.randint(0, NCLS, (B,), generator=g).to(gpu)
    return x, y


def test_smoothed_step_repeats_and_shifts_the_loss(det):
    gpu = det
    x, y = _batch(gpu)
    runs = []
    for eps in (0.1, 0.1, 0.0):
        model, opt, step = _train(gpu, eps)
        seen = []
        hook = model.register_forward_hook(lambda m, i, o: seen.append(o.detach().clone()))
        loss = step(x, y).clone()
        torch.cuda.synchronize()
        hook.remove()
        runs.append((loss, model._mpa_arena.master.clone(), seen[0]))
        del model, opt, step
    (la, pa, xa), (lb, pb, _), (l0, p0, x0) = runs
    assert torch.equal(la, lb) and torch.equal(pa, pb)
    assert torch.equal(xa, x0) and not torch.equal(pa, p0)
    assert xa.shape == (8, NCLS)
    xf = xa.float()
    picked = xf.gather(1, y.view(-1, 1)).squeeze(1)
    # CE_eps - CE_0 = eps * mean_rows(x[label] - mean_c x[c])
    want = 0.1 * float((picked - xf.mean(1)).mean())
    got = float(la) - float(l0)
    print("loss shift", got, want, float(la), float(l0))
    assert abs(got - want) <= 1e-3 * max(1.0, abs(float(la)))


def test_smoothed_step_graph_replays_bitwise_equal_eager(det):
    gpu = det
    x, y = _batch(gpu)
    model, opt, step = _train(gpu, 0.1)
    want = torch.stack([step(x, y).clone() for _ in range(3)])
    torch.cuda.synchronize()
    want_master = model._mpa_arena.master.clone()
    del model, opt, step
    model, opt, step = _train(gpu, 0.1)
    assert step.capture(x, y, warmup=2)
    got = torch.stack([step(x, y).clone() for _ in range(3)])
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert torch.equal(model._mpa_arena.master, want_master)
