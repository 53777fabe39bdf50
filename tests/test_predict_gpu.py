"""Top-k predictions with probabilities: ``topk_predict`` (csrc/kernels/loss.hip) and the
evaluation pipeline's prediction arrays.

Every kernel check takes the implementation and the device, so ``test_predict_cpu.py`` runs
the same checks with the oracle (``ops/ref.py``) on the CPU: each bound below is met by the
oracle alone, and a GPU failure is the kernel's.

Rules: the candidates of a row are its columns < NC whose logit is neither NaN nor -inf;
column c outranks d when x[c] > x[d], or x[c] == x[d] and c < d (``topk_correct``'s order);
idx[r, j] is the candidate that exactly j candidates outrank, prob[r, j] = exp(x[idx] -
logsumexp(x[r])); slots past the last candidate hold idx = -1, prob = 0.

The probability bound is the cross-entropy loss bound of ``test_loss_head_gpu.py``, 1e-3 *
max(1, |ref|), on log prob: a log-probability is a row loss with the sign flipped.  Padded
inputs carry the finite sentinel 1000.0 in their pad columns, so a kernel that reads them into
the ranking or the log-sum-exp fails visibly."""
import numpy as np
import pytest
import torch

from mpi_pytorch_amd.ops import ref
from test_loss_head_gpu import SHAPES, SENTINEL, padded, distinct_rows

pytestmark = pytest.mark.gpu

KS = [1, 5, 16]
IDX_FILL, PROB_FILL = -77, -5.0  # what an unwritten output element holds


def C():
    from mpi_pytorch_amd.ops import _ext
    return _ext.ext()


def outputs(B, k, dev):
    return (torch.full((B, k), IDX_FILL, dtype=torch.int32, device=dev),
            torch.full((B, k), PROB_FILL, dtype=torch.float32, device=dev))


def predict(impl, logits, k):
    idx, prob = outputs(logits.shape[0], k, logits.device)
    impl.topk_predict(logits, k, idx, prob)
    return idx, prob


def logprob_err(prob, want):
    """max over the slots with want > 0 of |log prob - log want| / max(1, |log want|)."""
    on = want > 0
    if not bool(on.any()):
        return 0.0
    lw = want[on].double().log()
    lp = prob[on].double().clamp_min(1e-300).log()
    return float(((lp - lw).abs() / lw.abs().clamp_min(1.0)).max())


# ------------------------------------------------------------------------ kernel checks
def check_vs_oracle(impl, dev, B, NC, ld, k):
    """Check 1: tie-heavy random logits against the oracle."""
    torch.manual_seed(70)
    logits = padded(torch.randn(B, NC, device=dev) * 3, ld)
    idx, prob = predict(impl, logits, k)
    idxr, probr = predict(ref, logits, k)
    err = logprob_err(prob, probr)
    print("oracle", (B, NC, ld), k, err, float(prob.sum(1).max()))
    assert torch.equal(idx, idxr)
    assert bool((idx[:, :min(k, NC)] >= 0).all()) and bool((idx < NC).all())
    assert bool((idx[:, NC:] == -1).all()) and bool((prob[:, NC:] == 0).all())
    assert err <= 1e-3
    assert bool((prob >= 0).all()) and bool((prob <= 1).all())
    assert bool((prob[:, 1:] <= prob[:, :-1]).all())
    assert float(prob.sum(1).max()) <= 1 + 1e-3


def check_tie_free(impl, dev, B, NC, ld, ks=(1, 5)):
    """Check 2: rows of distinct values (the whole bf16 range) against torch.topk."""
    torch.manual_seed(72)
    vals = distinct_rows(B, NC, dev)
    logits = padded(vals, ld)
    for k in ks:
        assert k < NC
        idx, prob = predict(impl, logits, k)
        assert torch.equal(idx.long(), vals.float().topk(k, 1).indices)
        assert bool(torch.isfinite(prob).all())
        assert bool((prob >= 0).all()) and bool((prob <= 1).all())


def check_vs_counting(impl, dev, B, NC, ld, k):
    """Check 3: the indices reproduce argmax_correct's and topk_correct's counts."""
    torch.manual_seed(70)
    logits = padded(torch.randn(B, NC, device=dev) * 3, ld)
    labels = torch.randint(0, NC, (B,), device=dev)
    labels[0], labels[1] = -1, NC
    idx, _prob = predict(impl, logits, k)
    top1 = torch.zeros(1, dtype=torch.int64, device=dev)
    topk = torch.zeros(1, dtype=torch.int64, device=dev)
    impl.argmax_correct(logits, labels, top1)
    impl.topk_correct(logits, labels, k, topk)
    assert int((idx[:, 0] == labels).sum()) == int(top1)
    assert int((idx == labels[:, None]).any(1).sum()) == int(topk)


def check_tie_rule(impl, dev):
    """Check 4: an all-equal row block; the pad sentinel reaches neither output."""
    for ld in (40, 41, 48):  # 16-byte path unpadded, scalar path, 16-byte path padded
        logits = padded(torch.full((8, 40), 1.5, device=dev), ld)
        for k in KS:
            idx, prob = predict(impl, logits, k)
            assert torch.equal(idx, torch.arange(k, dtype=torch.int32, device=dev).expand(8, k))
            err = logprob_err(prob, torch.full_like(prob, 1.0 / 40))
            assert err <= 1e-3, (ld, k, err)


def nan_block(dev):
    torch.manual_seed(74)
    vals = torch.randn(6, 40, device=dev) * 3
    ninf = float("-inf")
    vals[0] = float("nan")
    vals[1] = ninf
    vals[2] = ninf
    cols = torch.tensor([31, 2, 17, 8, 39], device=dev)
    vals[2, cols] = torch.tensor([0.5, 2.0, 2.0, -1.0, 0.5], device=dev)
    vals[3, 11] = float("nan")
    vals[4, 0] = ninf  # (and one -inf inside an otherwise finite row)
    return vals


def check_nan_inf_short(impl, dev, ld=48, small_ld=8):
    """Check 5: NaN, -inf and short rows, [6, 40] at ``ld`` and k = 8; NC = 5 < k at
    ``small_ld``.  (48, 8): the issue's case, the 16-byte path; (41, 7): the scalar path."""
    vals = nan_block(dev)
    logits = padded(vals, ld)
    idx, prob = predict(impl, logits, 8)
    idxr, probr = predict(ref, logits, 8)
    empty_i = torch.full((8,), -1, dtype=torch.int32, device=dev)
    for r in (0, 1):  # all NaN, all -inf: no candidate
        assert torch.equal(idx[r], empty_i) and bool((prob[r] == 0).all())
    assert idx[2].tolist() == [2, 17, 31, 39, 8, -1, -1, -1]
    assert bool((prob[2, 5:] == 0).all()) and bool((prob[2, :5] > 0).all())
    # one NaN elsewhere: the indices as if that column were absent
    gone = logits[3].float()  # (the bf16 values: rounding makes ties)
    gone[11] = float("-inf")
    assert torch.equal(idx[3].long(), torch.sort(gone, descending=True, stable=True).indices[:8])
    assert torch.equal(idx, idxr)
    finite = [2, 4, 5]  # (rows without a NaN: the probabilities are specified)
    assert logprob_err(prob[finite], probr[finite]) <= 1e-3
    assert int(idx[4, 7]) >= 0 and 0 not in idx[4].tolist()
    # argmax_stats' predicted-class counters on the same logits
    labels = torch.zeros(6, dtype=torch.int64, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    stats = torch.zeros(3, 40, dtype=torch.int64, device=dev)
    impl.argmax_stats(logits, labels, count, stats)
    first = idx[:, 0].long()
    assert torch.equal(stats[1], torch.bincount(first[first >= 0], minlength=40))
    # NC < k
    torch.manual_seed(75)
    small = padded(torch.randn(3, 5, device=dev) * 3, small_ld)
    idx, prob = predict(impl, small, 8)
    idxr, probr = predict(ref, small, 8)
    assert torch.equal(idx, idxr) and bool((idx[:, 5:] == -1).all())
    assert bool((prob[:, 5:] == 0).all()) and logprob_err(prob, probr) <= 1e-3
    assert torch.equal(idx[:, :5].long(), torch.sort(small.float(), dim=1, descending=True,
                                                     stable=True).indices)


def check_windows(impl, dev):
    """Check 6: outputs are rows [1, 1 + B) of sentinel-filled buffers; the logits are a
    window of a larger sentinel buffer at an offset that keeps (24 elements) or breaks (3) the
    16-byte alignment."""
    B, NC, ld, k = 5, 33, 64, 5
    torch.manual_seed(76)
    vals = (torch.randn(B, NC, device=dev) * 3).to(torch.bfloat16)
    want_i, want_p = predict(ref, vals, k)
    for off in (24, 3):
        big = torch.full((off + (B + 1) * ld,), SENTINEL, dtype=torch.bfloat16, device=dev)
        win = big.as_strided((B, NC), (ld, 1), off)
        win.copy_(vals)
        ibuf, pbuf = outputs(B + 2, k, dev)
        impl.topk_predict(win, k, ibuf[1:1 + B], pbuf[1:1 + B])
        assert torch.equal(ibuf[1:1 + B], want_i)
        assert logprob_err(pbuf[1:1 + B], want_p) <= 1e-3
        for edge in (0, B + 1):
            assert bool((ibuf[edge] == IDX_FILL).all()) and bool((pbuf[edge] == PROB_FILL).all())


def check_rows_independent(impl, dev, B, NC, ld, k=5, rows=None):
    """Check 7: two calls are bitwise equal, and a row alone gives the batch's bits."""
    torch.manual_seed(77)
    logits = padded(torch.randn(B, NC, device=dev) * 3, ld)
    idx, prob = predict(impl, logits, k)
    idx2, prob2 = predict(impl, logits, k)
    assert torch.equal(idx, idx2) and torch.equal(prob, prob2)
    for r in (range(B) if rows is None else rows):
        i1, p1 = predict(impl, logits[r:r + 1], k)
        assert torch.equal(i1[0], idx[r]) and torch.equal(p1[0], prob[r]), r


def check_refusals(impl, dev, error):
    """Check 8: bad arguments raise before anything is written."""
    B, k = 4, 5
    logits = padded(torch.zeros(B, 40, device=dev), 48)
    idx, prob = outputs(B, k, dev)
    wide_i, wide_p = outputs(B, k + 1, dev)
    cases = [
        (0, idx, prob), (17, idx, prob),
        (k, idx.long(), prob),                    # int64 idx
        (k, idx, wide_p[:, :k]),                  # non-contiguous prob
        (k, wide_i, prob), (k, idx, wide_p),      # [B, k + 1]
    ]
    for kk, i, p in cases:
        keep_i, keep_p = i.clone(), p.clone()
        with pytest.raises(error):
            impl.topk_predict(logits, kk, i, p)
        assert torch.equal(i, keep_i) and torch.equal(p, keep_p)
    assert bool((wide_i == IDX_FILL).all()) and bool((wide_p == PROB_FILL).all())
    impl.topk_predict(logits, k, idx, prob)  # (and the good call does write)
    assert bool((idx >= 0).all())


# ---------------------------------------------------------------------------- GPU runs
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("shape", SHAPES)
def test_topk_predict_matches_oracle(gpu, shape, k):
    check_vs_oracle(C(), gpu, *shape, k)


@pytest.mark.parametrize("shape", SHAPES)
def test_topk_predict_tie_free_rows(gpu, shape):
    check_tie_free(C(), gpu, *shape)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("shape", SHAPES)
def test_topk_predict_reproduces_the_counting_kernels(gpu, shape, k):
    check_vs_counting(C(), gpu, *shape, k)


def test_topk_predict_tie_rule_nan_inf_and_short_rows(gpu):
    check_tie_rule(C(), gpu)
    check_nan_inf_short(C(), gpu)
    check_nan_inf_short(C(), gpu, 41, 7)


def test_topk_predict_windows(gpu):
    check_windows(C(), gpu)


def test_topk_predict_rows_are_independent(gpu):
    check_rows_independent(C(), gpu, 300, 33, 64)
    check_rows_independent(C(), gpu, 4, 64500, 64512)


def test_topk_predict_rejects_bad_arguments(gpu):
    check_refusals(C(), gpu, RuntimeError)
    with pytest.raises(RuntimeError):  # logits that logits_ld refuses
        C().topk_predict(torch.zeros(4, 40, device=gpu), 1, *outputs(4, 1, gpu))


def test_predict_topk_op_allocates_and_dispatches(gpu):
    from mpi_pytorch_amd.ops import functional as Fn
    torch.manual_seed(78)
    logits = padded(torch.randn(7, 1000, device=gpu) * 3, 1024)
    idx, prob = Fn.predict_topk(logits, 5)
    assert idx.dtype == torch.int32 and prob.dtype == torch.float32
    assert idx.shape == prob.shape == (7, 5) and idx.device == logits.device
    want = predict(C(), logits, 5)
    assert torch.equal(idx, want[0]) and torch.equal(prob, want[1])
    into = outputs(7, 5, gpu)
    got = Fn.predict_topk(logits, 5, *into)
    assert got[0] is into[0] and got[1] is into[1] and torch.equal(into[0], idx)


# ---------------------------------------------------------------------------- pipeline
NCLS = 10


@pytest.fixture
def det(gpu):
    k = C()
    old = k.deterministic()
    k.set_deterministic(1)
    yield gpu
    k.set_deterministic(int(old))


@pytest.fixture(scope="module")
def model(gpu):
    from mpi_pytorch_amd.engine import build_training
    from mpi_pytorch_amd.parallel import World
    torch.manual_seed(0)
    m, _opt, _step, _ = build_training("resnet18", NCLS, gpu, World(device=gpu), 1e-3)
    m.eval()
    return m


def _manifest(n, seed=0):
    names = ["synthetic/%05d.jpg" % i for i in range(n)]
    return names, list(np.random.default_rng(seed).integers(0, NCLS, size=n))


@pytest.fixture(scope="module")
def plain(gpu, model):
    """The non-pipelined predictions and count of the 203-image manifest (computed once,
    under the deterministic mode the pipeline runs use)."""
    from mpi_pytorch_amd.data.manifest import SyntheticImages
    from mpi_pytorch_amd.engine.eval_pipeline import plain_eval, plain_predict
    k = C()
    old = k.deterministic()
    k.set_deterministic(1)
    try:
        names, labels = _manifest(203)
        src = SyntheticImages((96, 80))
        idx, prob = plain_predict(model, names, 16, src, gpu, (64, 64), 5)
        return idx, prob, plain_eval(model, names, labels, 16, src, gpu, (64, 64))
    finally:
        k.set_deterministic(int(old))


@pytest.mark.parametrize("lanes,assign", [(1, "random"), (3, "random"), (3, "roundrobin")])
def test_ring_pipeline_predictions_equal_plain_predict(det, model, plain, lanes, assign):
    from mpi_pytorch_amd.data.manifest import SyntheticImages
    from mpi_pytorch_amd.engine.eval_pipeline import StreamPipeline, make_ring
    gpu = det
    names, labels = _manifest(203)  # a short last batch
    ring, nb = make_ring(names, labels, 16, SyntheticImages((96, 80)), NCLS, depth=4, threads=3)
    try:
        pipe = StreamPipeline(model, gpu, (64, 64), lanes=lanes, assign=assign, predict_k=5)
        counts = pipe.run_ring(ring, nb, rows=len(names))
    finally:
        ring.stop()
    idx, prob = pipe.predictions()
    want_i, want_p, want_count = plain
    assert idx.shape == prob.shape == (203, 5)
    assert idx.dtype == np.int32 and prob.dtype == np.float32
    assert np.array_equal(idx, want_i) and np.array_equal(prob, want_p)
    assert sum(counts) == want_count > 0
    assert int((idx[:, 0] == np.asarray(labels)).sum()) == sum(counts)
    assert (idx >= 0).all() and (idx < NCLS).all() and (prob > 0).all()


def test_host_batches_pipeline_predictions(det, model, plain):
    from mpi_pytorch_amd.data.manifest import SyntheticImages
    from mpi_pytorch_amd.engine.eval_pipeline import StreamPipeline, _batches
    gpu = det
    names, labels = _manifest(203)
    pipe = StreamPipeline(model, gpu, (64, 64), lanes=2, assign="roundrobin", predict_k=5)
    counts = pipe.run(_batches(names, labels, 16, SyntheticImages((96, 80))), rows=len(names))
    idx, prob = pipe.predictions()
    assert np.array_equal(idx, plain[0]) and np.array_equal(prob, plain[1])
    assert sum(counts) == plain[2]


def test_pipeline_without_predict_k_allocates_nothing(det, model, plain):
    from mpi_pytorch_amd.data.manifest import SyntheticImages
    from mpi_pytorch_amd.engine.eval_pipeline import StreamPipeline, make_ring
    gpu = det
    names, labels = _manifest(203)
    ring, nb = make_ring(names, labels, 16, SyntheticImages((96, 80)), NCLS, depth=4, threads=3)
    try:
        pipe = StreamPipeline(model, gpu, (64, 64), lanes=2)
        counts = pipe.run_ring(ring, nb)
    finally:
        ring.stop()
    assert pipe.predictions() is None and pipe.pred_idx is None and pipe.pred_prob is None
    assert sum(counts) == plain[2]
    with pytest.raises(ValueError):
        StreamPipeline(model, gpu, (64, 64), predict_k=17)
