"""Neighbourhood attention (csrc/kernels/nattn.hip) against float64, its locality, its refusals
and a bitwise-repeatable NAT training step.

The checks take the implementation as an argument: ``tests/test_nat_cpu.py`` runs them with
``ref`` on the CPU, which shows that the reference alone meets them."""
import pytest
import torch

import test_attention_gpu as ag
from mpi_pytorch_amd.ops import ref

U, R, BF = ag.U, ag.R, ag.BF
SCALE = 32 ** -0.5
S = 49  # keys of every query

# (B, H, Hf, Wf): the neighbourhood is the whole map; clamping on both ends, a non-square map and
# a partial tile; the widest one-key (13) and two-key (14) query ranges; the 15-wide query range
# and several tiles on an axis; odd sizes with partial tiles on both axes (and the 17-wide range
# of 8 keys at L = 23); a batch walk of 3 images and 11 slab rows
CASES = [(1, 1, 7, 7), (2, 3, 8, 9), (1, 2, 13, 14), (1, 4, 9, 28), (2, 1, 17, 23), (33, 2, 8, 8)]
LOCAL_CASES = [(2, 3, 8, 9), (2, 1, 17, 23)]


def _inputs(case, dev):
    B, H, Hf, Wf = case
    gen = torch.Generator().manual_seed(sum(p * v for p, v in zip((1, 7, 31, 57), case)))
    qkv = torch.randn(B * Hf * Wf, 3 * H * 32, generator=gen).to(BF)
    do = torch.randn(B * Hf * Wf, H * 32, generator=gen).to(BF)
    rpb = torch.randn(H * 169, generator=gen) * 0.5
    return qkv.to(dev), do.to(dev), rpb.to(dev)


def _heads(t, case):
    """[B, H, N, 32] float64 of rows t [B N, H 32]"""
    B, H, Hf, Wf = case
    return ag._d(t).reshape(B, Hf * Wf, H, 32).transpose(1, 2)


def _split(t, case):
    H = case[1]
    return (_heads(t[:, i * H * 32:(i + 1) * H * 32], case) for i in range(3))


def check_against_float64(k_, dev, case):
    """Random bf16 normals, rpb N(0, 0.5), against float64 of the textbook formulation (gather each
    query's 49 keys by the index table, softmax, weighted sum).  The bounds are the forward-error
    forms of test_wattn_gpu.py with S = 49 and this kernel's chains.  A score is a 32-term fp32
    chain (32), times 32^-1/2 as one fp32 constant (its rounding and the product's: 2), plus the
    bias (1), minus the maximum or lse (1), through exp (<= 2 ulp with its argument): relative
    error cp u of every P, cp = 37 A + 4, A the largest sum_d |q_d| |k_d| 32^-1/2 + |rpb|.
    Forward, one pass over S keys (masked slots add exact zeros): the error enters numerator and
    row sum (2 cp), the form's one-tile term (3), two S-term fp32 sums (2 S), the division and the
    lse sum (2):  c1 = 2 cp + 3 + 2 S + 2,
        |o - o64| <= 2^-8 |o64| + (2^-8 + c1 u) sum_j P64 |V|,   and the same for dV with |dO|,
    whose sum runs over the at most 15 x 15 queries that attend a key, S-term sums at a time in
    the MFMA and a chain of at most 7 row pairs (the 2 S term covers 2 * 49 >= 7 + 15 * 15 / 16).
    The backward takes lse as given; delta_i = sum_j P dP is relative to D_i = sum_j P64 |dP64|;
    dP is a 32-term chain on G = sum_d |dO| |V| entering dS directly and through delta (66 Gm u
    P64); P's error enters dS twice (2 cp), delta is an S-term sum (S), the product, the dQ sum (S)
    and the scale (2):  c2 = 2 cp + 2 S + 6,  mag = P64 (|dP64| + D),
        |dQ - dQ64| <= 2^-8 |dQ64| + 32^-1/2 sum_j ((2 2^-8 + c2 u) mag + 66 Gm u P64) |K|
    and the same for dK over the attending queries.  drpb is an fp32 sum of the unrounded dS: a
    walk of at most B images, a fold of at most 64 queries and at most B tiles slab rows, so a
    chain of n = B + 64 + B tiles terms:
        |drpb - drpb64| <= sum ((c2 + n) u mag + 66 Gm u P64)."""
    B, H, Hf, Wf = case
    N = Hf * Wf
    qkv, do, rpb = _inputs(case, dev)
    kidx, bidx = ref.na_tables(Hf, Wf)
    q, k, v = _split(qkv, case)
    kg, vg = k[:, :, kidx], v[:, :, kidx]
    add = ag._d(rpb).reshape(H, 169)[:, bidx].unsqueeze(0)
    dot = lambda w, x: torch.einsum("bhnj,bhnjd->bhnd", w, x)
    gather = lambda w, x: torch.zeros(B, H, N, 32, dtype=torch.float64).index_add_(
        2, kidx.reshape(-1), (w.unsqueeze(-1) * x.unsqueeze(3)).reshape(B, H, N * S, 32))
    cp = 37 * float((torch.einsum("bhnd,bhnjd->bhnj", q.abs(), kg.abs()) * SCALE + add.abs()).max()) + 4
    c1 = 2 * cp + 3 + 2 * S + 2
    s = torch.einsum("bhnd,bhnjd->bhnj", q, kg) * SCALE + add
    p = torch.softmax(s, -1)
    o64 = dot(p, vg)
    o, lse = k_.na_fwd(qkv, rpb, H, Hf, Wf)
    assert o.shape == (B * N, H * 32) and lse.shape == (B, H, N)
    assert bool(((_heads(o, case) - o64).abs() <= R * o64.abs() + (R + c1 * U) * dot(p, vg.abs())).all())
    assert torch.allclose(ag._d(lse), torch.logsumexp(s, -1), rtol=0, atol=(c1 + 2) * U * (1 + float(s.abs().max())))
    # backward, lse as given
    d64 = _heads(do, case)
    p = torch.exp(s - ag._d(lse)[..., None])
    dp = torch.einsum("bhnd,bhnjd->bhnj", d64, vg)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    mag = p * (dp.abs() + (p * dp.abs()).sum(-1, keepdim=True))
    gm = float(torch.einsum("bhnd,bhnjd->bhnj", d64.abs(), vg.abs()).max())
    c2 = 2 * cp + 2 * S + 6
    drpb = torch.full_like(rpb, float("nan"))
    dqkv = k_.na_bwd(do, qkv, lse, rpb, drpb, H, Hf, Wf, True)
    assert dqkv.shape == qkv.shape
    dq, dk, dv = _split(dqkv, case)
    dv64 = gather(p, d64)
    assert bool(((dv - dv64).abs() <= R * dv64.abs() + (R + c1 * U) * gather(p, d64.abs())).all())
    err = (2 * R + c2 * U) * mag + 66 * gm * U * p
    dq64, dk64 = dot(ds, kg) * SCALE, gather(ds, q) * SCALE
    assert bool(((dq - dq64).abs() <= R * dq64.abs() + dot(err, kg.abs()) * SCALE).all())
    assert bool(((dk - dk64).abs() <= R * dk64.abs() + gather(err, q.abs()) * SCALE).all())
    fold = lambda t: torch.zeros(H, 169, dtype=torch.float64).index_add_(1, bidx.reshape(-1), t.sum(0).reshape(H, N * S))
    n = B + 64 + B * ((Hf + 7) // 8) * ((Wf + 7) // 8)
    berr = fold((c2 + n) * U * mag + 66 * gm * U * p)
    assert bool(((ag._d(drpb).reshape(H, 169) - fold(ds)).abs() <= berr).all())
    # accumulate into the sink, and two runs are bitwise equal
    acc = torch.ones_like(rpb)
    dqkv2 = k_.na_bwd(do, qkv, lse, rpb, acc, H, Hf, Wf, False)
    assert torch.equal(dqkv2, dqkv) and torch.equal(acc, 1 + drpb)
    assert all(torch.equal(a, b) for a, b in zip(k_.na_fwd(qkv, rpb, H, Hf, Wf), (o, lse)))


def check_locality(k_, dev, case):
    """New k and v for one pixel (near a corner, so its attending range is clamped) change o at
    exactly the queries whose neighbourhood holds it; do zero outside one query leaves dk and dv
    zero outside that query's 49 keys."""
    B, H, Hf, Wf = case
    N = Hf * Wf
    qkv, do, rpb = _inputs(case, dev)
    kidx = ref.na_tables(Hf, Wf)[0]
    pix = (B - 1) * N + 1 * Wf + (Wf - 2)
    new = qkv.clone()
    new[pix, H * 32:] = (new[pix, H * 32:].float() + 1.0).to(BF)
    o, o2 = (k_.na_fwd(t, rpb, H, Hf, Wf)[0].cpu() for t in (qkv, new))
    hit = torch.zeros(B * N, dtype=torch.bool)
    hit[(B - 1) * N:] = (kidx == pix - (B - 1) * N).any(1)
    assert 16 <= int(hit.sum()) <= 289  # 4 .. 17 attending queries per axis
    assert torch.equal(o2[~hit], o[~hit]) and bool((o2[hit] != o[hit]).any(1).all())
    one = torch.zeros_like(do)
    one[pix] = do[pix]
    lse = k_.na_fwd(qkv, rpb, H, Hf, Wf)[1]
    dkv = k_.na_bwd(one, qkv, lse, rpb, torch.empty_like(rpb), H, Hf, Wf, True)[:, H * 32:].cpu()
    keys = torch.zeros(B * N, dtype=torch.bool)
    keys[(B - 1) * N + kidx[pix - (B - 1) * N]] = True
    assert int(keys.sum()) == 49
    assert not bool(dkv[~keys].any()) and bool((dkv[keys] != 0).any(1).all())


def check_refusals(k_, dev):
    z = lambda *shape, dt=BF: torch.zeros(*shape, dtype=dt, device=dev)
    bad = [(z(42, 96), z(169, dt=torch.float32), 1, 6, 7), (z(42, 96), z(169, dt=torch.float32), 1, 7, 6),
           (z(49, 192), z(169, dt=torch.float32), 1, 7, 7),  # head dim 64
           (z(49, 96), z(225, dt=torch.float32), 1, 7, 7)]   # rpb length
    for qkv, rpb, H, Hf, Wf in bad:
        with pytest.raises((RuntimeError, ValueError)):
            k_.na_fwd(qkv, rpb, H, Hf, Wf)
        with pytest.raises((RuntimeError, ValueError)):
            k_.na_bwd(z(qkv.shape[0], H * 32), qkv, z(1, H, qkv.shape[0], dt=torch.float32), rpb,
                      torch.empty_like(rpb), H, Hf, Wf, True)


pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CASES)
def test_neighborhood_attention_against_float64(gpu, case):
    check_against_float64(ag.C(), gpu, case)


@pytest.mark.parametrize("case", LOCAL_CASES)
def test_neighborhood_attention_locality(gpu, case):
    check_locality(ag.C(), gpu, case)


def test_neighborhood_attention_refusals(gpu):
    check_refusals(ag.C(), gpu)


def test_nat_training_step_bitwise(gpu, monkeypatch):
    from mpi_pytorch_amd.engine import build_training
    from mpi_pytorch_amd.models.nat import NAT
    from mpi_pytorch_amd import models
    from mpi_pytorch_amd.parallel import World
    monkeypatch.setitem(models.NEIGHBORHOOD_ARCH, "nat",
                        ("nat_reduced", lambda n: NAT(64, (2, 1), (2, 4), 3.0, n), 64))
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(8, 64, 64, 8, generator=g) * (torch.arange(8) < 3)).to(gpu, BF)
    y = torch.randint(0, 10, (8,), generator=g).to(gpu)
    outs = []
    for _ in range(2):
        torch.manual_seed(0)
        model, _opt, step, _ = build_training("nat", 10, gpu, World(device=gpu), 1e-3)
        loss = step(x, y).clone()
        torch.cuda.synchronize()
        outs.append((loss.cpu(), model._mpa_arena.grad.cpu().clone(),
                     model._mpa_arena.master.cpu().clone()))
    assert bool(torch.isfinite(outs[0][0]).all()) and float(outs[0][1].abs().sum()) > 0
    assert all(torch.equal(a, b) for a, b in zip(*outs))
