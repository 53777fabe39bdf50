"""Fused attention and the ViT token kernels (csrc/kernels/attn.hip) against float64, one
encoder block against the fp32 CPU path, and a bitwise-repeatable ViT training step.

The checks take the implementation as an argument: ``tests/test_vit_cpu.py`` runs them with
``ref`` on the CPU, which shows that the reference alone meets them."""
import math

import pytest
import torch

import test_depthwise_gpu as dg

U = 2.0 ** -24   # fp32 unit roundoff
R = 2.0 ** -8    # bf16 unit roundoff
BF = torch.bfloat16

# (B, H, S): a single token; exactly one MFMA tile; one row and one key past a tile; exactly one
# key tile; a second key tile with one valid key (online rescale plus tail mask); ViT-B's shape
# (head stride); ten key tiles
CASES = [(1, 1, 1), (2, 3, 16), (1, 2, 17), (2, 2, 64), (1, 1, 65), (2, 12, 197), (1, 2, 577)]
UNIFORM_CASES = [c for c in CASES if c[2] in (1, 16, 64)]
# (B, Np, D): one patch; ViT-B; five vectors per row (no divisor of a 256-thread block)
TOKEN_CASES = [(2, 1, 8), (2, 196, 768), (3, 7, 40)]
PATCH_CASES = [(1, 16, 16, 8, 16), (2, 32, 48, 8, 16), (3, 8, 12, 2, 4)]


def _d(t):
    return t.double().cpu()


def _ints(shape, lo, hi, gen):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


def _pack(q, k, v, dev):
    """[B, H, S, 64] q, k, v -> the packed [B, S, 3, H, 64] bf16 buffer"""
    return torch.stack([q, k, v]).permute(1, 3, 0, 2, 4).contiguous().to(BF).to(dev)


def _unpack(t):
    return _d(t).permute(2, 0, 3, 1, 4)  # [3][B, H, S, 64]


def _heads(t, H):
    B, S = t.shape[:2]
    return _d(t).reshape(B, S, H, 64).permute(0, 2, 1, 3)


def check_lookup(k, dev, B, H, S):
    """Keys are a seeded +-1 code, q_i = 16 k_pi(i): the winning score is 128 and every other
    one at least 40 lower, so P is 1 on the match and <= e^-40 elsewhere: o is v[pi] bit for
    bit (the other terms vanish in the fp32 sums and the bf16 rounding), lse is 128."""
    gen = torch.Generator().manual_seed(7)
    key = _ints((B, H, S, 64), 0, 1, gen) * 2 - 1
    pi = torch.stack([torch.randperm(S, generator=gen) for _ in range(B * H)]).reshape(B, H, S)
    q = 16 * torch.gather(key, 2, pi[..., None].expand(-1, -1, -1, 64))
    v = torch.randn(B, H, S, 64, generator=gen).to(BF).float()
    s = (q.double() @ key.double().transpose(-1, -2)) / 8
    win = torch.gather(s, 3, pi[..., None])
    rest = s.scatter(3, pi[..., None], -math.inf).amax(-1, keepdim=True) if S > 1 else win - 40
    assert float((win - rest).min()) >= 40
    o, lse = k.attn_fwd(_pack(q, key, v, dev))
    want = torch.gather(v, 2, pi[..., None].expand(-1, -1, -1, 64))
    assert torch.equal(_heads(o, H), want.double())
    assert torch.allclose(_d(lse), torch.logsumexp(s, -1), rtol=2.0 ** -20, atol=0)


def check_uniform(k, dev, B, H, S):
    """All K rows equal, S a power of two, small integers: every P is 1 / S, so o is the exact
    mean of V and dV_j = (1 / S) sum_i dO_i bit for bit; with all V rows equal as well dP = delta
    and dq = dk = 0 exactly."""
    gen = torch.Generator().manual_seed(S)
    q = _ints((B, H, S, 64), -2, 2, gen)
    key = _ints((B, H, 1, 64), -2, 2, gen).expand(B, H, S, 64)
    do = _ints((B, S, H * 64), -3, 3, gen).to(BF).to(dev)
    for equal_v in (False, True):
        v = _ints((B, H, 1 if equal_v else S, 64), -3, 3, gen).expand(B, H, S, 64)
        qkv = _pack(q, key, v, dev)
        o, lse = k.attn_fwd(qkv)
        assert torch.equal(_heads(o, H), v.double().mean(2, keepdim=True).expand(B, H, S, 64))
        dq, dk, dv = _unpack(k.attn_bwd(do, qkv, o, lse))
        assert torch.equal(dv, (_heads(do, H).sum(2, keepdim=True) / S).expand(B, H, S, 64))
        if equal_v:
            assert not bool(dq.any()) and not bool(dk.any())


def check_rounding(k, dev, B, H, S):
    """Random normals (bf16, exactly representable) against float64.  The kernels round:
    a score is a 64-term fp32 chain, scaled by 1/8 (exact), minus the maximum or lse (1), through
    exp (<= 2 ulp with its argument): relative error cp u of every P with cp = 66 A + 4, A the
    largest sum_d |q_d| |k_d| / 8 (an error e of the argument is a relative error e of exp).
    Forward: that error enters the numerator and the row sum (2 cp); every key tile rescales
    the accumulator and the sum (one exp of a difference, one product: 3 T, T = ceil(S / 64));
    numerator and sum are S-term fp32 accumulations (2 S); one division and the lse sum (2):
        c1 = 2 cp + 3 T + 2 S + 2.
    P is rounded to bf16 as the MFMA operand (2^-8 on each term), o once more:
        |o - o64| <= 2^-8 |o64| + (2^-8 + c1 u) sum_j P64 |V|.
    The backward takes o and lse as given inputs (P64 = exp(s64 - lse), delta64 = sum dO o), so
    dV has the same chain (cp + S + 2 <= c1):
        |dV - dV64| <= 2^-8 |dV64| + (2^-8 + c1 u) sum_i P64 |dO|.
    dS = P (dP - delta) is rounded to bf16 once (2^-8); the second 2^-8 is the form's allowance.
    dP and delta are 64-term chains on the magnitudes G = sum_d |dO| |V| and sum_d |dO| |o|:
    their 66 u (G + D) is carried as c2 on (|dP64| + |delta64|) with Gm = max (G + D), which
    holds wherever |dP64| + |delta64| >= 1 / 64 and is 50 times below the 2^-8 terms elsewhere:
        c2 = cp + 66 * 64 Gm / 64 + S + 4 = cp + 66 Gm + S + 4,
        |dQ - dQ64| <= 2^-8 |dQ64| + (2 2^-8 + c2 u) 1/8 sum_j P64 (|dP64| + |delta64|) |K|,
    and the same for dK, summed over i with |Q|."""
    gen = torch.Generator().manual_seed(B * 1000 + H * 100 + S)
    q, key, v = (torch.randn(B, H, S, 64, generator=gen).to(BF).float() for _ in range(3))
    do = torch.randn(B, S, H * 64, generator=gen).to(BF).to(dev)
    qkv = _pack(q, key, v, dev)
    q, key, v = q.double(), key.double(), v.double()
    T = (S + 63) // 64
    cp = 66 * float((q.abs() @ key.abs().transpose(-1, -2)).max()) / 8 + 4
    c1 = 2 * cp + 3 * T + 2 * S + 2
    s = (q @ key.transpose(-1, -2)) / 8
    p = torch.softmax(s, -1)
    o64 = p @ v
    o, lse = k.attn_fwd(qkv)
    assert bool(((_heads(o, H) - o64).abs() <= R * o64.abs() + (R + c1 * U) * (p @ v.abs())).all())
    assert torch.allclose(_d(lse), torch.logsumexp(s, -1), rtol=0, atol=(c1 + 2) * U * (1 + s.abs().max()))
    # backward, o and lse as given
    d64, og = _heads(do, H), _heads(o, H)
    p = torch.exp(s - _d(lse)[..., None])
    dp = d64 @ v.transpose(-1, -2)
    delta = (d64 * og).sum(-1, keepdim=True)
    ds = p * (dp - delta)
    gm = float(((d64.abs() @ v.abs().transpose(-1, -2)) + (d64.abs() * og.abs()).sum(-1, keepdim=True)).max())
    c2 = cp + 66 * gm + S + 4
    mag = p * (dp.abs() + delta.abs())
    dq, dk, dv = _unpack(k.attn_bwd(do, qkv, o, lse))
    dv64 = p.transpose(-1, -2) @ d64
    assert bool(((dv - dv64).abs() <= R * dv64.abs() + (R + c1 * U) * (p.transpose(-1, -2) @ d64.abs())).all())
    dq64, dk64 = ds @ key / 8, ds.transpose(-1, -2) @ q / 8
    assert bool(((dq - dq64).abs() <= R * dq64.abs() + (2 * R + c2 * U) * (mag @ key.abs()) / 8).all())
    assert bool(((dk - dk64).abs() <= R * dk64.abs() + (2 * R + c2 * U) * (mag.transpose(-1, -2) @ q.abs()) / 8).all())


def check_attn_refusals(k, dev):
    bad = [torch.zeros(1, 4, 3, 2, 32, dtype=BF),                      # head dim 32
           torch.zeros(1, 0, 3, 2, 64, dtype=BF),                      # S == 0
           torch.zeros(1, 4, 3, 2, 64, dtype=torch.float64),           # dtype
           torch.zeros(1, 4, 2, 3, 64, dtype=BF).transpose(2, 3)]      # not contiguous
    for t in bad:
        with pytest.raises((RuntimeError, ValueError)):
            k.attn_fwd(t.to(dev))
    with pytest.raises((RuntimeError, ValueError)):  # last dimension is not 3 * H * 64
        k.attn_fwd(torch.zeros(1, 4, 200, dtype=BF, device=dev), 1)


def check_patchify(k, dev, B, Hi, Wi, C, P):
    gen = torch.Generator().manual_seed(Hi + Wi)
    x = torch.randn(B, Hi, Wi, C, generator=gen).to(BF).to(dev)
    want = x.cpu().reshape(B, Hi // P, P, Wi // P, P, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, P * P * C)
    got = k.patchify(x, P)
    assert got.shape == want.shape and torch.equal(got.cpu(), want)


def check_tokens(k, dev, B, Np, D):
    """Small integers: the sums are exact in any order."""
    gen = torch.Generator().manual_seed(Np + D)
    patch = _ints((B * Np, D), -3, 3, gen).to(BF).to(dev)
    cls, pos = _ints((D,), -3, 3, gen).to(dev), _ints((Np + 1, D), -3, 3, gen).to(dev)
    x = k.tokens_fwd(patch, cls, pos)
    want = torch.cat([_d(cls).expand(B, 1, D), _d(patch).reshape(B, Np, D)], 1) + _d(pos)
    assert x.shape == (B, Np + 1, D) and torch.equal(_d(x), want)
    dx = _ints((B, Np + 1, D), -3, 3, gen).to(BF).to(dev)
    for overwrite in (True, False):
        c0, p0 = _ints((D,), -9, 9, gen), _ints((Np + 1, D), -9, 9, gen)
        dc, dp = c0.clone().to(dev), p0.clone().to(dev)
        if overwrite:
            dc.fill_(float("nan"))
            dp.fill_(float("nan"))
        dpatch = k.tokens_bwd(dx, dc, dp, overwrite)
        assert torch.equal(dpatch.cpu(), dx.cpu()[:, 1:].reshape(B * Np, D))
        keep = 0 if overwrite else 1
        assert torch.equal(_d(dp), _d(dx).sum(0) + keep * p0.double())
        assert torch.equal(_d(dc), _d(dx)[:, 0].sum(0) + keep * c0.double())


pytestmark = pytest.mark.gpu


def C():
    from mpi_pytorch_amd.ops import _ext
    return _ext.ext()


@pytest.mark.parametrize("case", CASES)
def test_attention_lookup_exact(gpu, case):
    check_lookup(C(), gpu, *case)


@pytest.mark.parametrize("case", UNIFORM_CASES)
def test_attention_uniform_exact(gpu, case):
    check_uniform(C(), gpu, *case)


@pytest.mark.parametrize("case", CASES)
def test_attention_against_float64(gpu, case):
    check_rounding(C(), gpu, *case)


def test_attention_refusals(gpu):
    check_attn_refusals(C(), gpu)


@pytest.mark.parametrize("case", PATCH_CASES)
def test_patchify_bitwise(gpu, case):
    check_patchify(C(), gpu, *case)


@pytest.mark.parametrize("case", TOKEN_CASES)
def test_tokens_exact(gpu, case):
    check_tokens(C(), gpu, *case)


def test_encoder_block_parity_with_cpu_fp32(gpu):
    from mpi_pytorch_amd.models.vit import EncoderBlock
    from mpi_pytorch_amd.parallel.arena import ParamArena
    torch.manual_seed(3)
    bc, bg = EncoderBlock(2, 128, 256), EncoderBlock(2, 128, 256)
    for p in bc.parameters():  # away from the zero biases and unit scales of the initialisation
        if p.dim() == 1:
            torch.nn.init.normal_(p, 0.5, 0.5)
    bg.load_state_dict(bc.state_dict())
    bg = bg.to(gpu)
    B, S = 2, 17
    x = torch.randn(B * S, 128).to(BF)
    res = []
    for blk, dev in ((bc, torch.device("cpu")), (bg, gpu)):
        ParamArena(blk, dev)
        xi = (x.float() if dev.type == "cpu" else x.to(dev)).requires_grad_()
        y = blk(xi * 1, B, S)
        torch.manual_seed(4)
        y.backward(torch.randn(y.shape).to(BF).to(dev).to(y.dtype))
        res.append([y.detach(), xi.grad] + [q.grad for q in blk.parameters()])
    names = ["y", "dx"] + [n for n, _ in bc.named_parameters()]
    cos = {n: round(dg._cos(a, b), 4) for n, a, b in zip(names, *res)}
    assert min(cos.values()) >= 0.99, cos


def test_vit_training_step_bitwise(gpu, monkeypatch):
    from mpi_pytorch_amd.engine import build_training
    from mpi_pytorch_amd.models.vit import VisionTransformer
    from mpi_pytorch_amd import models
    from mpi_pytorch_amd.parallel import World
    monkeypatch.setitem(models.ATTN_ARCH, "vit",
                        ("vit_reduced", lambda n: VisionTransformer(64, 16, 2, 2, 128, 256, n), 64))
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(8, 64, 64, 8, generator=g) * (torch.arange(8) < 3)).to(gpu, BF)
    y = torch.randint(0, 10, (8,), generator=g).to(gpu)
    outs = []
    for _ in range(2):
        torch.manual_seed(0)
        model, _opt, step, _ = build_training("vit", 10, gpu, World(device=gpu), 1e-3)
        loss = step(x, y).clone()
        torch.cuda.synchronize()
        outs.append((loss.cpu(), model._mpa_arena.grad.cpu().clone(),
                     model._mpa_arena.master.cpu().clone()))
    assert bool(torch.isfinite(outs[0][0]).all()) and float(outs[0][1].abs().sum()) > 0
    assert all(torch.equal(a, b) for a, b in zip(*outs))
