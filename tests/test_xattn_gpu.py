"""Short-key cross-attention (csrc/kernels/xattn.hip) and the pre-bias GELU (ln.hip) against
float64, one spatial-reduction block against the fp32 CPU path, and a bitwise-repeatable PVT
training step.

The checks take the implementation as an argument: ``tests/test_pvt_cpu.py`` runs them with
``ref`` on the CPU, which shows that the reference alone meets them."""
import math

import pytest
import torch

import test_depthwise_gpu as dg
from test_attention_gpu import BF, R, U, _d, _heads, _ints

# xattn_plan_check prints "B 64 H 4 Sq 129: tiles 3 tpw 2 walks 2": the smallest geometry whose
# plan has two tiles in a walk, two slab rows per (batch, head) and a short last walk
PLAN_CASE = (64, 4, 129, 49)
# (B, H, Sq, Sk): one query, one key; exactly one MFMA tile; one row past a wave and 15 masked
# keys; a full key tile and exactly one query tile; a second query tile with one valid row and a
# key count just past the 32-column half of at_pos; PVT's stage 3 with an odd head count
CASES = [(1, 1, 1, 1), (2, 3, 16, 16), (1, 2, 17, 49), (2, 2, 64, 64), (1, 1, 65, 33), (2, 5, 196, 49),
         PLAN_CASE]
UNIFORM_CASES = [c for c in CASES if c[3] in (1, 16, 64)]
GELU_CASES = [(1, 8), (1003, 24), (37, 136)]


def _pack(q, key, v, dev):
    """[B, H, S, 64] q and k, v -> q [B, Sq, H 64] and kv [B, Sk, 2 H 64] bf16"""
    B, H, Sq, _ = q.shape
    qq = q.permute(0, 2, 1, 3).reshape(B, Sq, H * 64)
    kv = torch.stack([key, v]).permute(1, 3, 0, 2, 4).reshape(B, key.shape[2], 2 * H * 64)
    return qq.contiguous().to(BF).to(dev), kv.contiguous().to(BF).to(dev)


def _unpack_kv(t, H):
    B, Sk = t.shape[:2]
    return _d(t).reshape(B, Sk, 2, H, 64).permute(2, 0, 3, 1, 4)  # [2][B, H, Sk, 64]


def check_lookup(k, dev, B, H, Sq, Sk):
    """Keys are a seeded +-1 code, q_i = 16 k_pi(i) (pi maps queries to keys): the winning score
    is 128 and every other one at least 40 lower, so o is v[pi] bit for bit and lse is 128."""
    gen = torch.Generator().manual_seed(7)
    key = _ints((B, H, Sk, 64), 0, 1, gen) * 2 - 1
    pi = torch.randint(0, Sk, (B, H, Sq), generator=gen)
    q = 16 * torch.gather(key, 2, pi[..., None].expand(-1, -1, -1, 64))
    v = torch.randn(B, H, Sk, 64, generator=gen).to(BF).float()
    s = (q.double() @ key.double().transpose(-1, -2)) / 8
    win = torch.gather(s, 3, pi[..., None])
    rest = s.scatter(3, pi[..., None], -math.inf).amax(-1, keepdim=True) if Sk > 1 else win - 40
    assert float((win - rest).min()) >= 40
    o, lse = k.xattn_fwd(*_pack(q, key, v, dev), H)
    want = torch.gather(v, 2, pi[..., None].expand(-1, -1, -1, 64))
    assert torch.equal(_heads(o, H), want.double())
    assert torch.allclose(_d(lse), torch.logsumexp(s, -1), rtol=2.0 ** -20, atol=0)


def check_uniform(k, dev, B, H, Sq, Sk):
    """All K rows equal, Sk a power of two, small integers: every P is 1 / Sk, so o is the exact
    mean of V and dV_j = (1 / Sk) sum_i dO_i bit for bit (|dO| <= 3: the Sq-term sums stay below
    2^8, exact in fp32 and in bf16); with all V rows equal as well dP = delta and dq = dk = 0."""
    gen = torch.Generator().manual_seed(Sq + Sk)
    q = _ints((B, H, Sq, 64), -2, 2, gen)
    key = _ints((B, H, 1, 64), -2, 2, gen).expand(B, H, Sk, 64)
    do = _ints((B, Sq, H * 64), -3, 3, gen).to(BF).to(dev)
    assert 3 * Sq <= 256 and 3 * Sk <= 256
    for equal_v in (False, True):
        v = _ints((B, H, 1 if equal_v else Sk, 64), -3, 3, gen).expand(B, H, Sk, 64)
        qq, kv = _pack(q, key, v, dev)
        o, lse = k.xattn_fwd(qq, kv, H)
        assert torch.equal(_heads(o, H), v.double().mean(2, keepdim=True).expand(B, H, Sq, 64))
        dq, dkv = k.xattn_bwd(do, qq, kv, o, lse, H)
        dk, dv = _unpack_kv(dkv, H)
        assert torch.equal(dv, (_heads(do, H).sum(2, keepdim=True) / Sk).expand(B, H, Sk, 64))
        if equal_v:
            assert not bool(_d(dq).any()) and not bool(dk.any())


def check_rounding(k, dev, B, H, Sq, Sk):
    """Random normals (bf16, exactly representable) against float64: ``check_rounding`` of
    test_attention_gpu.py re-derived for one resident key tile.  cp = 66 A + 4 is the relative
    error (in u) of every P, A the largest sum_d |q_d| |k_d| / 8.
    Forward: cp enters the numerator and the row sum (2 cp); there is one key tile, so no
    rescale term; numerator and sum are Sk-term fp32 accumulations (2 Sk); one division and the
    lse sum (2):  c1 = 2 cp + 2 Sk + 2,
        |o - o64| <= 2^-8 |o64| + (2^-8 + c1 u) sum_j P64 |V|.
    Backward, o and lse as given.  dQ is complete in one block, as there with S = Sk:
        c2 = cp + 66 Gm + Sk + 4,
        |dQ - dQ64| <= 2^-8 |dQ64| + (2 2^-8 + c2 u) 1/8 sum_j P64 (|dP64| + |delta64|) |K|.
    dK and dV sum over the Sq queries in two levels, fp32 both: the MFMA accumulation of a walk,
    then the slab rows (at most T = ceil(Sq / 64) of them), so the accumulation constant is
    Sq + T; P and dS are rounded to bf16 once as operands (2^-8 per term; dS's second 2^-8 is the
    form's allowance as there) and the summed slab to bf16 once (the 2^-8 on the result):
        cv = cp + Sq + T + 2,          |dV - dV64| <= 2^-8 |dV64| + (2^-8 + cv u) sum_i P64 |dO|,
        ck = cp + 66 Gm + Sq + T + 4,  |dK - dK64| <= 2^-8 |dK64| + (2 2^-8 + ck u) 1/8 sum_i mag |Q|."""
    gen = torch.Generator().manual_seed(B * 1000 + H * 100 + Sq + Sk)
    q = torch.randn(B, H, Sq, 64, generator=gen).to(BF).float()
    key, v = (torch.randn(B, H, Sk, 64, generator=gen).to(BF).float() for _ in range(2))
    do = torch.randn(B, Sq, H * 64, generator=gen).to(BF).to(dev)
    qq, kv = _pack(q, key, v, dev)
    q, key, v = q.double(), key.double(), v.double()
    T = (Sq + 63) // 64
    cp = 66 * float((q.abs() @ key.abs().transpose(-1, -2)).max()) / 8 + 4
    c1 = 2 * cp + 2 * Sk + 2
    s = (q @ key.transpose(-1, -2)) / 8
    p = torch.softmax(s, -1)
    o64 = p @ v
    o, lse = k.xattn_fwd(qq, kv, H)
    assert bool(((_heads(o, H) - o64).abs() <= R * o64.abs() + (R + c1 * U) * (p @ v.abs())).all())
    assert torch.allclose(_d(lse), torch.logsumexp(s, -1), rtol=0, atol=(c1 + 2) * U * (1 + s.abs().max()))
    # backward, o and lse as given
    d64, og = _heads(do, H), _heads(o, H)
    p = torch.exp(s - _d(lse)[..., None])
    dp = d64 @ v.transpose(-1, -2)
    delta = (d64 * og).sum(-1, keepdim=True)
    ds = p * (dp - delta)
    gm = float(((d64.abs() @ v.abs().transpose(-1, -2)) + (d64.abs() * og.abs()).sum(-1, keepdim=True)).max())
    c2, cv, ck = cp + 66 * gm + Sk + 4, cp + Sq + T + 2, cp + 66 * gm + Sq + T + 4
    mag = p * (dp.abs() + delta.abs())
    dq, dkv = k.xattn_bwd(do, qq, kv, o, lse, H)
    dq, (dk, dv) = _heads(dq, H), _unpack_kv(dkv, H)
    dv64 = p.transpose(-1, -2) @ d64
    assert bool(((dv - dv64).abs() <= R * dv64.abs() + (R + cv * U) * (p.transpose(-1, -2) @ d64.abs())).all())
    dq64, dk64 = ds @ key / 8, ds.transpose(-1, -2) @ q / 8
    assert bool(((dq - dq64).abs() <= R * dq64.abs() + (2 * R + c2 * U) * (mag @ key.abs()) / 8).all())
    assert bool(((dk - dk64).abs() <= R * dk64.abs() + (2 * R + ck * U) * (mag.transpose(-1, -2) @ q.abs()) / 8).all())


def check_repeatable(k, dev, B, H, Sq, Sk):
    gen = torch.Generator().manual_seed(5)
    q, kv, do = (torch.randn(B, n, w * H * 64, generator=gen).to(BF).to(dev)
                 for n, w in ((Sq, 1), (Sk, 2), (Sq, 1)))
    o, lse = k.xattn_fwd(q, kv, H)
    a, b = k.xattn_bwd(do, q, kv, o, lse, H), k.xattn_bwd(do, q, kv, o, lse, H)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and bool(_d(a[1]).any())


def check_xattn_refusals(k, dev):
    z = lambda *s: torch.zeros(*s, dtype=BF, device=dev)
    with pytest.raises((RuntimeError, ValueError), match="64"):  # Sk > 64 says so
        k.xattn_fwd(z(1, 4, 64), z(1, 65, 128), 1)
    for q, kv, H in ((z(1, 4, 64), z(1, 0, 128), 1), (z(1, 4, 32), z(1, 4, 64), 1),
                     (z(2, 4, 64), z(1, 4, 128), 1), (z(1, 4, 128), z(1, 4, 128), 2)):
        with pytest.raises((RuntimeError, ValueError)):
            k.xattn_fwd(q, kv, H)


def check_gelu_pre_bias(k, dev, M, C):
    """gelu(h + b) and its backward against float64: ``check_gelu``'s bound of test_ln_gpu.py on
    t = h + b, plus the one fp32 rounding of the sum, u |t|, carried through |gelu'| <= 1.13 (and
    through |da gelu''| <= |da| for dh: |gelu''| <= 2 phi(0) < 1).  dbias is an fp32 sum of the M
    stored dh of a column: (M - 1) u sum |dh| in any order.  Without the bias: gelu_fwd(h) itself."""
    E = 2.0 ** -22
    torch.manual_seed(M + C)
    h, da = (torch.randn(M, C) * 2).to(BF).to(dev), torch.randn(M, C).to(BF).to(dev)
    b = torch.randn(C).to(dev)
    t, da64 = _d(h) + _d(b), _d(da)
    cdf = 0.5 * (1 + torch.erf(t / math.sqrt(2)))
    pdf = torch.exp(-0.5 * t * t) / math.sqrt(2 * math.pi)
    a64, der = t * cdf, cdf + t * pdf
    a = _d(k.gelu_fwd(h, b))
    assert bool(((a - a64).abs() <= R * a64.abs() + t.abs() * E / 2 + 4 * U * a64.abs() + 1.13 * U * t.abs()).all())
    db = torch.zeros(C, device=dev)
    dh = _d(k.gelu_bwd(da, h, db, b))
    fp32 = da64.abs() * (E / 2 + U * (4 * cdf + (t * t / 2 + 6) * (t * pdf).abs()) + U * t.abs())
    assert bool(((dh - da64 * der).abs() <= R * (da64 * der).abs() + fp32).all())
    assert bool(((_d(db) - dh.sum(0)).abs() <= M * U * dh.abs().sum(0)).all())
    assert torch.equal(k.gelu_fwd(h, None), k.gelu_fwd(h)) and not torch.equal(k.gelu_fwd(h), k.gelu_fwd(h, b))


pytestmark = pytest.mark.gpu


def C():
    from mpi_pytorch_amd.ops import _ext
    return _ext.ext()


@pytest.mark.parametrize("case", CASES)
def test_cross_attention_lookup_exact(gpu, case):
    check_lookup(C(), gpu, *case)


@pytest.mark.parametrize("case", UNIFORM_CASES)
def test_cross_attention_uniform_exact(gpu, case):
    check_uniform(C(), gpu, *case)


@pytest.mark.parametrize("case", CASES)
def test_cross_attention_against_float64(gpu, case):
    check_rounding(C(), gpu, *case)


def test_cross_attention_backward_repeats_bitwise_across_slab_rows(gpu):
    B, H, Sq, Sk = PLAN_CASE
    tpw, walks, ws_floats = C().xattn_plan(B, H, Sq, Sk)
    tiles = (Sq + 63) // 64
    assert tpw >= 2 and walks >= 2 and tiles % tpw and ws_floats == walks * B * H * 64 * 128
    check_repeatable(C(), gpu, *PLAN_CASE)


def test_cross_attention_refusals(gpu):
    check_xattn_refusals(C(), gpu)


@pytest.mark.parametrize("case", GELU_CASES)
def test_gelu_pre_bias_against_float64(gpu, case):
    check_gelu_pre_bias(C(), gpu, *case)


def test_sra_block_parity_with_cpu_fp32(gpu):
    from mpi_pytorch_amd.models.pvt import PVTBlock
    from mpi_pytorch_amd.parallel.arena import ParamArena
    torch.manual_seed(3)
    bc, bg = PVTBlock(128, 2, 4, 2), PVTBlock(128, 2, 4, 2)
    for p in bc.parameters():  # away from the zero biases and unit scales of the initialisation
        if p.dim() == 1:
            torch.nn.init.normal_(p, 0.5, 0.5)
    bg.load_state_dict(bc.state_dict())
    bg = bg.to(gpu)
    x = torch.randn(2, 8, 8, 128).to(BF)
    res = []
    for blk, dev in ((bc, torch.device("cpu")), (bg, gpu)):
        ParamArena(blk, dev)
        xi = (x.float() if dev.type == "cpu" else x.to(dev)).requires_grad_()
        y = blk(xi * 1)
        torch.manual_seed(4)
        y.backward(torch.randn(y.shape).to(BF).to(dev).to(y.dtype))
        res.append([y.detach(), xi.grad] + [q.grad for q in blk.parameters()])
    names = ["y", "dx"] + [n for n, _ in bc.named_parameters()]
    cos = {n: round(dg._cos(a, b), 4) for n, a, b in zip(names, *res)}
    assert min(cos.values()) >= 0.99, cos


def test_pvt_training_step_bitwise(gpu, monkeypatch):
    from mpi_pytorch_amd.engine import build_training
    from mpi_pytorch_amd.models.pvt import PyramidVisionTransformerV2
    from mpi_pytorch_amd import models
    from mpi_pytorch_amd.parallel import World
    monkeypatch.setitem(models.PYRAMID_ARCH, "pvt_v2", (
        "pvt_reduced", lambda n: PyramidVisionTransformerV2(depths=(1, 1, 1, 1), num_classes=n), 64))
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(8, 64, 64, 8, generator=g) * (torch.arange(8) < 3)).to(gpu, BF)
    y = torch.randint(0, 10, (8,), generator=g).to(gpu)
    outs = []
    for _ in range(2):
        torch.manual_seed(0)
        model, _opt, step, _ = build_training("pvt_v2", 10, gpu, World(device=gpu), 1e-3)
        loss = step(x, y).clone()
        torch.cuda.synchronize()
        outs.append((loss.cpu(), model._mpa_arena.grad.cpu().clone(),
                     model._mpa_arena.master.cpu().clone()))
    assert bool(torch.isfinite(outs[0][0]).all()) and float(outs[0][1].abs().sum()) > 0
    assert all(torch.equal(a, b) for a, b in zip(*outs))
