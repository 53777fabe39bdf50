"""GradJoin's rule table (``ops/functional.py``): every ordered combination of contribution
kinds gives the plain sum, leaves nothing parked, and launches exactly what the table in
GradJoin's docstring says.  On the CPU (fp32, ``ops.ref``) and on the native kernels."""
import itertools
import math

import pytest
import torch

from mpi_pytorch_amd.ops import functional as Fn
from mpi_pytorch_amd.ops import ref

# kind -> (R, stride, pad) of a conv dgrad; the other kinds are computed gradients
DGRADS = {"c3s1": (3, 1, 1), "c3s2": (3, 2, 1), "c1s2": (1, 2, 0)}
KINDS = list(DGRADS) + ["tensor", "masked"]
FULL = {"c3s1": True, "c3s2": True, "c1s2": False}  # taps on every pixel of dx


class Recorder:
    """A kernel namespace that logs (name, contribution index of the first argument,
    accumulates?, returned None?) of every call it passes through."""

    def __init__(self, mod):
        self._mod = mod
        self.log = []
        self.owner = {}

    def __getattr__(self, name):
        f = getattr(self._mod, name)

        def call(*args, **kwargs):
            out = f(*args, **kwargs)
            accum = name == "conv_dgrad" and len(args) > 9 and args[9] is not None
            self.log.append((name, self.owner.get(id(args[0])), accum, out is None))
            return out
        return call


def _make(kind, i, k, hw, C, Kout, dev, dtype):
    """Contribution ``i`` of a sequence: (what goes into the join, its fp32 value)."""
    from mpi_pytorch_amd.models.layers import Conv2d
    H, W = hw
    g = torch.Generator().manual_seed(100 + i)

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).to(dtype).to(dev)

    if kind in DGRADS:
        R, s, p = DGRADS[kind]
        Ko = Kout[s]
        P = (H + 2 * p - R) // s + 1
        dz = rnd(2, P, P, Ko)
        w = rnd(Ko, R, R, C, scale=1.0 / math.sqrt(R * R * Ko))
        wt = None
        if dev.type == "cuda":  # the transposed copy the arena keeps beside a bf16 weight
            wt = w.permute(3, 1, 2, 0).reshape(C, R * R, Ko).contiguous()
        val = ref.conv_dgrad(dz.float(), w.float(), H, W, s, s, p, p)
        k.owner[id(dz)] = i
        return Fn._Dgrad(k, dz, w, wt, Conv2d(C, Ko, R, s, p, bias=False), hw), val
    t = rnd(2, H, W, C)
    if kind == "tensor":
        return t, t.float().clone()
    mask = ref.relu_bitmask(rnd(2, H, W, C))
    return Fn._MaskedRes(t, mask), t.float() * ref.bitmask_unpack(mask, t.shape)


def _expected(kinds, pair_on):
    """The table: per newcomer, [(fused attempt or None, launches without / after it)]."""
    steps = []
    part, pi = kinds[0], 0  # the pending first arrival, then "tensor"
    for i, c in enumerate(kinds[1:], 1):
        fused = None
        if c in DGRADS and part in DGRADS:
            if pair_on and FULL[c] != FULL[part] and DGRADS[c][1] == DGRADS[part][1]:
                fused = ("conv_dgrad_pair", i if FULL[c] else pi)
            fresh, acc = (i, pi) if (FULL[c] or not FULL[part]) else (pi, i)
            rest = [("conv_dgrad", fresh, False), ("conv_dgrad", acc, True)]
        elif c in DGRADS:
            if part == "masked" and DGRADS[c][1] == 1:
                fused = ("conv_dgrad_res", i)
            rest = [("conv_dgrad", i, True)]
        elif part in DGRADS:
            rest = [("conv_dgrad", pi, True)]
        else:
            rest = [("add_bf16_", None, False)]
        steps.append((fused, rest))
        part = "tensor"
    return steps


def _check_calls(log, steps, what):
    """Each fused form is tried once; the other launches follow only if it returned None."""
    log = list(log)
    for fused, rest in steps:
        if fused is not None:
            assert log and log[0][:2] == fused, (what, log)
            if not log.pop(0)[3]:
                continue
        n = len(rest)
        assert [e[:3] for e in log[:n]] == rest, (what, log)
        del log[:n]
    assert not log, (what, log)


def _run(kinds, mod, hw, C, Kout, dev, dtype):
    k = Recorder(mod)
    made = [_make(kind, i, k, hw, C, Kout, dev, dtype) for i, kind in enumerate(kinds)]
    exp = sum(v for _c, v in made)  # (before the join: it accumulates in place)
    j = Fn.GradJoin(len(kinds))
    outs = [j.add(k, c) for c, _v in made]
    assert all(o is None for o in outs[:-1]), kinds
    assert j.partial is None and j.arrived == len(kinds), kinds
    return outs[-1], exp, k.log


@pytest.mark.parametrize("pair_on", [True, False])
@pytest.mark.parametrize("n", [2, 3])
def test_join_table_cpu(monkeypatch, n, pair_on):
    """Every ordered pair / triple of {3x3/s1, 3x3/s2, 1x1/s2 dgrad, tensor, masked shortcut}
    into a 2x10x10x8 input (the 1x1/s2 has tap-less phases)."""
    monkeypatch.setattr(Fn, "_PAIR", pair_on)
    cpu = torch.device("cpu")
    for kinds in itertools.product(KINDS, repeat=n):
        out, exp, log = _run(kinds, ref, (10, 10), 8, {1: 16, 2: 16}, cpu, torch.float32)
        assert torch.allclose(out, exp, rtol=1e-4, atol=1e-4), kinds
        steps = _expected(kinds, pair_on)
        _check_calls(log, steps, kinds)
        # on the CPU every fused form that is tried applies
        assert not any(e[3] for e in log if e[0] != "add_bf16_"), (kinds, log)


def test_join_table_examples():
    """The table above, spelled out for the cases the models rely on."""
    assert _expected(("masked", "c3s1"), True) == [
        (("conv_dgrad_res", 1), [("conv_dgrad", 1, True)])]
    for kinds, full in ((("c3s2", "c1s2"), 0), (("c1s2", "c3s2"), 1)):
        assert _expected(kinds, True)[0][0] == ("conv_dgrad_pair", full)
        assert _expected(kinds, False) == [
            (None, [("conv_dgrad", full, False), ("conv_dgrad", 1 - full, True)])]
    assert _expected(("c1s2", "tensor"), True) == [(None, [("conv_dgrad", 0, True)])]
    assert _expected(("c3s1", "c1s2"), True)[0][0] is None  # strides differ: no merged launch


@pytest.mark.gpu
@pytest.mark.parametrize("pair_on", [True, False])
@pytest.mark.parametrize("hw", [8, 14])
def test_join_table_gpu(gpu, monkeypatch, hw, pair_on):
    """Every ordered pair on the native kernels (bf16, transposed weights): batch 2, C = 64,
    K = 64 (stride 1) / 128 (stride 2), against the fp32 oracle sum of the same inputs at
    the bound of test_conv_dgrad_accumulate.  At 8x8 ``conv_dgrad_res`` may decline the
    shape (its fallback then runs); 14x14 is the smallest image of
    test_conv_dgrad_masked_residual / test_conv_dgrad_pair, where both fused forms apply."""
    from mpi_pytorch_amd.ops import _ext
    C = _ext.ext()
    monkeypatch.setattr(Fn, "_PAIR", pair_on)
    halo = C.igemm_halo_enabled()
    C.igemm_set_halo(1)  # (conv_dgrad_res is the halo kernel's epilogue)
    try:
        for kinds in itertools.product(KINDS, repeat=2):
            out, exp, log = _run(kinds, C, (hw, hw), 64, {1: 64, 2: 128}, gpu, torch.bfloat16)
            torch.cuda.synchronize()
            err = float((out.float() - exp).abs().max() / (exp.abs().max() + 1e-6))
            print(kinds, "rel %.2e" % err, [(e[0], e[3]) for e in log])
            assert err < 2e-2, (kinds, err)
            _check_calls(log, _expected(kinds, pair_on), kinds)
            if hw == 14:
                assert not any(e[3] for e in log if e[0] != "add_bf16_"), (kinds, log)
    finally:
        C.igemm_set_halo(1 if halo else 0)
