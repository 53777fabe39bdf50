"""Every kernel that has an oracle is called by a GPU test, and the checks those tests apply
are met by the oracle itself.

1. Inventory: for every public function of ``mpi_pytorch_amd/ops/ref.py`` that
   ``csrc/bindings.cpp`` also exports with ``m.def``, the text ``.<name>(`` occurs in some
   ``tests/*_gpu.py``.  (Diagnostics and setters have no ``ref`` twin: out of scope.)
2. The window / small-kernel checks of ``test_kernels_gpu.py`` take the implementation as an
   argument; run here on the CPU with ``ref`` as that implementation, they show that the
   sentinel construction, the neighbour checks and every tolerance formula hold for the
   oracle alone (so a GPU failure is the kernel's)."""
import glob
import os
import re

import pytest
import torch

import test_kernels_gpu as kg
from mpi_pytorch_amd.ops import ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")

# name -> reason why no GPU test calls it.  Keep it empty: write the test instead.
EXEMPT = {}


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as fh:
        return fh.read()


def test_every_kernel_with_an_oracle_is_called_by_a_gpu_test():
    public = re.findall(r"^def ([A-Za-z]\w*)\(", _read("mpi_pytorch_amd", "ops", "ref.py"), re.M)
    exported = set(re.findall(r'm\.def\(\s*"(\w+)"', _read("csrc", "bindings.cpp")))
    twins = [n for n in public if n in exported]
    assert len(twins) > 50  # (the collectors still find the definitions)
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "*_gpu.py")))
    text = "".join(_read(f) for f in files)
    assert not set(EXEMPT) - set(twins), "an exemption names no exported kernel"
    missing = [n for n in twins if "." + n + "(" not in text and n not in EXEMPT]
    assert not missing, "exported kernels with an oracle that no tests/*_gpu.py calls: %s" % missing
    stale = [n for n in EXEMPT if "." + n + "(" in text]
    assert not stale, "exempted but called by a GPU test: %s" % stale


@pytest.mark.parametrize("case", kg.WINDOW_CONV_CASES)
def test_oracle_meets_conv_window_checks(case):
    geom, ld, off, _ = case
    for bias, relu in kg.WINDOW_CONV_FLAVOURS:
        inputs, win = kg.check_conv_window(ref, CPU, geom, ld, off, bias, relu)
        kg.conv_window_same_as_contiguous(ref, CPU, inputs, win)


# (the streaming case differs from these only in size: the GPU run alone)
@pytest.mark.parametrize("case", kg.BN_WINDOW_CASES)
def test_oracle_meets_bn_window_checks(case):
    for relu in (True, False):
        for x_window in (False, True):
            kg.check_bn_fwd_window(ref, CPU, *case, relu, x_window)
    kg.check_bn_bwd_window(ref, CPU, *case)
    kg.check_bn_bwd_apply_window(ref, CPU, *case)


def test_neighbour_check_sees_a_spill():
    """One changed element right or left of the window fails the neighbour check; changes
    inside the window do not."""
    buf, win = kg.sentinel_window((5, 3), 16, 8, 4, torch.bfloat16, CPU)
    buf0 = buf.clone()
    win.zero_()
    assert kg.neighbours_untouched(buf, buf0, 8, 4)
    for col in (7, 12, 0, 15):
        spilled = buf.clone()
        spilled[4, 2, col] += 1.0
        assert not kg.neighbours_untouched(spilled, buf0, 8, 4)


def test_oracle_meets_small_kernel_checks():
    for case in kg.CHAN_CASES:
        for assign in (True, False):
            kg.check_chan_accum(ref, CPU, *case, assign)
        kg.check_chan_extract(ref, CPU, *case, torch.float32)  # (the CPU path keeps fp32)
    for n in (1, 7, 4099):
        kg.check_add_f32(ref, CPU, n)
    for n in (4, 4100):
        kg.check_zero_f32(ref, CPU, n)
    kg.check_step_inc(ref, CPU)
    for n in (8, 8 * 1003):
        kg.check_relu_fwd(ref, CPU, n)
    for M, Cc in ((1003, 24), (37, 136)):
        for relu in (True, False):
            kg.check_affine_act(ref, CPU, M, Cc, relu)
    for NC in (1000, 33):
        kg.check_ce_fwd_weighted(ref, CPU, 300, NC)


def test_affine_act_bound_rejects_two_bf16_steps():
    """The affine_act bound admits the fused multiply-add's value and rejects a result two
    bf16 steps away."""
    torch.manual_seed(51)
    x = kg.bf(64, 8, dev=CPU, scale=2.0).clamp(-8, 8)
    aff = torch.stack([torch.rand(8) + 0.5, torch.randn(8)])
    want = ref.affine_act(x, aff, False)
    fused = torch.addcmul(aff[1].double(), x.double(), aff[0].double()).to(torch.bfloat16)
    bound = kg.affine_act_bound(x, aff, want)
    assert bool(((fused.double() - want.double()).abs() <= bound).all())
    two = (want.view(torch.int16) + 2).view(torch.bfloat16)  # two steps up in magnitude
    big = want.float().abs() > 0.5
    assert bool(((two.double() - want.double()).abs() > bound)[big].all())
