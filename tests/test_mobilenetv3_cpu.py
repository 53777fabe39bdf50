"""MobileNetV3-Large and the squeeze-excite op layer on the CPU: the checks of ``test_se_gpu.py``
met by ``ref`` alone, the ``ref`` twins against torch's own ops and autograd, torchvision's
parameter layout, the registry, one training step, and the launch-plan check program."""
import os
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

import test_se_gpu as sg
from mpi_pytorch_amd.config import Config
from mpi_pytorch_amd.engine import build_model, loss_fn
from mpi_pytorch_amd.models import initialize_model
from mpi_pytorch_amd.models.mobilenetv3 import mobilenet_v3_large
from mpi_pytorch_amd.ops import ref
from mpi_pytorch_amd.parallel import World

CPU = torch.device("cpu")
KDIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc", "kernels")


@pytest.mark.parametrize("case", sg.EXACT_CASES)
def test_reference_alone_is_exact(case):
    sg.check_exact(ref, CPU, case)


@pytest.mark.parametrize("case", sg.ROUNDING_CASES)
@pytest.mark.parametrize("act", [1, 2])
def test_reference_alone_meets_the_rounding_bounds(act, case):
    sg.check_rounding(ref, CPU, act, case)


def test_reference_hardswish_points_and_repeatability():
    sg.check_hardswish_points(ref, CPU)
    sg.check_repeatable(ref, CPU)


@pytest.mark.parametrize("act", [1, 2])
def test_ref_twins_match_a_torch_composed_se_segment(act):
    torch.manual_seed(2)
    N, H, W, Cc, Cs = 2, 5, 6, 16, 8
    z = torch.randn(N, H, W, Cc, requires_grad=True)
    gamma, rstd, mean = torch.rand(Cc) + 0.5, torch.rand(Cc) + 0.5, torch.randn(Cc) * 0.2
    beta = torch.randn(Cc) * 0.3
    fc1, fc2 = torch.nn.Conv2d(Cc, Cs, 1), torch.nn.Conv2d(Cs, Cc, 1)
    aff = torch.stack([gamma * rstd, beta - mean * gamma * rstd])
    t = (z * aff[0] + aff[1]).permute(0, 3, 1, 2)
    a = F.hardswish(t) if act == 2 else F.relu(t)
    s = F.adaptive_avg_pool2d(a, 1)
    hid = F.relu(fc1(s))
    gt = F.hardsigmoid(fc2(hid))
    u = (a * gt).permute(0, 2, 3, 1)
    du = torch.randn_like(u)
    u.backward(du)
    w1, w2 = fc1.weight.detach().permute(0, 2, 3, 1), fc2.weight.detach().permute(0, 2, 3, 1)
    zd, close = z.detach(), lambda x, y: torch.allclose(x, y, atol=2e-5, rtol=1e-4)  # noqa: E731
    pooled = ref.act_pool(zd, aff, act)
    h, gate = ref.se_gate(pooled, w1, fc1.bias.detach(), w2, fc2.bias.detach())
    assert close(pooled, s.flatten(1)) and close(h, hid.flatten(1)) and close(gate, gt.flatten(1))
    assert close(ref.act_gate_fwd(zd, aff, act, gate), u)
    dgate = ref.act_gate_bwd_pool(du, zd, aff, act)
    dpre2, dpre1, dpool = ref.se_gate_bwd(dgate, h, gate, w1, w2, 1.0 / (H * W))
    for fc, dpre, inp in ((fc2, dpre2, h), (fc1, dpre1, pooled)):
        gw, gb = torch.zeros_like(fc.weight).permute(0, 2, 3, 1).contiguous(), torch.zeros_like(fc.bias)
        ref.se_fc_wgrad(dpre, inp, gw, gb, overwrite=True)
        assert close(gw.permute(0, 3, 1, 2), fc.weight.grad) and close(gb, fc.bias.grad)
    # z's gradient through the affine alone: a "BN" with statistics held fixed is dx = g aff[0]
    e = torch.empty(0)
    g = ref.act_gate_bwd_dx(du, zd, aff, act, gate, dpool, e, e, e, e)
    assert close(g * aff[0], z.grad)
    sums = ref.act_gate_bwd_sums(du, zd, aff, act, gate, dpool, mean, rstd)
    assert close(sums[0], g.sum((0, 1, 2))) and close(sums[1], (g * (zd - mean) * rstd).sum((0, 1, 2)))


@pytest.mark.parametrize("act", [0, 1, 2])
def test_bn_act_gate_matches_torch_batchnorm_autograd(act):
    """The op layer's train-mode BN backward (sums, dx, dgamma, dbeta) with an SE gate."""
    from mpi_pytorch_amd.models.layers import BatchNorm2d, SqueezeExcitation
    from mpi_pytorch_amd.ops import functional as Fn
    torch.manual_seed(5)
    N, H, W, Cc, Cs = 3, 4, 5, 16, 8
    bn, se = BatchNorm2d(Cc, eps=1e-3), SqueezeExcitation(Cc, Cs)
    torch.nn.init.uniform_(bn.weight, 0.5, 1.5)
    torch.nn.init.normal_(bn.bias, 0.0, 0.5)
    z = torch.randn(N, H, W, Cc, requires_grad=True)
    u = Fn.bn_act_gate(z, bn, act, se)
    du = torch.randn_like(u)
    u.backward(du)
    got = [u.detach(), z.grad, bn.weight.grad, bn.bias.grad, se.fc1.weight.grad, se.fc2.bias.grad]
    z2 = z.detach().clone().requires_grad_()
    ps = [p.detach().clone().requires_grad_() for p in
          (bn.weight, bn.bias, se.fc1.weight, se.fc1.bias, se.fc2.weight, se.fc2.bias)]
    t = F.batch_norm(z2.permute(0, 3, 1, 2), None, None, ps[0], ps[1], True, 0.1, 1e-3)
    a = {0: t, 1: F.relu(t), 2: F.hardswish(t)}[act]
    hid = F.relu(F.conv2d(F.adaptive_avg_pool2d(a, 1), ps[2].permute(0, 3, 1, 2), ps[3]))
    u2 = (a * F.hardsigmoid(F.conv2d(hid, ps[4].permute(0, 3, 1, 2), ps[5]))).permute(0, 2, 3, 1)
    u2.backward(du)
    want = [u2.detach(), z2.grad, ps[0].grad, ps[1].grad, ps[2].grad, ps[5].grad]
    for a_, b_ in zip(got, want):
        assert torch.allclose(a_, b_, atol=1e-4, rtol=1e-3), (a_ - b_).abs().max()


@pytest.mark.parametrize("classes,total", [(1000, 5483032), (64500, 86826532)])
def test_parameter_layout_is_torchvisions(classes, total):
    sd = initialize_model("mobilenet_v3", classes, False)[0].state_dict()
    ps = [v for k, v in sd.items() if "running_" not in k and "num_batches" not in k]
    assert sum(p.numel() for p in ps) == total
    assert tuple(sd["features.4.block.2.fc1.weight"].shape) == (24, 72, 1, 1)
    assert tuple(sd["features.15.block.2.fc2.bias"].shape) == (960,)
    assert tuple(sd["features.13.block.1.0.weight"].shape) == (672, 1, 5, 5)
    assert tuple(sd["features.0.1.running_var"].shape) == (16,)
    assert tuple(sd["classifier.0.weight"].shape) == (1280, 960)
    assert tuple(sd["classifier.3.weight"].shape) == (classes, 1280)


def test_state_dict_round_trip_is_bitwise():
    torch.manual_seed(0)
    sd = mobilenet_v3_large(10).state_dict()
    m = mobilenet_v3_large(10)
    m.load_state_dict(sd)
    sd2 = m.state_dict()
    assert list(sd) == list(sd2) and all(torch.equal(sd[k], sd2[k]) for k in sd)


def test_registry_and_config():
    assert initialize_model("mobilenet_v3", 20, False)[1] == 224
    with pytest.raises(ValueError):
        initialize_model("mobilenet_v4", 10, False)
    assert Config(MODEL_NAME="mobilenet_v3").CHECKPOINT_NAME == "checkpoint_mobilenet_v3.pt"


def test_train_step_cpu():
    torch.manual_seed(0)
    m, _ = build_model("mobilenet_v3", 20, False, CPU, World())
    loss = loss_fn(m(torch.randn(2, 32, 32, 3)), torch.randint(0, 20, (2,)))
    loss.backward()
    g = m._mpa_arena.grad
    assert bool(torch.isfinite(loss)) and torch.isfinite(g).all() and float(g.abs().sum()) > 0


def test_launch_plans_hold_their_invariants(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "se_plan_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-I", KDIR,
                        os.path.join(KDIR, "se_plan_check.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "se_plan_check sweep ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
