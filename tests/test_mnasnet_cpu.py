"""MNASNet-1.0 and the depthwise conv op layer on the CPU: torchvision's parameter layout, the
``groups`` argument of ``layers.Conv2d``, the model registry, the fp32 ``ref`` twins, the
checks of ``test_depthwise_gpu.py`` met by ``ref`` alone, and the launch-plan check program."""
import os
import shutil
import subprocess

import pytest
import torch

import test_depthwise_gpu as dg
from mpi_pytorch_amd.engine import build_model, loss_fn
from mpi_pytorch_amd.models import ARCH, EXTRA_ARCH, initialize_model
from mpi_pytorch_amd.models.layers import Conv2d
from mpi_pytorch_amd.models.mnasnet import mnasnet1_0
from mpi_pytorch_amd.ops import ref
from mpi_pytorch_amd.parallel import World

CPU = torch.device("cpu")
KDIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc", "kernels")


def _params(sd):
    return [v for k, v in sd.items() if "running_" not in k and "num_batches" not in k]


@pytest.mark.parametrize("classes,total", [(1000, 4383312), (64500, 85726812)])
def test_parameter_layout_is_torchvisions(classes, total):
    sd = initialize_model("mnasnet", classes, False)[0].state_dict()
    ps = _params(sd)
    assert (sum(p.numel() for p in ps), len(ps)) == (total, 158)
    assert tuple(sd["layers.3.weight"].shape) == (32, 1, 3, 3)
    assert tuple(sd["layers.8.0.layers.3.weight"].shape) == (48, 1, 3, 3)
    assert tuple(sd["layers.10.1.layers.3.weight"].shape) == (480, 1, 5, 5)
    assert tuple(sd["classifier.1.weight"].shape) == (classes, 1280)


def test_state_dict_round_trip_is_bitwise():
    torch.manual_seed(0)
    sd = mnasnet1_0(10).state_dict()
    m = mnasnet1_0(10)
    m.load_state_dict(sd)
    sd2 = m.state_dict()
    assert list(sd) == list(sd2) and all(torch.equal(sd[k], sd2[k]) for k in sd)


def test_groups_and_registry():
    with pytest.raises(ValueError):
        Conv2d(8, 8, 3, 1, 1, groups=4)
    with pytest.raises(ValueError):
        initialize_model("mnasnet2", 10, False)
    assert list(ARCH) == ["resnet18", "resnet34", "alexnet", "vgg", "vgg16", "squeezenet",
                          "densenet", "inception"]
    assert list(EXTRA_ARCH) == ["mnasnet"]


def test_train_step_cpu():
    torch.manual_seed(0)
    m, _ = build_model("mnasnet", 20, False, CPU, World())
    loss = loss_fn(m(torch.randn(2, 32, 32, 3)), torch.randint(0, 20, (2,)))
    loss.backward()
    g = m._mpa_arena.grad
    assert bool(torch.isfinite(loss)) and torch.isfinite(g).all() and float(g.abs().sum()) > 0


@pytest.mark.parametrize("k,s", [(3, 1), (5, 2)])
def test_ref_twins_match_nn_conv2d_autograd(k, s):
    torch.manual_seed(1)
    C, p = 16, k // 2
    conv = torch.nn.Conv2d(C, C, k, s, p, groups=C, bias=False)
    x = torch.randn(2, 9, 10, C, requires_grad=True)
    y = conv(x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    dy = torch.randn_like(y)
    y.backward(dy)
    w = conv.weight.detach().permute(0, 2, 3, 1).contiguous()  # [C, k, k, 1]
    e = torch.empty(0)
    assert torch.allclose(ref.dwconv_fwd(x.detach(), w, s, s, p, p, e, e), y, atol=1e-5)
    assert torch.allclose(ref.dwconv_dgrad(dy, w, 9, 10, s, s, p, p), x.grad, atol=1e-5)
    g = torch.zeros_like(w)
    ref.dwconv_wgrad(dy, x.detach(), g, s, s, p, p, overwrite=True)
    assert torch.allclose(g, conv.weight.grad.permute(0, 2, 3, 1), atol=1e-4)


@pytest.mark.parametrize("case", dg.CASES[:6])
def test_reference_alone_is_exact(case):
    dg.check_exact(ref, CPU, case)


def test_reference_alone_meets_the_rounding_bounds():
    dg.check_rounding(ref, CPU)


def test_launch_plans_hold_their_invariants(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "dw_plan_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-I", KDIR,
                        os.path.join(KDIR, "dw_plan_check.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "dw_plan_check sweep ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
