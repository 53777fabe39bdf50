"""ResNeXt-50 32x4d and the grouped conv op layer on the CPU: torchvision's parameter layout,
the grouped geometries of ``layers.Conv2d``, the model registry, the fp32 ``ref`` twins, the
checks of ``test_gconv_gpu.py`` met by ``ref`` alone, and the launch-plan check program."""
import os
import shutil
import subprocess

import pytest
import torch

import test_gconv_gpu as gg
from mpi_pytorch_amd.engine import build_model, loss_fn
from mpi_pytorch_amd.models import ARCH, GROUPED_ARCH, initialize_model
from mpi_pytorch_amd.models.layers import Conv2d
from mpi_pytorch_amd.models.resnet import resnext50_32x4d
from mpi_pytorch_amd.ops import ref
from mpi_pytorch_amd.parallel import World

CPU = torch.device("cpu")
KDIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc", "kernels")


@pytest.mark.parametrize("classes,total", [(1000, 25028904), (64500, 155140404)])
def test_parameter_layout_is_torchvisions(classes, total):
    sd = initialize_model("resnext50", classes, False)[0].state_dict()
    ps = [v for k, v in sd.items() if "running_" not in k and "num_batches" not in k]
    assert (sum(p.numel() for p in ps), len(ps)) == (total, 161)
    assert tuple(sd["layer1.0.conv2.weight"].shape) == (128, 4, 3, 3)
    assert tuple(sd["layer4.2.conv2.weight"].shape) == (1024, 32, 3, 3)
    assert tuple(sd["layer2.0.downsample.0.weight"].shape) == (512, 256, 1, 1)
    assert tuple(sd["fc.weight"].shape) == (classes, 2048)


def test_state_dict_round_trip_is_bitwise():
    torch.manual_seed(0)
    sd = resnext50_32x4d(10).state_dict()
    m = resnext50_32x4d(10)
    m.load_state_dict(sd)
    sd2 = m.state_dict()
    assert list(sd) == list(sd2) and all(torch.equal(sd[k], sd2[k]) for k in sd)


def test_groups_and_registry():
    assert Conv2d(128, 128, 3, 1, 1, bias=False, groups=32).weight.shape == (128, 3, 3, 4)
    for args, kw in (((8, 8, 3, 1, 1), {"groups": 4}),        # Cg = 2
                     ((64, 64, 5, 1, 2), {"groups": 8}),      # 5 x 5
                     ((64, 128, 3, 1, 1), {"groups": 8}),     # cin != cout
                     ((64, 64, 3, 1, 0), {"groups": 8})):     # padding 0
        with pytest.raises(ValueError):
            Conv2d(*args, **kw)
    with pytest.raises(ValueError):
        initialize_model("resnext51", 10, False)
    assert list(GROUPED_ARCH) == ["resnext50"] and "resnext50" not in ARCH
    assert GROUPED_ARCH["resnext50"][0] == "resnext50_32x4d" and GROUPED_ARCH["resnext50"][2] == 224


def test_train_step_cpu():
    torch.manual_seed(0)
    m, _ = build_model("resnext50", 20, False, CPU, World())
    loss = loss_fn(m(torch.randn(2, 32, 32, 3)), torch.randint(0, 20, (2,)))
    loss.backward()
    g = m._mpa_arena.grad
    assert bool(torch.isfinite(loss)) and torch.isfinite(g).all() and float(g.abs().sum()) > 0


@pytest.mark.parametrize("groups,s", [(8, 1), (2, 2)])
def test_ref_twins_match_nn_conv2d_autograd(groups, s):
    torch.manual_seed(1)
    C = 32
    conv = torch.nn.Conv2d(C, C, 3, s, 1, groups=groups, bias=False)
    x = torch.randn(2, 9, 10, C, requires_grad=True)
    y = conv(x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    dy = torch.randn_like(y)
    y.backward(dy)
    w = conv.weight.detach().permute(0, 2, 3, 1).contiguous()  # [C, 3, 3, Cg]
    e = torch.empty(0)
    assert torch.allclose(ref.gconv_fwd(x.detach(), w, s, s, 1, 1, e, e), y, atol=1e-5)
    assert torch.allclose(ref.gconv_dgrad(dy, w, 9, 10, s, s, 1, 1), x.grad, atol=1e-5)
    g = torch.zeros_like(w)
    ref.gconv_wgrad(dy, x.detach(), g, s, s, 1, 1, overwrite=True)
    assert torch.allclose(g, conv.weight.grad.permute(0, 2, 3, 1), atol=1e-4)


@pytest.mark.parametrize("case", gg.CASES)
def test_reference_alone_is_exact(case):
    gg.check_exact(ref, CPU, case)


@pytest.mark.parametrize("case", [gg.CASE_D, gg.CASE_E2])
def test_reference_alone_meets_the_rounding_bounds(case):
    gg.check_rounding(ref, CPU, case)


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined"]])
def test_launch_plans_hold_their_invariants(tmp_path, flags):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "gconv_plan_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags,
                        "-I", KDIR, os.path.join(KDIR, "gconv_plan_check.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "gconv_plan_check sweep ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
