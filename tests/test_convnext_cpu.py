"""ConvNeXt-Tiny and its op layer on the CPU: torchvision's parameter layout, the registry, a
reduced model against a plain ``torch.nn`` composition, the checks of ``test_ln_gpu.py`` met by
``ref`` alone, and the launch-plan check programs."""
import os
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

import test_ln_gpu as lg
from mpi_pytorch_amd.models import LN_ARCH, initialize_model
from mpi_pytorch_amd.models.convnext import ConvNeXt, convnext_tiny
from mpi_pytorch_amd.ops import ref
from mpi_pytorch_amd.parallel.arena import ParamArena

CPU = torch.device("cpu")
KDIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc", "kernels")

STAGE1_AND_HEAD = [
    ("features.0.0.weight", (96, 3, 4, 4)), ("features.0.0.bias", (96,)),
    ("features.0.1.weight", (96,)), ("features.0.1.bias", (96,)),
    ("features.1.0.layer_scale", (96, 1, 1)),
    ("features.1.0.block.0.weight", (96, 1, 7, 7)), ("features.1.0.block.0.bias", (96,)),
    ("features.1.0.block.2.weight", (96,)), ("features.1.0.block.2.bias", (96,)),
    ("features.1.0.block.3.weight", (384, 96)), ("features.1.0.block.3.bias", (384,)),
    ("features.1.0.block.5.weight", (96, 384)), ("features.1.0.block.5.bias", (96,)),
    ("features.2.0.weight", (96,)), ("features.2.0.bias", (96,)),
    ("features.2.1.weight", (192, 96, 2, 2)), ("features.2.1.bias", (192,)),
    ("classifier.0.weight", (768,)), ("classifier.0.bias", (768,)),
    ("classifier.2.weight", (1000, 768)), ("classifier.2.bias", (1000,)),
]


def test_parameter_layout_is_torchvisions():
    assert list(LN_ARCH) == ["convnext"]
    m = initialize_model("convnext", 1000, False)[0]
    sd = m.state_dict()
    assert sum(v.numel() for v in sd.values()) == 28589128
    assert all(tuple(sd[k].shape) == s for k, s in STAGE1_AND_HEAD)
    keys = [k for k in sd if k.startswith(("features.0.", "features.1.0.", "features.2.", "classifier."))]
    assert keys == [k for k, _ in STAGE1_AND_HEAD]
    assert float(sd["features.1.0.layer_scale"].max()) == pytest.approx(1e-6)
    assert m.features[1][0].layer_scale.dim() == 1  # a per-channel scale for --wd_exclude_1d
    m2 = convnext_tiny(1000)
    m2.load_state_dict(sd)
    sd2 = m2.state_dict()
    assert list(sd) == list(sd2) and all(torch.equal(sd[k], sd2[k]) for k in sd)


def _nn_forward(sd, x, depths):
    """The same network from torch.nn.functional on NCHW, reading the state_dict."""
    def ln2d(t, p):
        t = F.layer_norm(t.permute(0, 2, 3, 1), t.shape[1:2], sd[p + "weight"], sd[p + "bias"], 1e-6)
        return t.permute(0, 3, 1, 2)
    x = ln2d(F.conv2d(x, sd["features.0.0.weight"], sd["features.0.0.bias"], 4), "features.0.1.")
    for i, depth in enumerate(depths):
        for b in range(depth):
            p = "features.%d.%d." % (2 * i + 1, b)
            y = F.conv2d(x, sd[p + "block.0.weight"], sd[p + "block.0.bias"], 1, 3, 1, x.shape[1])
            y = F.layer_norm(y.permute(0, 2, 3, 1), y.shape[1:2], sd[p + "block.2.weight"],
                             sd[p + "block.2.bias"], 1e-6)
            y = F.gelu(F.linear(y, sd[p + "block.3.weight"], sd[p + "block.3.bias"]))
            y = F.linear(y, sd[p + "block.5.weight"], sd[p + "block.5.bias"]).permute(0, 3, 1, 2)
            x = x + sd[p + "layer_scale"] * y
        if i + 1 < len(depths):
            p = "features.%d." % (2 * i + 2)
            x = F.conv2d(ln2d(x, p + "0."), sd[p + "1.weight"], sd[p + "1.bias"], 2)
    x = ln2d(x.mean((2, 3), keepdim=True), "classifier.0.").flatten(1)
    return F.linear(x, sd["classifier.2.weight"], sd["classifier.2.bias"])


def test_reduced_model_matches_torch_nn():
    torch.manual_seed(0)
    depths = (1, 1, 1, 1)
    m = ConvNeXt(depths, (24, 48, 96, 192), 10, layer_scale=0.5)
    for p in m.parameters():
        if p.dim() == 1:
            torch.nn.init.normal_(p, 0.5, 0.3)
    sd = {k: v.clone().requires_grad_() for k, v in m.state_dict().items()}
    ParamArena(m, CPU)
    x = torch.randn(2, 64, 64, 3)
    dy = torch.randn(2, 10)
    y = m(x)
    y.backward(dy)
    want = _nn_forward(sd, x.permute(0, 3, 1, 2), depths)
    want.backward(dy)
    assert torch.allclose(y, want, rtol=1e-4, atol=1e-4)
    got = dict(m.named_parameters())
    for name in ("features.0.0.weight", "features.1.0.block.0.weight", "features.1.0.block.0.bias",
                 "features.1.0.block.2.weight", "features.1.0.block.3.bias",
                 "features.1.0.layer_scale", "features.2.0.bias", "features.2.1.weight",
                 "classifier.0.weight", "classifier.2.weight"):
        p = got[name]
        g = p._mpa_export(p.grad) if getattr(p, "_mpa_export", None) else p.grad
        assert torch.allclose(g, sd[name].grad, rtol=1e-3, atol=1e-4), name


def test_train_step_through_the_registry():
    from mpi_pytorch_amd.engine import build_model, loss_fn
    from mpi_pytorch_amd.parallel import World
    torch.manual_seed(0)
    m, _ = build_model("convnext", 20, False, CPU, World())
    loss = loss_fn(m(torch.randn(2, 32, 32, 3)), torch.randint(0, 20, (2,)))
    loss.backward()
    g = m._mpa_arena.grad
    assert bool(torch.isfinite(loss)) and torch.isfinite(g).all() and float(g.abs().sum()) > 0


@pytest.mark.parametrize("pre", [False, True])
@pytest.mark.parametrize("shape", lg.LN_SHAPES)
def test_reference_alone_meets_the_layer_norm_checks(shape, pre):
    lg.check_ln_exact(ref, CPU, *shape, pre)
    lg.check_ln_rounding(ref, CPU, *shape, pre)


def test_reference_alone_meets_the_elementwise_checks():
    for M in lg.GELU_ROWS:
        lg.check_gelu(ref, CPU, M)
    for shape in lg.SCALE_SHAPES:
        lg.check_scale_add(ref, CPU, *shape)
    for case in lg.DW7_CASES[:3]:
        lg.check_dw7_exact(ref, CPU, case)


@pytest.mark.parametrize("name", ["ln_plan_check", "dw_plan_check"])
def test_launch_plans_hold_their_invariants(tmp_path, name):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / name)
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-I", KDIR,
                        os.path.join(KDIR, name + ".cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and name + " sweep ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
