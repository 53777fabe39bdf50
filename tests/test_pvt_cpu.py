"""PVT v2 B2 and its op layer on the CPU: the official parameter layout, the registry, the checks
of ``test_xattn_gpu.py`` met by ``ref`` alone, and the launch-plan check program."""
import os
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

import test_xattn_gpu as xg
from mpi_pytorch_amd.models import PYRAMID_ARCH, head_parameters, initialize_model
from mpi_pytorch_amd.models.layers import SpatialReductionAttention
from mpi_pytorch_amd.models.pvt import PyramidVisionTransformerV2
from mpi_pytorch_amd.ops import ref

CPU = torch.device("cpu")
KDIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc", "kernels")

SPOT = [
    ("patch_embed1.proj.weight", (64, 3, 7, 7)), ("patch_embed2.proj.weight", (128, 64, 3, 3)),
    ("patch_embed1.norm.weight", (64,)), ("block1.0.norm1.bias", (64,)),
    ("block1.0.attn.q.weight", (64, 64)), ("block1.0.attn.kv.weight", (128, 64)),
    ("block1.0.attn.kv.bias", (128,)), ("block1.0.attn.proj.weight", (64, 64)),
    ("block1.0.attn.sr.weight", (64, 64, 8, 8)), ("block1.0.attn.sr.bias", (64,)),
    ("block1.0.attn.norm.weight", (64,)), ("block1.0.mlp.fc1.weight", (512, 64)),
    ("block3.5.mlp.dwconv.dwconv.weight", (1280, 1, 3, 3)), ("block3.5.mlp.dwconv.dwconv.bias", (1280,)),
    ("block3.5.mlp.fc2.weight", (320, 1280)), ("block4.2.attn.kv.weight", (1024, 512)),
    ("norm4.weight", (512,)), ("head.weight", (1000, 512)), ("head.bias", (1000,)),
]


def _count():
    """The parameter total from the configuration's shapes."""
    n, cin = 512 * 1000 + 1000, 3
    for s, (D, depth, m, r) in enumerate(zip((64, 128, 320, 512), (3, 4, 6, 3), (8, 8, 4, 4), (8, 4, 2, 1))):
        k = 7 if s == 0 else 3
        n += cin * D * k * k + D + 2 * D + 2 * D                       # embed conv, its norm, norm{i}
        blk = 2 * D + 4 * D * D + 4 * D + 2 * D                        # norm1, q / kv / proj, norm2
        blk += (D * D * r * r + D + 2 * D) if r > 1 else 0             # sr, its norm
        blk += D * m * D + m * D + 9 * m * D + m * D + m * D * D + D   # fc1, dwconv, fc2
        n += depth * blk
        cin = D
    return n


def test_parameter_layout_is_the_official_one():
    assert list(PYRAMID_ARCH) == ["pvt_v2"] and PYRAMID_ARCH["pvt_v2"][2] == 224
    m = initialize_model("pvt_v2", 1000, False)[0]
    sd = m.state_dict()
    assert all(tuple(sd[k].shape) == s for k, s in SPOT)
    assert not [k for k in sd if k.startswith("block4.") and (".attn.sr." in k or ".attn.norm." in k)]
    assert _count() == 25362856 and sum(v.numel() for v in sd.values()) == _count()
    assert len(sd) == 4 * 6 + 2 + 13 * 20 + 3 * 16  # embeds and norm{i}, head; blocks with / without sr
    m2 = initialize_model("pvt_v2", 1000, False)[0]
    m2.load_state_dict(sd)
    sd2 = m2.state_dict()
    assert list(sd) == list(sd2) and all(torch.equal(sd[k], sd2[k]) for k in sd)


def test_registry_replaces_the_head_and_trains():
    m = initialize_model("pvt_v2", 37, True)[0]
    head = list(head_parameters(m))
    assert [tuple(p.shape) for p in head] == [(64, 512), (64,)] and all(p.requires_grad for p in head)
    assert m.head.out_features == 37 and not m.patch_embed1.proj.weight.requires_grad

    from mpi_pytorch_amd.parallel.arena import ParamArena
    torch.manual_seed(0)
    m = PyramidVisionTransformerV2(depths=(1, 1, 1, 1), num_classes=10)
    arena = ParamArena(m, CPU)
    loss = F.cross_entropy(m(torch.randn(2, 64, 64, 3)), torch.tensor([1, 7]))
    loss.backward()
    assert bool(torch.isfinite(loss)) and torch.isfinite(arena.grad).all()
    assert all(float(p.grad.abs().sum()) > 0 for p in m.parameters())


def test_block_matches_the_published_algorithm():
    """Fixes kv's [2][H][64] column order, the reduction's token order and the bias of the MLP's
    depthwise conv against the official forward, written with torch's own layers."""
    from mpi_pytorch_amd.models.pvt import PVTBlock
    torch.manual_seed(1)
    blk = PVTBlock(128, 2, 4, 2)
    for p in blk.parameters():
        if p.dim() == 1:
            torch.nn.init.normal_(p, 0.2, 0.3)
    sd = blk.state_dict()
    x = torch.randn(2, 8, 6, 128)
    B, Hf, Wf, D = x.shape
    t = x.reshape(B, Hf * Wf, D)
    n1 = F.layer_norm(t, (D,), sd["norm1.weight"], sd["norm1.bias"], 1e-6)
    q = F.linear(n1, sd["attn.q.weight"], sd["attn.q.bias"]).reshape(B, -1, 2, 64).permute(0, 2, 1, 3)
    red = F.conv2d(n1.permute(0, 2, 1).reshape(B, D, Hf, Wf), sd["attn.sr.weight"], sd["attn.sr.bias"], stride=2)
    red = F.layer_norm(red.reshape(B, D, -1).permute(0, 2, 1), (D,), sd["attn.norm.weight"], sd["attn.norm.bias"], 1e-5)
    k, v = F.linear(red, sd["attn.kv.weight"], sd["attn.kv.bias"]).reshape(B, -1, 2, 2, 64).permute(2, 0, 3, 1, 4)
    o = (torch.softmax(q @ k.transpose(-2, -1) / 8, -1) @ v).transpose(1, 2).reshape(B, -1, D)
    t = t + F.linear(o, sd["attn.proj.weight"], sd["attn.proj.bias"])
    h = F.linear(F.layer_norm(t, (D,), sd["norm2.weight"], sd["norm2.bias"], 1e-6), sd["mlp.fc1.weight"], sd["mlp.fc1.bias"])
    h = F.conv2d(h.transpose(1, 2).reshape(B, 4 * D, Hf, Wf), sd["mlp.dwconv.dwconv.weight"],
                 sd["mlp.dwconv.dwconv.bias"], padding=1, groups=4 * D).flatten(2).transpose(1, 2)
    want = t + F.linear(F.gelu(h), sd["mlp.fc2.weight"], sd["mlp.fc2.bias"])
    with torch.no_grad():
        got = blk(x.clone()).reshape(B, Hf * Wf, D)
    assert torch.allclose(got, want, rtol=2e-2, atol=2e-2)  # (P is a bf16 operand)
    assert float(F.cosine_similarity(got.flatten(), want.flatten(), 0)) > 0.9999


def test_layer_refusals():
    with pytest.raises(ValueError, match="64"):
        SpatialReductionAttention(96, 2)
    m = PyramidVisionTransformerV2(depths=(1, 1, 1, 1), num_classes=10)
    with pytest.raises(ValueError, match="64"):  # 288 x 288: 9 x 9 = 81 keys
        m(torch.randn(1, 288, 288, 3))


@pytest.mark.parametrize("case", xg.CASES)
def test_reference_alone_meets_the_cross_attention_checks(case):
    xg.check_lookup(ref, CPU, *case)
    xg.check_rounding(ref, CPU, *case)
    if case in xg.UNIFORM_CASES:
        xg.check_uniform(ref, CPU, *case)


def test_reference_alone_meets_the_other_checks():
    xg.check_repeatable(ref, CPU, *xg.PLAN_CASE)
    xg.check_xattn_refusals(ref, CPU)
    for case in xg.GELU_CASES:
        xg.check_gelu_pre_bias(ref, CPU, *case)


def test_cross_attention_plan_holds_its_invariants(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "xattn_plan_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-I", KDIR,
                        os.path.join(KDIR, "xattn_plan_check.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "xattn_plan_check sweep ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
