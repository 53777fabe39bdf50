"""NAT-Mini and its op layer on the CPU: the official parameter layout, the registry, the checks
of ``test_nattn_gpu.py`` met by ``ref`` alone, and the launch-plan check program."""
import os
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

import test_nattn_gpu as ng
from mpi_pytorch_amd.models import NEIGHBORHOOD_ARCH, head_parameters, initialize_model
from mpi_pytorch_amd.ops import ref

CPU = torch.device("cpu")
KDIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc", "kernels")

SPOT = [
    ("patch_embed.proj.0.weight", (32, 3, 3, 3)), ("patch_embed.proj.0.bias", (32,)),
    ("patch_embed.proj.1.weight", (64, 32, 3, 3)), ("patch_embed.norm.weight", (64,)),
    ("levels.0.blocks.0.norm1.bias", (64,)), ("levels.0.blocks.0.attn.qkv.weight", (192, 64)),
    ("levels.0.blocks.0.attn.rpb", (2, 13, 13)), ("levels.0.blocks.2.attn.proj.bias", (64,)),
    ("levels.0.blocks.0.mlp.fc1.weight", (192, 64)), ("levels.0.downsample.reduction.weight", (128, 64, 3, 3)),
    ("levels.0.downsample.norm.weight", (128,)), ("levels.2.blocks.5.mlp.fc2.weight", (256, 768)),
    ("levels.3.blocks.4.attn.rpb", (16, 13, 13)), ("norm.weight", (512,)), ("head.weight", (1000, 512)),
]


def test_parameter_layout_is_the_official_one():
    assert list(NEIGHBORHOOD_ARCH) == ["nat"] and NEIGHBORHOOD_ARCH["nat"][2] == 224
    m = initialize_model("nat", 1000, False)[0]
    sd = m.state_dict()
    assert all(tuple(sd[k].shape) == s for k, s in SPOT)
    assert "levels.3.downsample.reduction.weight" not in sd and "levels.0.downsample.reduction.bias" not in sd
    assert sum(v.numel() for v in sd.values()) == 19984174
    m2 = initialize_model("nat", 1000, False)[0]
    m2.load_state_dict(sd)
    sd2 = m2.state_dict()
    assert list(sd) == list(sd2) and all(torch.equal(sd[k], sd2[k]) for k in sd)


def test_registry_replaces_the_head_and_trains():
    from mpi_pytorch_amd.parallel.arena import ParamArena
    m = initialize_model("nat", 37, True)[0]
    head = list(head_parameters(m))
    assert [tuple(p.shape) for p in head] == [(64, 512), (64,)] and all(p.requires_grad for p in head)
    assert m.head.out_features == 37 and not m.levels[0].blocks[0].attn.rpb.requires_grad
    with pytest.raises(ValueError, match="224"):
        m(torch.randn(1, 192, 224, 3))
    torch.manual_seed(0)
    m = initialize_model("nat", 10, False)[0]
    arena = ParamArena(m, CPU)
    loss = F.cross_entropy(m(torch.randn(1, 224, 224, 3)), torch.tensor([7]))
    loss.backward()
    assert bool(torch.isfinite(loss)) and torch.isfinite(arena.grad).all()
    assert all(float(p.grad.abs().sum()) > 0 for p in m.parameters())


def test_reference_forward_matches_a_per_query_loop():
    B, H, Hf, Wf = case = (1, 1, 8, 9)
    qkv, _, rpb = ng._inputs(case, CPU)
    q, k, v = (t[0, 0] for t in ng._split(qkv, case))
    want = torch.empty(Hf * Wf, 32, dtype=torch.float64)
    for yi in range(Hf):
        for xi in range(Wf):
            y0, x0 = min(max(yi - 3, 0), Hf - 7), min(max(xi - 3, 0), Wf - 7)
            keys = [(yj, xj) for yj in range(y0, y0 + 7) for xj in range(x0, x0 + 7)]
            s = torch.stack([q[yi * Wf + xi] @ k[yj * Wf + xj] * 32 ** -0.5
                             + rpb.double().reshape(13, 13)[yj - yi + 6, xj - xi + 6] for yj, xj in keys])
            want[yi * Wf + xi] = torch.softmax(s, 0) @ torch.stack([v[yj * Wf + xj] for yj, xj in keys])
    got = ref.na_fwd(qkv.float(), rpb, H, Hf, Wf)[0].double()
    assert torch.allclose(got, want, rtol=2 ** -7, atol=2 ** -7)  # (P is a bf16 operand)
    assert float(F.cosine_similarity(got.flatten(), want.flatten(), 0)) > 0.9999


@pytest.mark.parametrize("case", ng.CASES)
def test_reference_alone_meets_the_float64_check(case):
    ng.check_against_float64(ref, CPU, case)


def test_reference_alone_meets_the_other_checks():
    for case in ng.LOCAL_CASES:
        ng.check_locality(ref, CPU, case)
    ng.check_refusals(ref, CPU)


def test_neighborhood_attention_plan_holds_its_invariants(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "nattn_plan_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-I", KDIR,
                        os.path.join(KDIR, "nattn_plan_check.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "nattn_plan_check sweep ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
