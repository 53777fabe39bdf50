"""ViT-B/16 and its op layer on the CPU: the attention oracle against
``torch.nn.MultiheadAttention``, torchvision's parameter layout, the registry, the checks of
``test_attention_gpu.py`` met by ``ref`` alone, and the launch-plan check program."""
import os
import shutil
import subprocess

import pytest
import torch

import test_attention_gpu as ag
from mpi_pytorch_amd.models import ATTN_ARCH, head_parameters, initialize_model
from mpi_pytorch_amd.models.vit import VisionTransformer
from mpi_pytorch_amd.ops import ref

CPU = torch.device("cpu")
KDIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc", "kernels")

LAYER0_AND_ENDS = [
    ("class_token", (1, 1, 768)), ("conv_proj.weight", (768, 3, 16, 16)), ("conv_proj.bias", (768,)),
    ("encoder.pos_embedding", (1, 197, 768)),
    ("encoder.layers.encoder_layer_0.ln_1.weight", (768,)),
    ("encoder.layers.encoder_layer_0.ln_1.bias", (768,)),
    ("encoder.layers.encoder_layer_0.self_attention.in_proj_weight", (2304, 768)),
    ("encoder.layers.encoder_layer_0.self_attention.in_proj_bias", (2304,)),
    ("encoder.layers.encoder_layer_0.self_attention.out_proj.weight", (768, 768)),
    ("encoder.layers.encoder_layer_0.self_attention.out_proj.bias", (768,)),
    ("encoder.layers.encoder_layer_0.ln_2.weight", (768,)),
    ("encoder.layers.encoder_layer_0.ln_2.bias", (768,)),
    ("encoder.layers.encoder_layer_0.mlp.0.weight", (3072, 768)),
    ("encoder.layers.encoder_layer_0.mlp.0.bias", (3072,)),
    ("encoder.layers.encoder_layer_0.mlp.3.weight", (768, 3072)),
    ("encoder.layers.encoder_layer_0.mlp.3.bias", (768,)),
    ("encoder.ln.weight", (768,)), ("encoder.ln.bias", (768,)),
    ("heads.head.weight", (1000, 768)), ("heads.head.bias", (1000,)),
]


@pytest.mark.parametrize("case", [(2, 3, 16), (1, 2, 17), (2, 2, 65)])
def test_oracle_matches_nn_multihead_attention(case):
    """Fixes the q/k/v row order of in_proj and the packed [B, S, 3, H, 64] layout."""
    B, H, S = case
    D = 64 * H
    torch.manual_seed(S)
    mha = torch.nn.MultiheadAttention(D, H, batch_first=True)
    x = torch.randn(B, S, D, requires_grad=True)
    dy = torch.randn(B, S, D)
    want = mha(x, x, x, need_weights=False)[0]
    want.backward(dy)
    with torch.no_grad():
        qkv = torch.nn.functional.linear(x, mha.in_proj_weight, mha.in_proj_bias)
        o, lse = ref.attn_fwd(qkv, H)
        y = torch.nn.functional.linear(o, mha.out_proj.weight, mha.out_proj.bias)
        dqkv = ref.attn_bwd(dy @ mha.out_proj.weight, qkv, o, lse, H)
    assert torch.allclose(y, want, rtol=2e-2, atol=2e-2)  # (P is a bf16 operand)
    dx = dqkv @ mha.in_proj_weight.detach()
    assert float(torch.nn.functional.cosine_similarity(dx.flatten(), x.grad.flatten(), 0)) > 0.9999
    dw = dqkv.reshape(-1, 3 * D).t() @ x.detach().reshape(-1, D)
    assert float(torch.nn.functional.cosine_similarity(dw.flatten(), mha.in_proj_weight.grad.flatten(), 0)) > 0.9999


def test_parameter_layout_is_torchvisions():
    assert list(ATTN_ARCH) == ["vit"]
    m = initialize_model("vit", 1000, False)[0]
    sd = m.state_dict()
    assert sum(v.numel() for v in sd.values()) == 86567656
    assert all(tuple(sd[k].shape) == s for k, s in LAYER0_AND_ENDS)
    keys = [k for k in sd if "encoder_layer_" not in k or "encoder_layer_0." in k]
    assert keys == [k for k, _ in LAYER0_AND_ENDS] and len(sd) == 4 + 12 * 12 + 4
    # left out of weight decay and trust ratio by --wd_exclude_1d
    assert m.class_token.dim() == 1 and m.encoder.pos_embedding.dim() == 1
    m2 = initialize_model("vit", 1000, False)[0]
    m2.load_state_dict(sd)
    sd2 = m2.state_dict()
    assert list(sd) == list(sd2) and all(torch.equal(sd[k], sd2[k]) for k in sd)
    w = m.conv_proj.weight
    assert torch.equal(w._mpa_import(w._mpa_export(w)), w)  # pad-channel columns are zero


def test_registry_replaces_the_head_and_trains():
    m = initialize_model("vit", 37, True)[0]
    head = list(head_parameters(m))
    assert [tuple(p.shape) for p in head] == [(64, 768), (64,)] and all(p.requires_grad for p in head)
    assert m.heads.head.out_features == 37 and not m.conv_proj.weight.requires_grad

    from mpi_pytorch_amd.parallel.arena import ParamArena
    torch.manual_seed(0)
    m = VisionTransformer(32, 16, 2, 2, 128, 256, 10)
    torch.nn.init.normal_(m.heads.head.weight, std=0.1)
    arena = ParamArena(m, CPU)
    loss = torch.nn.functional.cross_entropy(m(torch.randn(2, 32, 32, 3)), torch.tensor([1, 7]))
    loss.backward()
    g = arena.grad
    assert bool(torch.isfinite(loss)) and torch.isfinite(g).all()
    assert all(float(p.grad.abs().sum()) > 0 for p in m.parameters())


@pytest.mark.parametrize("case", ag.CASES)
def test_reference_alone_meets_the_attention_checks(case):
    ag.check_lookup(ref, CPU, *case)
    ag.check_rounding(ref, CPU, *case)
    if case in ag.UNIFORM_CASES:
        ag.check_uniform(ref, CPU, *case)


def test_reference_alone_meets_the_token_checks_and_refusals():
    ag.check_attn_refusals(ref, CPU)
    for case in ag.PATCH_CASES:
        ag.check_patchify(ref, CPU, *case)
    for case in ag.TOKEN_CASES:
        ag.check_tokens(ref, CPU, *case)


def test_attention_plan_holds_its_invariants(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "attn_plan_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-I", KDIR,
                        os.path.join(KDIR, "attn_plan_check.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "attn_plan_check sweep ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
