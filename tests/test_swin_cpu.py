"""Swin-T and its op layer on the CPU: the window-attention oracle against autograd through the
published algorithm, torchvision's parameter layout, the registry, the checks of
``test_wattn_gpu.py`` met by ``ref`` alone, and the launch-plan check program."""
import os
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

import test_wattn_gpu as wg
from mpi_pytorch_amd.models import WINDOW_ARCH, head_parameters, initialize_model
from mpi_pytorch_amd.models.swin import SwinTransformer, _cells
from mpi_pytorch_amd.ops import ref

CPU = torch.device("cpu")
KDIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc", "kernels")

BLOCK0_AND_ENDS = [
    ("features.0.0.weight", (96, 3, 4, 4)), ("features.0.0.bias", (96,)),
    ("features.0.2.weight", (96,)), ("features.0.2.bias", (96,)),
    ("features.1.0.norm1.weight", (96,)), ("features.1.0.norm1.bias", (96,)),
    ("features.1.0.attn.relative_position_bias_table", (169, 3)),
    ("features.1.0.attn.relative_position_index", (2401,)),
    ("features.1.0.attn.qkv.weight", (288, 96)), ("features.1.0.attn.qkv.bias", (288,)),
    ("features.1.0.attn.proj.weight", (96, 96)), ("features.1.0.attn.proj.bias", (96,)),
    ("features.1.0.norm2.weight", (96,)), ("features.1.0.norm2.bias", (96,)),
    ("features.1.0.mlp.0.weight", (384, 96)), ("features.1.0.mlp.0.bias", (384,)),
    ("features.1.0.mlp.3.weight", (96, 384)), ("features.1.0.mlp.3.bias", (96,)),
    ("features.2.reduction.weight", (192, 384)), ("features.2.norm.weight", (384,)),
    ("features.2.norm.bias", (384,)),
    ("norm.weight", (768,)), ("norm.bias", (768,)), ("head.weight", (1000, 768)), ("head.bias", (1000,)),
]


def _published(x, wqkv, bqkv, table, index, H, ws, shift):
    """torchvision's shifted_window_attention up to the out-projection: x [B, Hf, Wf, C]."""
    B, Hf, Wf, C = x.shape
    S = ws * ws
    if shift:
        x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
    nw = (Hf // ws) * (Wf // ws)
    xw = x.view(B, Hf // ws, ws, Wf // ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B * nw, S, C)
    q, k, v = F.linear(xw, wqkv, bqkv).reshape(B * nw, S, 3, H, C // H).permute(2, 0, 3, 1, 4)
    attn = (q * (C // H) ** -0.5) @ k.transpose(-2, -1)
    attn = attn + table[index].view(S, S, H).permute(2, 0, 1).unsqueeze(0)
    if shift:
        attn = attn.view(B, nw, H, S, S) + ref.swin_shift_mask(Hf, Wf, ws, shift)[None, :, None]
        attn = attn.view(-1, H, S, S)
    o = (F.softmax(attn, -1) @ v).transpose(1, 2).reshape(B, Hf // ws, Wf // ws, ws, ws, C)
    o = o.permute(0, 1, 3, 2, 4, 5).reshape(B, Hf, Wf, C)
    return torch.roll(o, shifts=(shift, shift), dims=(1, 2)) if shift else o


@pytest.mark.parametrize("case", [(2, 3, 14, 14, 7, 3), (1, 2, 8, 8, 4, 1), (2, 2, 14, 7, 7, 0)])
def test_oracle_matches_the_published_algorithm(case):
    """Fixes the [3][H][32] column order, the table's head-major storage and the roll's sign."""
    B, H, Hf, Wf, ws, shift = case
    C = 32 * H
    torch.manual_seed(Hf + shift)
    x = torch.randn(B, Hf, Wf, C, requires_grad=True)
    w, b = (torch.randn(3 * C, C) * C ** -0.5).requires_grad_(), torch.randn(3 * C).requires_grad_()
    table = (torch.randn((2 * ws - 1) ** 2, H) * 0.5).requires_grad_()
    dy = torch.randn(B * Hf * Wf, C)
    want = _published(x, w, b, table, ref.swin_relative_index(ws).flatten(), H, ws, shift).reshape(-1, C)
    want.backward(dy)
    with torch.no_grad():
        flat = table.t().reshape(-1)  # the model's storage
        qkv = F.linear(x.reshape(-1, C), w, b)
        o, lse = ref.wattn_fwd(qkv, flat, H, Hf, Wf, ws, shift)
        dflat = torch.zeros_like(flat)
        dqkv = ref.wattn_bwd(dy, qkv, lse, flat, dflat, H, Hf, Wf, ws, shift, True)
    cos = lambda a, g: float(F.cosine_similarity(a.flatten(), g.flatten(), 0))
    assert torch.allclose(o, want, rtol=2e-2, atol=2e-2)  # (P is a bf16 operand)
    assert cos(dqkv @ w.detach(), x.grad) > 0.9999 and cos(dqkv.t() @ x.detach().reshape(-1, C), w.grad) > 0.9999
    assert cos(dflat.reshape(H, -1).t(), table.grad) > 0.9999


def test_closed_form_rel_is_the_index_buffer():
    m = SwinTransformer(4, 64, (1,), (2,), 4, 10)
    buf = m.features[1][0].attn.relative_position_index
    ys, xs = torch.arange(16) // 4, torch.arange(16) % 4
    rel = (ys[:, None] - ys[None] + 3) * 7 + (xs[:, None] - xs[None] + 3)
    assert buf.dtype == torch.int64 and torch.equal(buf, rel.flatten())
    assert sorted(set(buf.tolist())) == list(range(49))


def test_parameter_layout_is_torchvisions():
    assert list(WINDOW_ARCH) == ["swin"]
    m = initialize_model("swin", 1000, False)[0]
    sd = m.state_dict()
    # from the layer shapes (torchvision's published count)
    n, dim = 96 * 48 + 96 + 2 * 96 + 2 * 768 + 768 * 1000 + 1000, 96
    for s, (depth, H) in enumerate(zip((2, 2, 6, 2), (3, 6, 12, 24))):
        n += depth * (4 * dim + 169 * H + 3 * dim * dim + 3 * dim + dim * dim + dim + 8 * dim * dim + 5 * dim)
        if s < 3:
            n += 8 * dim * dim + 8 * dim
            dim *= 2
    assert n == 28288354 and sum(p.numel() for p in m.parameters()) >= n  # (stored with pad rows)
    assert sum(v.numel() for k, v in sd.items() if "relative_position_index" not in k) == n
    assert all(tuple(sd[k].shape) == s for k, s in BLOCK0_AND_ENDS)
    keys = [k for k in sd if k.startswith(("features.0.", "features.1.0.", "features.2.", "norm.", "head."))]
    assert keys == [k for k, _ in BLOCK0_AND_ENDS] and len(sd) == 4 + 12 * 14 + 3 * 3 + 4
    # left out of weight decay and trust ratio by --wd_exclude_1d; the index is no parameter
    attn = m.features[1][0].attn
    assert attn.relative_position_bias_table.dim() == 1
    assert [n for n, _ in attn.named_buffers()] == ["relative_position_index"]
    m2 = initialize_model("swin", 1000, False)[0]
    m2.load_state_dict(sd)
    sd2 = m2.state_dict()
    assert list(sd) == list(sd2) and all(torch.equal(sd[k], sd2[k]) for k in sd)
    assert torch.equal(m2.features[2].reduction.weight, m.features[2].reduction.weight)


def test_patch_merge_permutation_round_trips():
    """The merged rows times the stored weight equal torchvision's concat times the exported one."""
    torch.manual_seed(2)
    merge = SwinTransformer(4, 64, (1, 1), (2, 4), 4, 10).features[2]
    w = merge.reduction.weight
    assert torch.equal(w._mpa_import(w._mpa_export(w)), w) and torch.equal(_cells(_cells(w)), w)
    x = torch.randn(2, 8, 8, 64)
    tv = torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1).reshape(-1, 256)
    ours = ref.patchify(x, 2)
    assert torch.equal(_cells(ours), tv)
    assert torch.allclose(ours @ w.t(), tv @ merge.state_dict()["reduction.weight"].t(), rtol=1e-5, atol=1e-5)


def test_registry_replaces_the_head_and_trains():
    m = initialize_model("swin", 37, True)[0]
    head = list(head_parameters(m))
    assert [tuple(p.shape) for p in head] == [(64, 768), (64,)] and all(p.requires_grad for p in head)
    assert m.head.out_features == 37 and not m.features[0][0].weight.requires_grad

    from mpi_pytorch_amd.parallel.arena import ParamArena
    torch.manual_seed(0)
    m = SwinTransformer(4, 64, (2, 1), (2, 4), 4, 10)
    arena = ParamArena(m, CPU)
    loss = F.cross_entropy(m(torch.randn(2, 32, 32, 3)), torch.tensor([1, 7]))
    loss.backward()
    assert bool(torch.isfinite(loss)) and torch.isfinite(arena.grad).all()
    assert all(float(p.grad.abs().sum()) > 0 for p in m.parameters())


@pytest.mark.parametrize("case", wg.CASES)
def test_reference_alone_meets_the_window_attention_checks(case):
    wg.check_against_float64(ref, CPU, case)
    if case[0] * case[2] * case[3] > case[4] ** 2 or case[5]:
        wg.check_window_isolation(ref, CPU, case)


def test_reference_alone_meets_the_exact_checks_and_refusals():
    for case in wg.UNIFORM_CASES:
        wg.check_uniform(ref, CPU, case)
    wg.check_wattn_refusals(ref, CPU)
    for case in wg.UNPATCH_CASES:
        wg.check_unpatchify(ref, CPU, *case)


def test_window_attention_plan_holds_its_invariants(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "wattn_plan_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-I", KDIR,
                        os.path.join(KDIR, "wattn_plan_check.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "wattn_plan_check sweep ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
