"""Swin-V2-T and its op layer on the CPU: the checks of ``test_wattn_cos_gpu.py`` met by ``ref``
alone, the cosine oracle against autograd through the composed formulation, torchvision's
parameter layout, and the registry.  (The launch-plan check program is built and run by ``test_swin_cpu.py``.)"""
import math

import pytest
import torch
import torch.nn.functional as F

import test_wattn_cos_gpu as cg
from mpi_pytorch_amd.models import WINDOW_V2_ARCH, initialize_model
from mpi_pytorch_amd.ops import ref

CPU = torch.device("cpu")

BLOCK0_AND_ENDS = [
    ("features.0.0.weight", (96, 3, 4, 4)), ("features.0.0.bias", (96,)),
    ("features.0.2.weight", (96,)), ("features.0.2.bias", (96,)),
    ("features.1.0.norm1.weight", (96,)), ("features.1.0.norm1.bias", (96,)),
    ("features.1.0.attn.logit_scale", (3, 1, 1)),
    ("features.1.0.attn.relative_coords_table", (1, 15, 15, 2)),
    ("features.1.0.attn.relative_position_index", (4096,)),
    ("features.1.0.attn.qkv.weight", (288, 96)), ("features.1.0.attn.qkv.bias", (288,)),
    ("features.1.0.attn.proj.weight", (96, 96)), ("features.1.0.attn.proj.bias", (96,)),
    ("features.1.0.attn.cpb_mlp.0.weight", (512, 2)), ("features.1.0.attn.cpb_mlp.0.bias", (512,)),
    ("features.1.0.attn.cpb_mlp.2.weight", (3, 512)),
    ("features.1.0.norm2.weight", (96,)), ("features.1.0.norm2.bias", (96,)),
    ("features.1.0.mlp.0.weight", (384, 96)), ("features.1.0.mlp.0.bias", (384,)),
    ("features.1.0.mlp.3.weight", (96, 384)), ("features.1.0.mlp.3.bias", (96,)),
    ("features.2.reduction.weight", (192, 384)), ("features.2.norm.weight", (192,)),
    ("features.2.norm.bias", (192,)),
    ("norm.weight", (768,)), ("norm.bias", (768,)), ("head.weight", (10, 768)), ("head.bias", (10,)),
]


@pytest.mark.parametrize("case", cg.CASES)
def test_reference_alone_meets_the_cosine_checks(case):
    cg.check_cos_against_float64(ref, CPU, case)


def test_reference_alone_meets_the_zero_row_check_and_refusals():
    cg.check_zero_row(ref, CPU)
    cg.check_cos_refusals(ref, CPU)


@pytest.mark.parametrize("H,ws", cg.CPB_CASES)
def test_reference_alone_meets_the_position_bias_checks(H, ws):
    cg.check_cpb(ref, CPU, H, ws)


@pytest.mark.parametrize("case", [(2, 3, 14, 14, 7, 3), (1, 2, 8, 8, 4, 1), (2, 2, 16, 8, 8, 0)])
def test_oracle_matches_the_composed_formulation(case):
    """roll -> partition -> normalise -> softmax -> reverse under autograd, in fp32: fixes the
    logit scale's clamp and gradient, the bias layout and the projection terms of dq and dk."""
    B, H, Hf, Wf, ws, shift = case
    S, C = ws * ws, 32 * H
    torch.manual_seed(Hf + shift)
    qkv = torch.randn(B * Hf * Wf, 3 * C, requires_grad=True)
    flat = (16 * torch.rand(H * (2 * ws - 1) ** 2)).requires_grad_()
    ls = torch.linspace(2.0, 5.0, H).requires_grad_()
    dy = torch.randn(B * Hf * Wf, C)
    q, k, v = ref.window_partition(qkv, Hf, Wf, ws, shift).reshape(-1, S, 3, H, 32).permute(2, 0, 3, 1, 4)
    attn = F.normalize(q, dim=-1) @ F.normalize(k, dim=-1).transpose(-2, -1)
    attn = attn * torch.clamp(ls, max=math.log(100.0)).exp().reshape(1, H, 1, 1)
    attn = attn + flat.reshape(H, -1)[:, ref.swin_relative_index(ws).flatten()].reshape(1, H, S, S)
    attn = attn + ref.swin_shift_mask(Hf, Wf, ws, shift).repeat(B, 1, 1)[:, None]
    want = ref.window_reverse((F.softmax(attn, -1) @ v).transpose(1, 2).reshape(-1, S, C), Hf, Wf, ws, shift)
    want.backward(dy)
    with torch.no_grad():
        o, lse = ref.wattn_cos_fwd(qkv, ls, flat, H, Hf, Wf, ws, shift)
        dflat, dls = torch.zeros_like(flat), torch.zeros_like(ls)
        dqkv = ref.wattn_cos_bwd(dy, qkv, lse, ls, flat, dflat, dls, H, Hf, Wf, ws, shift, True)
    cos = lambda a, g: float(F.cosine_similarity(a.flatten(), g.flatten(), 0))
    assert torch.allclose(o, want, rtol=2e-2, atol=2e-2)  # (P is a bf16 operand)
    assert cos(dqkv, qkv.grad) > 0.9999 and cos(dflat, flat.grad) > 0.9999
    assert float(dls[-1]) == 0 and float(ls.grad[-1]) == 0 and cos(dls[:-1], ls.grad[:-1]) > 0.9999


def test_parameter_layout_is_torchvisions():
    assert list(WINDOW_V2_ARCH) == ["swin_v2"] and WINDOW_V2_ARCH["swin_v2"][2] == 256
    m = initialize_model("swin_v2", 10, False)[0]
    sd = m.state_dict()
    # from the layer shapes (torchvision's published count for 1000 classes)
    n, dim = 96 * 48 + 96 + 2 * 96 + 2 * 768 + 768 * 1000 + 1000, 96
    for s, (depth, H) in enumerate(zip((2, 2, 6, 2), (3, 6, 12, 24))):
        n += depth * (4 * dim + H + 1536 + 512 * H + 3 * dim * dim + 3 * dim + dim * dim + dim + 8 * dim * dim + 5 * dim)
        if s < 3:
            n += 8 * dim * dim + 4 * dim
            dim *= 2
    assert n == 28351570
    buffers = ("relative_position_index", "relative_coords_table")
    assert sum(v.numel() for k, v in sd.items() if not k.endswith(buffers)) == n - 990 * 769
    assert all(tuple(sd[k].shape) == s for k, s in BLOCK0_AND_ENDS)
    keys = [k for k in sd if k.startswith(("features.0.", "features.1.0.", "features.2.", "norm.", "head."))]
    assert keys == [k for k, _ in BLOCK0_AND_ENDS] and len(sd) == 4 + 12 * 18 + 3 * 3 + 4
    attn = m.features[1][0].attn
    assert attn.logit_scale.dim() == 1 and torch.equal(attn.logit_scale, torch.full((3,), math.log(10.0)))
    assert [n for n, _ in attn.named_buffers()] == ["relative_coords_table", "relative_position_index"]
    for k, v in sd.items():  # the k third of every qkv bias
        if k.endswith("qkv.bias"):
            assert float(v[v.numel() // 3:2 * v.numel() // 3].abs().max()) == 0
    sd = {k: (torch.randn_like(v) if v.is_floating_point() and "relative" not in k else v) for k, v in sd.items()}
    m2 = initialize_model("swin_v2", 10, False)[0]
    m2.load_state_dict(sd)
    sd2 = m2.state_dict()
    for k in sd:  # a round trip, but for the k bias, which is held at zero
        third = sd[k].numel() // 3
        want = sd[k] if not k.endswith("qkv.bias") else torch.cat([sd[k][:third], torch.zeros(third), sd[k][2 * third:]])
        assert torch.equal(sd2[k], want), k
    assert list(sd) == list(sd2)


def test_forward_shape_at_256_on_the_cpu_path():
    torch.manual_seed(0)
    m = initialize_model("swin_v2", 10, False)[0]
    with torch.no_grad():
        y = m(torch.randn(1, 256, 256, 3))
    assert y.shape == (1, 10) and bool(torch.isfinite(y).all())
