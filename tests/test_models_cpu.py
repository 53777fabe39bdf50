"""Model zoo on the CPU path: torchvision parameter names/shapes/counts, head replacement,
feature-extract freezing, and exact fp32 parity of forward+backward against an
independent NCHW implementation built from plain torch.nn.functional calls."""
import pytest
import torch
import torch.nn.functional as F

from mpi_pytorch_amd.models import initialize_model, ARCH
from mpi_pytorch_amd.engine import build_model, build_training, loss_fn
from mpi_pytorch_amd.parallel import World

# torchvision totals at 1000 classes
TV_PARAMS_1000 = {"resnet18": 11689512, "resnet34": 21797672, "alexnet": 61100840,
                  "vgg": 132868840, "squeezenet": 1248424, "densenet": 7978856,
                  "inception": 27161264, "vgg16": 138357544}
# at 64,500 classes
TV_PARAMS_64500 = {"resnet18": 44265012, "resnet34": 54373172, "alexnet": 321260340,
                   "vgg": 393028340, "squeezenet": 33823924, "densenet": 73066356,
                   "inception": 206104264, "vgg16": 398517044}
N_PARAM_TENSORS = {"resnet18": 62, "resnet34": 110, "alexnet": 16, "vgg": 38, "squeezenet": 52,
                   "densenet": 364, "inception": 292, "vgg16": 32}


def _sd_params(model):
    sd = model.state_dict()
    names = {n for n, _ in model.named_parameters()}
    return {k: v for k, v in sd.items() if k in names}


@pytest.mark.parametrize("name", list(ARCH))
def test_param_counts_match_torchvision(name):
    m, _ = initialize_model(name, 1000, False)
    ps = _sd_params(m)
    assert sum(v.numel() for v in ps.values()) == TV_PARAMS_1000[name]
    assert len(ps) == N_PARAM_TENSORS[name]


@pytest.mark.parametrize("name", ["resnet18", "squeezenet", "densenet", "alexnet"])
def test_head_replacement_64500(name):
    m, isz = initialize_model(name, 64500, False)
    assert sum(v.numel() for v in _sd_params(m).values()) == TV_PARAMS_64500[name]
    assert isz == ARCH[name][2]


def test_input_sizes():
    assert initialize_model("resnet34", 10, False)[1] == 128
    assert initialize_model("inception", 10, False)[1] == 299
    with pytest.raises(ValueError):
        initialize_model("lenet", 10, False)


def test_state_dict_layout_resnet18():
    m, _ = initialize_model("resnet18", 64500, False)
    sd = m.state_dict()
    assert len(sd) == 122
    assert sd["conv1.weight"].shape == (64, 3, 7, 7)
    assert sd["layer2.0.downsample.0.weight"].shape == (128, 64, 1, 1)
    assert sd["fc.weight"].shape == (64500, 512)
    assert sd["bn1.num_batches_tracked"].dtype == torch.long
    # round trip
    m2, _ = initialize_model("resnet18", 64500, False)
    m2.load_state_dict(sd)
    for k, v in m2.state_dict().items():
        assert torch.equal(v, sd[k]), k


def test_vgg_flatten_layout_roundtrip():
    m, _ = initialize_model("vgg", 10, False)
    sd = m.state_dict()
    assert sd["classifier.0.weight"].shape == (4096, 25088)
    m2, _ = initialize_model("vgg", 10, False)
    m2.load_state_dict(sd)
    assert torch.equal(m2.state_dict()["classifier.0.weight"], sd["classifier.0.weight"])


def test_feature_extract_freezes_all_but_head():
    m, _ = initialize_model("resnet18", 100, True)
    trainable = [n for n, p in m.named_parameters() if p.requires_grad]
    assert trainable == ["fc.weight", "fc.bias"]


# ------------------------------------------------------------- independent NCHW oracle
def _ref_resnet18(sd, x_nchw):
    def bn(x, p):
        return F.batch_norm(x, None, None, sd[p + ".weight"], sd[p + ".bias"], True, 0.1, 1e-5)

    x = F.relu(bn(F.conv2d(x_nchw, sd["conv1.weight"], stride=2, padding=3), "bn1"))
    x = F.max_pool2d(x, 3, 2, 1)
    for li, stride in zip(range(1, 5), (1, 2, 2, 2)):
        for b in range(2):
            pre = "layer%d.%d." % (li, b)
            s = stride if b == 0 else 1
            out = F.relu(bn(F.conv2d(x, sd[pre + "conv1.weight"], stride=s, padding=1), pre + "bn1"))
            out = bn(F.conv2d(out, sd[pre + "conv2.weight"], padding=1), pre + "bn2")
            if pre + "downsample.0.weight" in sd:
                x = bn(F.conv2d(x, sd[pre + "downsample.0.weight"], stride=s), pre + "downsample.1")
            x = F.relu(out + x)
    x = F.adaptive_avg_pool2d(x, 1).flatten(1)
    return F.linear(x, sd["fc.weight"], sd["fc.bias"])


def test_resnet18_cpu_matches_functional_oracle():
    torch.manual_seed(0)
    m, _ = build_model("resnet18", 10, False, torch.device("cpu"), World())
    sd = {k: v.clone().requires_grad_(v.dtype.is_floating_point and "running" not in k)
          for k, v in m.state_dict().items()}
    x = torch.randn(4, 64, 64, 3)
    y = torch.randint(0, 10, (4,))
    loss = loss_fn(m(x), y)
    loss.backward()
    lr = F.cross_entropy(_ref_resnet18(sd, x.permute(0, 3, 1, 2)), y)
    lr.backward()
    assert abs(float(loss) - float(lr)) < 1e-4
    ours = {n: p.grad for n, p in m.named_parameters()}
    exp = m.conv1._exp  # internal KRSC -> OIHW
    assert torch.allclose(exp(ours["conv1.weight"]), sd["conv1.weight"].grad, atol=1e-4, rtol=1e-3)
    assert torch.allclose(m.layer3[0].conv1._exp(ours["layer3.0.conv1.weight"]),
                          sd["layer3.0.conv1.weight"].grad, atol=1e-4, rtol=1e-3)
    # the classifier stores its output dim padded to a multiple of 32 (zero rows)
    assert torch.allclose(m.fc._exp(ours["fc.weight"]), sd["fc.weight"].grad, atol=1e-5, rtol=1e-4)
    assert torch.allclose(m.fc._exp_bias(ours["fc.bias"]), sd["fc.bias"].grad, atol=1e-5, rtol=1e-4)
    assert float(ours["fc.weight"][10:].abs().max()) == 0.0  # padded rows get no gradient
    assert torch.allclose(ours["layer2.0.bn1.weight"], sd["layer2.0.bn1.weight"].grad, atol=1e-4,
                          rtol=1e-3)


@pytest.mark.parametrize("name,hw", [("alexnet", 95), ("squeezenet", 64), ("vgg16", 32),
                                     ("densenet", 32), ("inception", 299)])
def test_models_train_step_cpu(name, hw):
    torch.manual_seed(0)
    m, _ = build_model(name, 20, False, torch.device("cpu"), World())
    x = torch.randn(2, hw, hw, 3)
    y = torch.randint(0, 20, (2,))
    out = m(x)
    if name == "inception":
        assert isinstance(out, tuple) and out[1].shape == (2, 20)
    loss = loss_fn(out, y)
    loss.backward()
    g = m._mpa_arena.grad
    assert torch.isfinite(g).all() and float(g.abs().sum()) > 0
    m.eval()
    with torch.no_grad():
        assert m(x).shape == (2, 20)


def _block_grads(join_on: bool):
    from mpi_pytorch_amd.models import resnet as R
    prev = R._JOIN
    R._JOIN = join_on
    try:
        torch.manual_seed(0)
        ds = R.Downsample(R.Conv2d(8, 16, 1, 2, 0, bias=False), R.BatchNorm2d(16))
        blocks = torch.nn.Sequential(R.BasicBlock(8, 8), R.BasicBlock(8, 16, 2, ds)).train()
        from mpi_pytorch_amd.parallel import ParamArena
        ParamArena(blocks, "cpu")  # weight gradients land in the flat arena (as in training)
        x = torch.randn(2, 10, 10, 8, requires_grad=True)
        out = blocks(x)
        (out.float() * torch.linspace(-1, 1, out.numel()).view_as(out)).sum().backward()
        return [x.grad.clone()] + [p.grad.clone() for p in blocks.parameters()]
    finally:
        R._JOIN = prev


def test_residual_grad_join_matches_autograd_sum():
    """GradJoin (residual-input gradients summed inside the second dgrad's epilogue)
    gives the same gradients as autograd's separate add, for the identity shortcut and
    the 1x1/s2 downsample shortcut."""
    a = _block_grads(True)
    b = _block_grads(False)
    assert len(a) == len(b)
    for ga, gb in zip(a, b):
        assert torch.allclose(ga, gb, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("order", ["ds_first", "conv_first"])
def test_grad_join_order_independent(order):
    """The deferred-dgrad protocol sums both contributions whichever op autograd runs
    first, and the fresh launch is the full-coverage 3x3/s2 dgrad."""
    from mpi_pytorch_amd.ops import functional as Fn
    from mpi_pytorch_amd.ops import ref
    from mpi_pytorch_amd.models.layers import Conv2d
    torch.manual_seed(1)
    c3 = Conv2d(8, 16, 3, 2, 1, bias=False)
    c1 = Conv2d(8, 16, 1, 2, 0, bias=False)
    w3 = torch.randn(16, 3, 3, 8)
    w1 = torch.randn(16, 1, 1, 8)
    dz = torch.randn(2, 5, 5, 16)
    exp = ref.conv_dgrad(dz, w3, 10, 10, 2, 2, 1, 1) + ref.conv_dgrad(dz, w1, 10, 10, 2, 2, 0, 0)
    j = Fn.GradJoin()
    calls = [(w3, c3), (w1, c1)] if order == "conv_first" else [(w1, c1), (w3, c3)]
    r0 = j.add(ref, Fn._Dgrad(ref, dz, calls[0][0], None, calls[0][1], (10, 10)))
    assert r0 is None and j.partial is not None
    r1 = j.add(ref, Fn._Dgrad(ref, dz, calls[1][0], None, calls[1][1], (10, 10)))
    assert j.partial is None
    assert torch.allclose(r1, exp, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("k,s,p,hw", [(7, 2, 3, (32, 32)), (7, 2, 3, (33, 35)), (7, 2, 0, (31, 30)),
                                      (3, 2, 0, (29, 31)), (4, 2, 1, (20, 22))])
def test_pixel_pair_stem_matches_conv2d(k, s, p, hw):
    """Pixel-pair stem (4-channel canvas viewed as 8-channel pixel pairs, stride-1 conv
    with a ceil(S/2)-wide kernel) == the image conv, forward and weight gradient, from
    both a raw 3-channel image and the pre-padded canvas of input_spec."""
    from mpi_pytorch_amd.models.layers import Conv2d
    from mpi_pytorch_amd.parallel import ParamArena
    from mpi_pytorch_amd.ops import functional as Fn
    from mpi_pytorch_amd.ops import ref
    torch.manual_seed(0)
    conv = Conv2d(3, 16, k, s, p, bias=False)
    assert conv.pair
    ParamArena(torch.nn.ModuleList([conv]), "cpu")
    w = conv.state_dict()["weight"]  # OIHW [16, 3, k, k]
    H, W = hw
    x = torch.randn(2, H, W, 3)
    y_ref = F.conv2d(x.permute(0, 3, 1, 2), w, stride=s, padding=p)
    # raw image path (converted by fit_input)
    conv.weight.grad.zero_()
    y = Fn.conv_act(x, conv)
    assert torch.allclose(y.permute(0, 3, 1, 2), y_ref, atol=1e-4, rtol=1e-4)
    # canvas path: what the preprocess kernel writes
    spec = conv.input_spec(hw)
    t, b, l, r = spec["pad"]
    canvas = F.pad(F.pad(x, (0, 1)), (0, 0, l, r, t, b))
    y2 = Fn.conv_act(canvas, conv)
    assert torch.equal(y2, y)
    # weight gradient through the pair layout, exported back to OIHW
    g = torch.randn_like(y)
    (y * g).sum().backward()
    xr = x.permute(0, 3, 1, 2).clone().requires_grad_(False)
    wr = w.clone().requires_grad_(True)
    (F.conv2d(xr, wr, stride=s, padding=p) * g.permute(0, 3, 1, 2)).sum().backward()
    gw = conv._exp(conv.weight.grad)
    assert torch.allclose(gw, wr.grad, atol=1e-3, rtol=1e-3)
    # the stored padding (4th channel; column past an odd kernel) holds exactly zero grad
    full = conv.weight.grad.view(16, k, conv.sp, 2, 4)
    assert float(full[..., 3].abs().max()) == 0.0
    if k % 2:
        assert float(full[:, :, -1, 1].abs().max()) == 0.0
    # preprocess writes the same canvas
    img = torch.randint(0, 256, (2, H, W, 3), dtype=torch.uint8)
    a = ref.preprocess(img, H, W, [0.5] * 3, [0.25] * 3, 0, 4, torch.float32, spec["pad"])
    b_ = F.pad(F.pad(ref.preprocess(img, H, W, [0.5] * 3, [0.25] * 3, 0, 3, torch.float32),
                     (0, 1)), (0, 0, l, r, t, b))
    assert torch.equal(a, b_)


def test_pixel_pair_stem_state_dict_roundtrip():
    from mpi_pytorch_amd.models.layers import Conv2d
    conv = Conv2d(3, 8, 7, 2, 3, bias=False)
    w = torch.randn(8, 3, 7, 7)
    conv.load_state_dict({"weight": w})
    assert torch.equal(conv.state_dict()["weight"], w)
    assert tuple(conv.weight.shape) == (8, 7, 4, 8)


def test_whole_model_gradients_are_shattered_in_fp32():
    """Why model-level gradient DIRECTION cannot be a tight GPU check (docs/NOTES.md
    "Numerics", utils/parity.py): on the CPU, in fp32, rounding only the input image to bf16
    already turns ResNet-34's weight gradient by cos ~0.94 (Inception-v3 ~0.4), while 1e-6
    noise leaves it at 0.9995.  The GPU tests therefore compare per unit, teacher-forced
    (tests/test_layer_parity_gpu.py)."""
    from mpi_pytorch_amd.engine import build_model, loss_fn
    from mpi_pytorch_amd.parallel import World
    torch.manual_seed(0)
    m, _ = build_model("resnet34", 40, False, torch.device("cpu"), World())
    torch.manual_seed(1)
    x = torch.randn(4, 64, 64, 3) * 0.5
    y = torch.randint(0, 40, (4,))

    def grad(xx):
        m._mpa_arena.grad.zero_()
        for mod in m.modules():
            if getattr(mod, "running_mean", None) is not None:
                mod.running_mean.zero_()
                mod.running_var.fill_(1.0)
        loss_fn(m(xx), y).backward()
        return m._mpa_arena.grad.clone()

    g0 = grad(x)
    cos = lambda a, b: float(F.cosine_similarity(a, b, dim=0))
    c_bf16 = cos(g0, grad(x.to(torch.bfloat16).float()))
    c_tiny = cos(g0, grad(x * (1 + 1e-6 * torch.randn_like(x))))
    assert c_tiny > 0.999 and c_bf16 < 0.99, (c_tiny, c_bf16)


def test_inception_pool_branch_commutes_with_conv(monkeypatch):
    """PoolBranch runs avg_pool(conv1x1(x)) instead of conv1x1(avg_pool(x)) (both linear,
    count_include_pad): output, input gradient and parameter gradients equal the
    torchvision order (MPA_POOL_FIRST) to fp32 rounding, with BN in train mode."""
    import mpi_pytorch_amd.models.inception as I
    from mpi_pytorch_amd.parallel import ParamArena
    torch.manual_seed(0)
    m = I.PoolBranch(64, 32, 1)
    m._mpa_arena = ParamArena(m, torch.device("cpu"))
    m.train()
    x = torch.randn(4, 9, 9, 64, requires_grad=True)
    outs = []
    for first in (False, True):
        monkeypatch.setattr(I, "_POOL_FIRST", first)
        x.grad = None
        m._mpa_arena.zero_grad()
        y = m(x)
        y.backward(torch.linspace(-1, 1, y.numel()).view_as(y))
        outs.append((y.detach(), x.grad.clone(), m._mpa_arena.grad.clone()))
    for a, b in zip(*outs):
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-4 * float(b.abs().max()))


def test_inception_grouped_heads_equal_separate_convs():
    """Inception's 1x1 branch heads as ONE grouped GEMM (weights back to back in the arena,
    per-branch BN on channel windows, one wgrad / dgrad) == the separate BasicConv2d's, in
    fp32 on the CPU: same logits, same running statistics, gradients to fp32 rounding."""
    import mpi_pytorch_amd.ops.functional as Fn
    torch.manual_seed(0)
    model, _o, _s, _ = build_training("inception", 10, torch.device("cpu"), World(), 1e-3)
    model.dropout.p = 0.0
    a = model._mpa_arena
    heads = [m for m in model.modules() if hasattr(m, "heads")]
    assert len(heads) == 10
    for m in heads:  # every group is one flat arena range
        assert a.flat_view([h.conv.weight for h in m.heads()], "grad") is not None
    x = torch.randn(2, 299, 299, 8) * (torch.arange(8) < 3)
    y = torch.randint(0, 10, (2,))
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    res = []
    for merged in (True, False):
        for m in heads:
            m.merge_1x1 = merged
        model.load_state_dict(sd)
        a.zero_grad()
        out = model(x)
        loss_fn(out, y).backward()
        res.append((out[0].detach(), a.grad.clone(),
                    [v.clone() for k, v in model.state_dict().items() if "running" in k]))
    (o1, g1, r1), (o2, g2, r2) = res
    assert torch.allclose(o1, o2, atol=1e-5)
    assert all(torch.allclose(u, v, atol=1e-5) for u, v in zip(r1, r2))
    assert float((g1 - g2).abs().max()) < 1e-5 * float(g2.abs().max())


@pytest.mark.parametrize("defer", [True, False])
def test_densenet_feature_buffer_blocks_equal_plain_autograd(monkeypatch, defer):
    """DenseNet blocks on one feature buffer (norm1 on the channel prefix with per-feature
    statistics taken once, input gradients added into one accumulator - with the deferred
    per-channel norm1 corrections, or the per-layer BN backward) == per-layer concat + plain
    autograd, in fp32 on the CPU (train and eval forward, gradients, running statistics)."""
    from mpi_pytorch_amd.models import densenet as dn
    monkeypatch.setattr(dn, "_DEFER", defer)
    torch.manual_seed(0)
    model, _o, _s, _ = build_training("densenet", 10, torch.device("cpu"), World(), 1e-3)
    a = model._mpa_arena
    x = torch.randn(2, 64, 64, 8) * (torch.arange(8) < 3)
    y = torch.randint(0, 10, (2,))
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    res = []
    for fused in (True, False):
        model.fused_blocks = fused
        model.load_state_dict(sd)
        model.train()
        a.zero_grad()
        out = model(x)
        loss_fn(out, y).backward()
        model.eval()
        with torch.no_grad():
            ev = model(x)
        res.append((out.detach(), ev, a.grad.clone(),
                    [v.clone() for k, v in model.state_dict().items() if "running" in k]))
    (o1, e1, g1, r1), (o2, e2, g2, r2) = res
    assert torch.allclose(o1, o2, atol=1e-5) and torch.allclose(e1, e2, atol=1e-5)
    assert all(torch.allclose(u, v, atol=1e-5) for u, v in zip(r1, r2))
    assert float((g1 - g2).abs().max()) < 1e-5 * float(g2.abs().max())


def test_densenet_direct_layer_walk_equals_nested_backward(monkeypatch):
    """Each dense layer's backward by calling its chain of backward nodes directly
    (densenet._walk_backward) == a nested torch.autograd.backward per layer, bitwise."""
    from mpi_pytorch_amd.models import densenet as dn
    torch.manual_seed(0)
    model, _o, _s, _ = build_training("densenet", 10, torch.device("cpu"), World(), 1e-3)
    a = model._mpa_arena
    x = torch.randn(2, 64, 64, 8) * (torch.arange(8) < 3)
    y = torch.randint(0, 10, (2,))
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    res = []
    walked = []
    real = dn._walk_backward
    monkeypatch.setattr(dn, "_walk_backward", lambda n, g: walked.append(1) or real(n, g))
    for walk in (True, False):
        monkeypatch.setattr(dn, "_WALK", walk)
        model.load_state_dict(sd)
        a.zero_grad()
        loss_fn(model(x), y).backward()
        res.append(a.grad.clone())
    assert len(walked) == 58  # every layer took the direct walk
    assert torch.equal(res[0], res[1])


def test_inception_fused_stem_pools_equal_modules():
    """Conv2d_2b -> maxpool1 and Conv2d_4a -> maxpool2 as fused conv+BN+ReLU+max-pool ops ==
    the BasicConv2d + MaxPool2d modules (fp32, CPU): logits, running stats, gradients."""
    torch.manual_seed(0)
    model, _o, _s, _ = build_training("inception", 10, torch.device("cpu"), World(), 1e-3)
    model.dropout.p = 0.0
    a = model._mpa_arena
    x = torch.randn(2, 299, 299, 8) * (torch.arange(8) < 3)
    y = torch.randint(0, 10, (2,))
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    res = []
    for fused in (True, False):
        model.fuse_stem_pools = fused
        model.load_state_dict(sd)
        a.zero_grad()
        out = model(x)
        loss_fn(out, y).backward()
        res.append((out[0].detach(), a.grad.clone(),
                    [v.clone() for k, v in model.state_dict().items() if "running" in k]))
    (o1, g1, r1), (o2, g2, r2) = res
    assert torch.allclose(o1, o2, atol=1e-5)
    assert all(torch.allclose(u, v, atol=1e-5) for u, v in zip(r1, r2))
    assert float((g1 - g2).abs().max()) < 1e-5 * float(g2.abs().max())


def test_densenet_transition_pool_first_equals_torchvision_order(monkeypatch):
    """The transition's average pool commuted ahead of its bias-free 1x1 conv (both linear)
    gives torchvision's norm -> relu -> conv -> pool output and gradients (fp32, CPU)."""
    from mpi_pytorch_amd.models import densenet as dn
    torch.manual_seed(0)
    model, _o, _s, _ = build_training("densenet", 10, torch.device("cpu"), World(), 1e-3)
    tr = model.features.transition1
    x0 = torch.randn(2, 8, 8, tr.norm.num_features)
    res = []
    for first in (True, False):
        monkeypatch.setattr(dn, "_POOL_FIRST", first)
        model._mpa_arena.zero_grad()
        x = x0.clone().requires_grad_(True)
        y = tr(x)
        y.square().sum().backward()
        res.append((y.detach(), x.grad.clone(), model._mpa_arena.grad.clone()))
    (y1, gx1, g1), (y2, gx2, g2) = res
    assert torch.allclose(y1, y2, atol=1e-5, rtol=1e-5)
    assert torch.allclose(gx1, gx2, atol=1e-5, rtol=1e-4)
    assert float((g1 - g2).abs().max()) < 1e-4 * float(g2.abs().max())


def test_resnet_deferred_downsample_bn_equals_materialized(monkeypatch):
    """The downsample BN applied by bn2 while it reads the residual (Fn.BNDefer: statistics
    half only in the downsample op) == the materialized downsample BN output: logits,
    gradients, running statistics and num_batches_tracked (fp32, CPU)."""
    from mpi_pytorch_amd.models import resnet as rn
    torch.manual_seed(0)
    model, _o, _s, _ = build_training("resnet18", 10, torch.device("cpu"), World(), 1e-3)
    a = model._mpa_arena
    x = torch.randn(2, 64, 64, 3)
    y = torch.randint(0, 10, (2,))
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    res = []
    for defer in (True, False):
        monkeypatch.setattr(rn, "_DS_DEFER", defer)
        model.load_state_dict(sd)
        model.train()
        a.zero_grad()
        out = model(x)
        loss_fn(out, y).backward()
        res.append((out.detach(), a.grad.clone(),
                    [v.clone() for k, v in model.state_dict().items()
                     if "running" in k or "num_batches" in k]))
    (o1, g1, r1), (o2, g2, r2) = res
    assert torch.allclose(o1, o2, atol=1e-5)
    assert all(torch.allclose(u.float(), v.float(), atol=1e-5) for u, v in zip(r1, r2))
    assert float((g1 - g2).abs().max()) < 1e-5 * float(g2.abs().max())


def test_resnet_dgrad_pair_equals_two_dgrads(monkeypatch):
    """Each residual stage's conv1 (3x3/s2) and 1x1/s2 shortcut dgrads merged into one
    launch (Fn._dgrad_pair -> conv_dgrad_pair; 3 per ResNet-18 step) == the two separate
    dgrads summed by GradJoin (fp32, CPU)."""
    from mpi_pytorch_amd.ops import functional as Fn
    from mpi_pytorch_amd.ops import ref
    torch.manual_seed(0)
    model, _o, _s, _ = build_training("resnet18", 10, torch.device("cpu"), World(), 1e-3)
    a = model._mpa_arena
    x = torch.randn(2, 64, 64, 3)
    y = torch.randint(0, 10, (2,))
    calls = []
    real = ref.conv_dgrad_pair

    def counting(*args, **kw):
        r = real(*args, **kw)
        calls.append(r is not None)
        return r

    monkeypatch.setattr(ref, "conv_dgrad_pair", counting)
    grads = []
    for pair in (True, False):
        monkeypatch.setattr(Fn, "_PAIR", pair)
        a.zero_grad()
        loss_fn(model(x), y).backward()
        grads.append(a.grad.clone())
    assert calls == [True, True, True]
    g1, g2 = grads
    assert float((g1 - g2).abs().max()) < 1e-5 * float(g2.abs().max())


def test_resnet_masked_shortcut_gradient_equals_written(monkeypatch):
    """Identity blocks hand their shortcut gradient to conv1's dgrad unwritten (_MaskedRes:
    conv_dgrad_res adds dy * mask in its epilogue; 5 per ResNet-18 step) == bn2's backward
    writing g and conv1's dgrad accumulating into it (fp32, CPU)."""
    from mpi_pytorch_amd.ops import functional as Fn
    from mpi_pytorch_amd.ops import ref
    torch.manual_seed(0)
    model, _o, _s, _ = build_training("resnet18", 10, torch.device("cpu"), World(), 1e-3)
    a = model._mpa_arena
    x = torch.randn(2, 64, 64, 3)
    y = torch.randint(0, 10, (2,))
    calls = []
    real = ref.conv_dgrad_res
    monkeypatch.setattr(ref, "conv_dgrad_res", lambda *t: calls.append(1) or real(*t))
    grads = []
    for on in (True, False):
        monkeypatch.setattr(Fn, "_RES_MASK", on)
        a.zero_grad()
        loss_fn(model(x), y).backward()
        grads.append(a.grad.clone())
    assert len(calls) == 5
    g1, g2 = grads
    assert float((g1 - g2).abs().max()) < 1e-5 * float(g2.abs().max())


def test_resnet_bn_pair_backward_equals_separate(monkeypatch):
    """bn2 + the deferred downsample BN backwarded together (bn_bwd_pair: one reduce and
    one apply pass, g never written; 3 per ResNet-18 step) == bn2's backward handing g to
    the downsample op's own BN backward: gradients incl. both BNs' affine gradients."""
    from mpi_pytorch_amd.ops import functional as Fn
    from mpi_pytorch_amd.ops import ref
    torch.manual_seed(0)
    model, _o, _s, _ = build_training("resnet18", 10, torch.device("cpu"), World(), 1e-3)
    a = model._mpa_arena
    x = torch.randn(2, 64, 64, 3)
    y = torch.randint(0, 10, (2,))
    calls = []
    real = ref.bn_bwd_pair
    monkeypatch.setattr(ref, "bn_bwd_pair", lambda *t: calls.append(1) or real(*t))
    grads = []
    for pair in (True, False):
        monkeypatch.setattr(Fn, "_BN_PAIR", pair)
        a.zero_grad()
        loss_fn(model(x), y).backward()
        grads.append(a.grad.clone())
    assert len(calls) == 3
    g1, g2 = grads
    assert float((g1 - g2).abs().max()) < 1e-5 * float(g2.abs().max())


def test_feature_stack_links_match_unlinked():
    """FusedSequential's conv -> ReLU -> conv / 2x2 max-pool hand-offs (the consumer's
    backward applies the producer's ReLU mask / BN reduction, no act_bwd or reduce pass)
    give the same
    gradients as the unlinked form, for plain ReLU (VGG-16 / AlexNet) and BN+ReLU
    (VGG11_bn) producers."""
    import mpi_pytorch_amd.models.layers as L
    from mpi_pytorch_amd.models.layers import (Conv2d, BatchNorm2d, ReLU, MaxPool2d,
                                               FusedSequential)
    from mpi_pytorch_amd.parallel import ParamArena
    torch.manual_seed(0)

    def make():
        torch.manual_seed(0)
        seq = FusedSequential(Conv2d(3, 16, 3, 1, 1), ReLU(True), Conv2d(16, 16, 3, 1, 1),
                              ReLU(True), MaxPool2d(2, 2), Conv2d(16, 24, 3, 1, 1, bias=False),
                              BatchNorm2d(24), ReLU(True), Conv2d(24, 24, 3, 1, 1, bias=False),
                              BatchNorm2d(24), ReLU(True), Conv2d(24, 8, 3, 2, 1))
        ParamArena(seq, torch.device("cpu"))
        seq.train()
        return seq

    from mpi_pytorch_amd.ops import ref
    x = torch.randn(2, 12, 12, 3)
    grads = []
    pooled = []
    real = ref.maxpool_bwd_relu
    ref.maxpool_bwd_relu = lambda *t: pooled.append(1) or real(*t)
    for on in (True, False):
        old = L._LINK
        L._LINK = on
        try:
            seq = make()
            assert any(seq.links(seq.groups())) == on
            y = seq(x.clone())
            (y.float() ** 2).sum().backward()
            grads.append([p.grad.clone() for p in seq.parameters()])
        finally:
            L._LINK = old
            ref.maxpool_bwd_relu = real if not on else ref.maxpool_bwd_relu
    ref.maxpool_bwd_relu = real
    assert pooled == [1]  # conv -> ReLU -> 2x2 pool: the pool's backward took the ReLU
    for a, b in zip(*grads):
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-5), (a - b).abs().max()


@pytest.mark.parametrize("merged", [True, False])
def test_inception_branches_written_in_place_equal_concat(monkeypatch, merged):
    """Inception blocks whose branches write their outputs at their channel offsets of the
    block output (Fn.ChannelBuffer; backward hands each branch a row-strided window of the
    gradient) == branch tensors concatenated by copy (MPA_CAT_INTO=0), fp32 on the CPU:
    same logits and running statistics, gradients to fp32 rounding."""
    import mpi_pytorch_amd.models.inception as I
    torch.manual_seed(0)
    model, _o, _s, _ = build_training("inception", 10, torch.device("cpu"), World(), 1e-3)
    model.dropout.p = 0.0
    for m in model.modules():
        if hasattr(m, "heads"):
            m.merge_1x1 = merged
    a = model._mpa_arena
    x = torch.randn(2, 299, 299, 8) * (torch.arange(8) < 3)
    y = torch.randint(0, 10, (2,))
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    res = []
    for into in (True, False):
        monkeypatch.setattr(I, "_CAT_INTO", into)
        model.load_state_dict(sd)
        a.zero_grad()
        out = model(x)
        loss_fn(out, y).backward()
        res.append((out[0].detach(), a.grad.clone(),
                    [v.clone() for k, v in model.state_dict().items() if "running" in k]))
    (o1, g1, r1), (o2, g2, r2) = res
    assert torch.allclose(o1, o2, atol=1e-5)
    assert all(torch.allclose(u, v, atol=1e-5) for u, v in zip(r1, r2))
    assert float((g1 - g2).abs().max()) < 1e-5 * float(g2.abs().max())
