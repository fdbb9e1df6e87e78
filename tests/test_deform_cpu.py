"""CPU: the deformable-convolution restatement (tests/deform_refs.py) against what can be known without mmcv -- zero offsets are the
plain convolution, autograd's gradients pass gradcheck, hand-computed samples at the boundary rules -- and the DCN backbone at the
drop-in boundary: registry, state-dict ABI, configs, init_weights from an ImageNet-style file, the constructor's refusals,
fallback_on_stride, the shared frozen trunk and the dcn_offset_lr_mult rule."""
import os

import pytest
import torch
import torch.nn.functional as F

import erd_amd  # noqa: F401
from erd_amd import Config, MODELS
from erd_amd import optim_cfg as OC
from erd_amd.modules import ConvHolder, DeformConvHolder
from e2e_util import ROOT
import deform_refs as R
from oracle import erd_oracle as O

CFGS = os.path.join(ROOT, "configs", "gfl_increment")
MAPS = [(1, 1, 1), (2, 2, 3), (1, 5, 7), (1, 8, 6), (3, 18, 34)]
DCN = dict(type="DCN", deform_groups=1, fallback_on_stride=False)
BACKBONE = dict(type="ResNet", depth=50, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=1, norm_cfg=dict(type="BN", requires_grad=True),
                norm_eval=True, style="pytorch", dcn=DCN, stage_with_dcn=(False, True, True, True))


# ---- the restatement -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 2])
def test_zero_offsets_are_the_plain_convolution(s):
    g = torch.Generator().manual_seed(s)
    for N, H, W in MAPS:
        x, w = torch.randn(N, H, W, 8, generator=g).double(), torch.randn(12, 8, 3, 3, generator=g).double()
        OH, OW = R.out_hw(H, W, s)
        y = R.deform_conv(x, torch.zeros(N, OH, OW, 18), w, s)
        ref = F.conv2d(x.permute(0, 3, 1, 2), w, None, s, 1).permute(0, 2, 3, 1)
        assert y.shape == ref.shape and float((y - ref).abs().max()) <= 1e-12, (N, H, W)


@pytest.mark.parametrize("s,OH,OW", [(1, 5, 6), (2, 3, 3)])
def test_gradients_pass_gradcheck_at_generic_offsets(s, OH, OW):
    """with the fp32 rounding of the position switched off (it is piecewise constant: finite differences cannot see through it)"""
    g = torch.Generator().manual_seed(3 + s)
    x = torch.randn(1, 5, 6, 4, generator=g).double().requires_grad_(True)
    off = (torch.rand(1, OH, OW, 18, generator=g).double() * 4 - 2).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b: R.deform_cols(a, b, s, round_pos=False), (x, off), eps=1e-6, atol=1e-6)


def test_hand_known_samples():
    H, W = 4, 5
    x = torch.arange(H * W, dtype=torch.float64).view(H, W) + 1
    # the output is [1, H, W]: use pixel (0, 0) only, whose centre tap sits at (0, 0)
    one = lambda h, w: float(R.deform_cols(x[None, :, :, None], _off(H, W, h, w), 1)[0, 0, 0, 4, 0])
    assert one(0.5, 0.5) == float(x[0:2, 0:2].mean())                        # the mean of four pixels
    assert one(-1.0, 1.0) == 0 and one(1.0, -1.0) == 0                       # exactly -1: outside
    assert one(float(H), 1.0) == 0 and one(1.0, float(W)) == 0               # exactly H / W: outside
    assert one(-0.5, 2.0) == 0.5 * float(x[0, 2])                            # half of row 0
    assert one(H - 0.5, 2.0) == 0.5 * float(x[H - 1, 2])                     # half of row H - 1
    assert one(1.0, W - 0.5) == 0.5 * float(x[1, W - 1]) and one(1.0, -0.5) == 0.5 * float(x[1, 0])
    assert one(2.0, 3.0) == float(x[2, 3])                                   # an integer position: the pixel itself
    assert one(3e9, 0.0) == 0 and one(0.0, -3e9) == 0                        # never an index
    # d/dh at an integer position is the one-sided derivative of the cell [h0, h0 + 1]
    off = _off(H, W, 2.0, 3.0).double().requires_grad_(True)
    R.deform_cols(x[None, :, :, None], off, 1)[0, 0, 0, 4, 0].backward()
    assert float(off.grad[0, 0, 0, 8]) == float(x[3, 3] - x[2, 3]) and float(off.grad[0, 0, 0, 9]) == float(x[2, 4] - x[2, 3])


def _off(H, W, h, w):
    off = torch.zeros(1, H, W, 18)
    off[0, 0, 0, 8], off[0, 0, 0, 9] = h, w
    return off


def test_position_is_one_fp32_addition():
    """an offset of 2^-30 vanishes against the tap coordinate 1 in fp32 (and not in fp64): the sample is the pixel itself"""
    x = torch.tensor([[1.0, 5.0], [9.0, 2.0]], dtype=torch.float64)
    off = torch.zeros(1, 2, 2, 18)
    off[0, 0, 0, 16] = 2.0 ** -30      # tap 8 of pixel (0, 0) sits at (1, 1)
    assert float(R.deform_cols(x[None, :, :, None], off, 1)[0, 0, 0, 8, 0]) == 2.0
    assert float(R.deform_cols(x[None, :, :, None], off, 1, round_pos=False)[0, 0, 0, 8, 0]) == 2.0 * (1 - 2.0 ** -30)


# ---- the module ---------------------------------------------------------------------------------------------------------------------
def test_registry_builds_the_dcn_resnet_with_the_reference_keys_and_shapes():
    net = MODELS.build(dict(BACKBONE))
    sd = net.state_dict()
    want = R.dcn_param_shapes(50)
    assert sorted(sd) == sorted(want) and all(tuple(sd[k].shape) == tuple(want[k]) for k in want)
    offs = sorted(k for k in sd if "conv_offset" in k)
    assert len(offs) == 2 * (4 + 6 + 3) and not any(k.startswith("layer1.") for k in offs)
    for li, planes in ((1, 128), (2, 256), (3, 512)):
        assert tuple(sd[f"layer{li + 1}.0.conv2.conv_offset.weight"].shape) == (18, planes, 3, 3)
        assert tuple(sd[f"layer{li + 1}.0.conv2.conv_offset.bias"].shape) == (18,)
        assert tuple(sd[f"layer{li + 1}.0.conv2.weight"].shape) == (planes, planes, 3, 3)
        assert sd[f"layer{li + 1}.0.conv2.weight"].permute(0, 2, 3, 1).is_contiguous()
    assert all(float(sd[k].abs().max()) == 0 for k in offs), "conv_offset starts at zero"
    assert isinstance(net.layer1[0].conv2, ConvHolder) and isinstance(net.layer2[0].conv2, DeformConvHolder)
    assert net.layer2[0].conv2.conv_offset.stride == 2 and net.layer2[1].conv2.conv_offset.stride == 1
    assert all(p.requires_grad == (not k.startswith(("conv1", "bn1", "layer1."))) for k, p in net.named_parameters())
    # without dcn nothing changes
    plain = MODELS.build({k: v for k, v in BACKBONE.items() if k not in ("dcn", "stage_with_dcn")})
    assert sorted(plain.state_dict()) == sorted(O.resnet_param_shapes(50))


def test_fallback_on_stride_keeps_the_stride_2_blocks_plain():
    net = MODELS.build(dict(BACKBONE, dcn=dict(DCN, fallback_on_stride=True)))
    for li in (2, 3, 4):
        layer = getattr(net, f"layer{li}")
        assert isinstance(layer[0].conv2, ConvHolder) and not layer[0].with_dcn
        assert all(isinstance(b.conv2, DeformConvHolder) and b.with_dcn for b in list(layer)[1:])
    assert sorted(net.state_dict()) == sorted(R.dcn_param_shapes(50, fallback_on_stride=True))


def test_what_is_not_built_raises_naming_the_value():
    with pytest.raises(NotImplementedError, match="DCNv2"):
        MODELS.build(dict(BACKBONE, dcn=dict(DCN, type="DCNv2")))
    with pytest.raises(NotImplementedError, match="deform_groups=4"):
        MODELS.build(dict(BACKBONE, dcn=dict(DCN, deform_groups=4)))
    with pytest.raises(NotImplementedError, match="groups=32"):
        MODELS.build(dict(BACKBONE, type="ResNeXt", depth=101, groups=32, base_width=4))
    with pytest.raises(AssertionError, match="stage_with_dcn"):
        MODELS.build(dict(BACKBONE, stage_with_dcn=(False, True, True)))


def test_init_weights_from_an_imagenet_style_file_leaves_conv_offset_zero(tmp_path):
    g = torch.Generator().manual_seed(0)
    plain = {k: torch.randn(shp, generator=g) if "running_var" not in k else torch.rand(shp, generator=g) + 0.5
             for k, shp in O.resnet_param_shapes(50).items()}
    plain.update({"fc.weight": torch.zeros(10, 2048), "fc.bias": torch.zeros(10)})
    path = str(tmp_path / "resnet50-imagenet.pth")
    torch.save(plain, path)
    net = MODELS.build(dict(BACKBONE, init_cfg=dict(type="Pretrained", checkpoint=path)))
    net.init_weights()
    sd = net.state_dict()
    assert all(float(v.abs().max()) == 0 for k, v in sd.items() if "conv_offset" in k)
    assert torch.equal(sd["layer3.2.conv2.weight"], plain["layer3.2.conv2.weight"]) and torch.equal(sd["conv1.weight"], plain["conv1.weight"])
    # anything else missing still raises
    del plain["layer2.1.conv2.weight"]
    torch.save(plain, path)
    with pytest.raises(RuntimeError, match="layer2.1.conv2.weight"):
        MODELS.build(dict(BACKBONE, init_cfg=dict(type="Pretrained", checkpoint=path))).init_weights()
    # a dconv checkpoint (every key present) loads strictly
    full = {k: torch.full(shp, 0.25) for k, shp in R.dcn_param_shapes(50).items()}
    net.load_state_dict(full, strict=True)
    assert float(net.layer4[2].conv2.conv_offset.bias.detach()[0]) == 0.25


@pytest.mark.parametrize("name,ncls", [("gfl_r50_dconv_c3-c5_fpn_1x_coco_first_40_cats.py", 40),
                                       ("gfl_r50_dconv_c3-c5_fpn_1x_coco_first_40_incre_last_40_cats.py", 80)])
def test_dconv_configs_load_and_build(name, ncls):
    cfg = Config.fromfile(os.path.join(CFGS, name))
    bb = cfg.model.backbone
    assert (bb.type, bb.depth, bb.frozen_stages, bb.norm_eval) == ("ResNet", 50, 1, True)
    assert dict(bb.dcn) == DCN and tuple(bb.stage_with_dcn) == (False, True, True, True)
    assert bb.init_cfg.checkpoint == "torchvision://resnet50"
    if "ori_setting" in cfg.model:
        cfg.model.latest_model_flag = False
        assert cfg.model.ori_setting.ori_num_classes == 40
        assert cfg.model.ori_setting.ori_checkpoint_file.endswith("gfl_r50_dconv_c3-c5_fpn_1x_coco_first_40_cats/epoch_12.pth")
        assert os.path.isfile(os.path.join(ROOT, cfg.model.ori_setting.ori_config_file))
    model = MODELS.build(cfg.model)
    sd = model.state_dict()
    assert sd["bbox_head.gfl_cls.weight"].shape[0] == ncls
    assert sorted(sd) == sorted(R.dcn_gfl_state_dict(ncls, 50))
    assert tuple(sd["backbone.layer4.2.conv2.conv_offset.weight"].shape) == (18, 512, 3, 3)


def test_student_and_teacher_share_the_frozen_trunk():
    """stage 1 has no DCN block: the trunk rule (same depth / frozen_stages, equal frozen tensors) holds for DCN detectors"""
    cfg2 = Config.fromfile(os.path.join(CFGS, "gfl_r50_dconv_c3-c5_fpn_1x_coco_first_40_incre_last_40_cats.py"))
    cfg1 = Config.fromfile(os.path.join(CFGS, "gfl_r50_dconv_c3-c5_fpn_1x_coco_first_40_cats.py"))
    cfg2.model.latest_model_flag = False
    student, teacher = MODELS.build(cfg2.model), MODELS.build(cfg1.model)
    teacher.backbone.load_state_dict(student.backbone.state_dict(), strict=True)
    student.attach_teacher(teacher, 40)
    assert student.shares_trunk()
    assert not any(isinstance(m, DeformConvHolder) for b in student.backbone.layer1 for m in b.modules())
    with torch.no_grad():
        teacher.backbone.layer1[0].conv1.weight.add_(1.0)
    assert not student.shares_trunk()


def test_dcn_offset_lr_mult_acts_on_exactly_the_conv_offset_parameters():
    net = MODELS.build(dict(BACKBONE))
    names = [n for n, _ in net.named_parameters()]
    rows = OC.resolve_paramwise(net, 0.01, 1e-4, dict(dcn_offset_lr_mult=0.1, bias_lr_mult=2.0))
    assert [r["name"] for r in rows] == names
    n_off = 0
    for r, (n, p) in zip(rows, net.named_parameters()):
        if not p.requires_grad:
            assert r["lr"] == 0.01
        elif ".conv_offset." in n:
            n_off += 1
            assert r["lr"] == pytest.approx(0.001, rel=1e-12), n      # weight AND bias; bias_lr_mult does not apply to that bias
        else:
            assert r["lr"] == 0.01, n                                  # (the BN biases are norm biases: no bias_lr_mult either)
    assert n_off == 2 * (4 + 6 + 3)
    # a custom key that matches wins over the rule; without the multiplier nothing changes
    rows = OC.resolve_paramwise(net, 0.01, 1e-4, dict(dcn_offset_lr_mult=0.1, custom_keys={"layer4.2.conv2.conv_offset": dict(lr_mult=0.5)}))
    by = {r["name"]: r["lr"] for r in rows}
    assert by["layer4.2.conv2.conv_offset.weight"] == pytest.approx(0.005) and by["layer4.1.conv2.conv_offset.bias"] == pytest.approx(0.001)
    rows = OC.resolve_paramwise(net, 0.01, 1e-4, dict(bias_lr_mult=2.0))
    by = {r["name"]: r["lr"] for r in rows}
    assert by["layer4.1.conv2.conv_offset.bias"] == 0.01 and by["layer4.1.conv2.conv_offset.weight"] == 0.01
