"""CPU: the ResNeXt backbone at the drop-in boundary (registry, state-dict ABI, configs) and the host restatement
tests/grouped_refs.resnext_forward against the real reference (live where its tree is present, and through the committed fixture
tests/golden/f13_resnext.npz, which tools/gen_resnext_golden.py writes from the reference)."""
import os
import sys

import numpy as np
import pytest
import torch

import erd_amd
from erd_amd import Config, MODELS
from e2e_util import ROOT
import grouped_refs as R
from oracle import erd_oracle as O
from oracle import ref_stub

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_resnext_golden as GEN      # noqa: E402

CFGS = os.path.join(ROOT, "configs", "gfl_increment")
GOLDEN = os.path.join(ROOT, "tests", "golden", "f13_resnext.npz")
BACKBONE = dict(type="ResNeXt", num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=1, norm_cfg=dict(type="BN", requires_grad=True),
                norm_eval=True, style="pytorch")


@pytest.mark.parametrize("depth,groups,base_width,conv2", [
    (50, 32, 4, [(128, 4, 3, 3), (256, 8, 3, 3), (512, 16, 3, 3), (1024, 32, 3, 3)]),
    (101, 32, 4, [(128, 4, 3, 3), (256, 8, 3, 3), (512, 16, 3, 3), (1024, 32, 3, 3)]),
    (101, 64, 4, [(256, 4, 3, 3), (512, 8, 3, 3), (1024, 16, 3, 3), (2048, 32, 3, 3)])])
def test_registry_builds_resnext_with_the_reference_keys_and_shapes(depth, groups, base_width, conv2):
    net = MODELS.build(dict(BACKBONE, depth=depth, groups=groups, base_width=base_width))
    sd = net.state_dict()
    want = R.resnext_param_shapes(depth, groups, base_width)
    assert sorted(sd) == sorted(want)
    assert all(tuple(sd[k].shape) == tuple(want[k]) for k in want)
    for li, shp in enumerate(conv2):
        for b in (0, 1):
            w = sd[f"layer{li + 1}.{b}.conv2.weight"]
            assert tuple(w.shape) == shp
            assert w.permute(0, 2, 3, 1).is_contiguous()      # [O][kh][kw][I / groups] in memory, as the kernels read it
    # frozen_stages=1: stem + layer1 frozen, the rest trains
    assert all(p.requires_grad == (not k.startswith(("conv1", "bn1", "layer1."))) for k, p in net.named_parameters())


def test_groups_1_is_exactly_resnet():
    a = MODELS.build(dict(BACKBONE, depth=50, groups=1, base_width=4))
    b = MODELS.build(dict(BACKBONE, type="ResNet", depth=50))
    assert {k: tuple(v.shape) for k, v in a.state_dict().items()} == {k: tuple(v.shape) for k, v in b.state_dict().items()}


def test_unsupported_channels_per_group_raise_at_construction():
    with pytest.raises(NotImplementedError, match="4, 8, 16, 32"):
        MODELS.build(dict(BACKBONE, depth=50, groups=32, base_width=8))      # cg = 64 in layer4


@pytest.mark.parametrize("name,ncls", [("gfl_x101_32x4d_fpn_1x_coco_first_40_cats.py", 40),
                                       ("gfl_x101_32x4d_fpn_1x_coco_first_40_incre_last_40_cats.py", 80)])
def test_x101_configs_load_and_build(name, ncls):
    cfg = Config.fromfile(os.path.join(CFGS, name))
    bb = cfg.model.backbone
    assert (bb.type, bb.depth, bb.groups, bb.base_width, bb.frozen_stages, bb.norm_eval) == ("ResNeXt", 101, 32, 4, 1, True)
    assert bb.init_cfg.checkpoint == "open-mmlab://resnext101_32x4d"
    if "ori_setting" in cfg.model:
        cfg.model.latest_model_flag = False
        assert cfg.model.ori_setting.ori_num_classes == 40
        assert os.path.isfile(os.path.join(ROOT, cfg.model.ori_setting.ori_config_file))
    model = MODELS.build(cfg.model)
    sd = model.state_dict()
    assert tuple(sd["backbone.layer3.22.conv2.weight"].shape) == (512, 16, 3, 3)
    assert sd["bbox_head.gfl_cls.weight"].shape[0] == ncls
    want = R.resnext_gfl_state_dict(ncls, 101, 32, 4)
    assert sorted(sd) == sorted(want)
    with pytest.raises(FileNotFoundError):      # 'open-mmlab://...' resolves on disk only
        os.environ.pop("ERD_ALLOW_RANDOM_BACKBONE", None)
        model.backbone.init_weights()


def _restatement(x):
    shapes = R.resnext_param_shapes(GEN.DEPTH, GEN.GROUPS, GEN.BASE_WIDTH)
    sd = {"backbone." + k: O.procedural_tensor(GEN.SEED, "backbone." + k, shp) for k, shp in shapes.items()}
    train = {k for k in sd if O.trainable(k) and sd[k].dtype == torch.float32}
    sd = {k: (v.clone().requires_grad_(True) if k in train else v) for k, v in sd.items()}
    outs = R.resnext_forward(sd, x, GEN.DEPTH, GEN.GROUPS, GEN.BASE_WIDTH)
    sum((o * w).sum() for o, w in zip(outs, R.stage_loss_weights(outs))).backward()
    return sd, outs, train


def test_restatement_matches_the_committed_reference_fixture():
    z = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 976074      # no larger than the largest fixture already committed
    x = torch.from_numpy(z["x"])
    assert torch.equal(x, GEN.golden_input())
    sd, outs, train = _restatement(x)
    # The fixture was computed by ANOTHER fp32 evaluation (the reference's modules on the generating host; a host with another thread
    # count sums the convolutions in another order), so the bounds are those two fp32 implementations of this network are held to in
    # tests/test_gpu_e2e.py: activations 1e-3 of the map's largest value; per gradient tensor the sampled entries within 5e-2 of its
    # largest entry (a ReLU flip moves a tensor by about a percent at this size) and 1e-3 in the median.  The tight pin -- bit-equal
    # outputs, gradients within 3e-6 -- is the live test below, on the host that holds the reference.
    for i, o in enumerate(outs):
        ref = torch.from_numpy(z[f"out{i}"])
        assert float((o.detach() - ref).abs().max()) <= 1e-3 * float(ref.abs().max()), i
    names = [str(n) for n in z["grad_names"]]
    assert {"backbone." + n for n in names} == train
    errs = []
    for n in names:
        g = sd["backbone." + n].grad.reshape(-1)[torch.from_numpy(z["gidx." + n])]
        assert np.array_equal(z["gidx." + n], GEN.sample_index(n, sd["backbone." + n].numel()))
        errs.append(float((g - torch.from_numpy(z["gval." + n])).abs().max()) / max(float(z["gmax." + n]), 1e-30))
        assert errs[-1] <= 5e-2, (n, errs[-1])
    assert float(np.median(errs)) <= 1e-3, float(np.median(errs))


@pytest.mark.skipif(not ref_stub.available(), reason="reference tree not present")
def test_restatement_matches_the_live_reference_resnext():
    """the real mmdet/models/backbones/resnext.py, executed through oracle/ref_stub.py, on inputs that are not the fixture's"""
    import golden_inputs as G
    net = GEN.reference_resnext()
    shapes = R.resnext_param_shapes(GEN.DEPTH, GEN.GROUPS, GEN.BASE_WIDTH)
    net.load_state_dict({k: O.procedural_tensor(GEN.SEED, "backbone." + k, shp) for k, shp in shapes.items()}, strict=True)
    net.train()
    x = G.randn(1313, 2, 3, 48, 80)
    ref_outs = net(x)
    sum((o * w).sum() for o, w in zip(ref_outs, R.stage_loss_weights(ref_outs))).backward()
    sd, outs, train = _restatement(x)
    for a, b in zip(outs, ref_outs):
        assert torch.equal(a, b) or float((a - b).abs().max()) <= 1e-6
    ref_grads = {"backbone." + k: p.grad for k, p in net.named_parameters() if p.grad is not None}
    assert set(ref_grads) == train      # frozen_stages=1 on both sides
    for k, g in ref_grads.items():
        assert float((sd[k].grad - g).abs().max()) <= 3e-6 * float(g.abs().max()) + 1e-12, k
