"""GPU: ResNet-50 with deformable convolutions in c3-c5 (dcn=dict(type='DCN', deform_groups=1), stage_with_dcn=(F, T, T, T)) against
the restatement tests/deform_refs.py composed with the oracle: the backbone's stage outputs and parameter gradients in fp64, a whole
ERD step on DCN teacher and student, two trainer steps with a checkpoint round trip, and tools/train.py on the new 40+40 config."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("oracle_threads")]

import deform_refs as R
import golden_inputs as G
from e2e_util import ROOT, make_samples
from oracle import erd_oracle as O

RTOL = 1e-3           # stage outputs / losses: the bound of tests/test_gpu_resnext.py and of tests/test_gpu_e2e.py's F7 test
OFFSET_SCALE = 0.15   # times the procedural conv_offset tensors: offsets of about a pixel in layer2 (asserted below)
CFGS = os.path.join(ROOT, "configs", "gfl_increment")
CFG_FIRST = os.path.join(CFGS, "gfl_r50_dconv_c3-c5_fpn_1x_coco_first_40_cats.py")
CFG_INCRE = os.path.join(CFGS, "gfl_r50_dconv_c3-c5_fpn_1x_coco_first_40_incre_last_40_cats.py")
DCN = dict(type="DCN", deform_groups=1, fallback_on_stride=False)


def relerr(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-20))


def _r50_dcn():
    from erd_amd.modules import ResNet
    return ResNet(depth=50, frozen_stages=1, norm_eval=True, dcn=DCN, stage_with_dcn=(False, True, True, True))


def _double(sd):
    return {k: (v.double() if v.dtype == torch.float32 else v) for k, v in sd.items()}


def _first_offsets(sd64, x64):
    """the offsets of layer2.0 in the restatement"""
    sub = {k[len("backbone."):]: v for k, v in sd64.items() if k.startswith("backbone.")}
    h = O.resnet_layer(sub, O.resnet_stem(sub, x64), 0, 50)
    p = "layer2.0"
    o1 = F.relu(O._bn_eval(F.conv2d(h, sub[p + ".conv1.weight"]), sub, p + ".bn1")).permute(0, 2, 3, 1)
    return R.conv_offset(o1, sub[p + ".conv2.conv_offset.weight"], sub[p + ".conv2.conv_offset.bias"], 2)


def test_dcn_backbone_matches_the_fp64_restatement():
    """stage outputs within 1e-3 of the map's largest value; gradients of grouped_refs.stage_loss_weights' loss per tensor within 5e-2
    of the tensor's largest entry and 1e-3 in the median (the bounds of test_resnext50_backbone_matches_the_reference_fixture)"""
    from grouped_refs import stage_loss_weights
    from erd_amd import functional as Fn
    sd = {k: v for k, v in R.dcn_gfl_state_dict(40, 50, seed=0, offset_scale=OFFSET_SCALE).items() if k.startswith("backbone.")}
    x = G.randn(77, 2, 3, 64, 96)
    sd64 = _double(sd)
    spread = float(_first_offsets(sd64, x.double()).std())
    assert 0.3 < spread < 2.0, spread
    train = {k for k in sd if O.trainable(k) and sd[k].dtype == torch.float32}
    leaf = {k: (v.clone().requires_grad_(True) if k in train else v) for k, v in sd64.items()}
    refs = R.dcn_resnet_forward(leaf, x.double(), 50)
    ws = stage_loss_weights(refs)
    sum((o * w.double()).sum() for o, w in zip(refs, ws)).backward()

    net = _r50_dcn()
    net.load_state_dict({k[len("backbone."):]: v for k, v in sd.items()}, strict=True)
    net = net.cuda().train()
    outs = net(x.cuda())
    for i, (o, r) in enumerate(zip(outs, refs)):
        assert tuple(o.shape) == tuple(r.shape)
        assert relerr(o.detach().cpu().contiguous().double(), r.detach()) < RTOL, i
    sum((o * w.cuda()).sum() for o, w in zip(outs, ws)).backward()
    Fn.trail_join(x.device)
    torch.cuda.synchronize()
    params = dict(net.named_parameters())
    assert {"backbone." + k for k, p in params.items() if p.requires_grad} == train
    errs = {}
    for k in sorted(train):
        g = leaf[k].grad
        errs[k] = float((params[k[len("backbone."):]].grad.detach().cpu().double() - g).abs().max()) / max(float(g.abs().max()), 1e-30)
        assert errs[k] < 5e-2, (k, errs[k])
    off = [v for k, v in errs.items() if "conv_offset" in k]
    print("gradient error / largest entry: median %.2e max %.2e; conv_offset tensors median %.2e max %.2e" % (
        float(np.median(list(errs.values()))), max(errs.values()), float(np.median(off)), max(off)))
    assert len(off) == 26 and float(np.median(list(errs.values()))) < 1e-3
    assert all(float(leaf[k].grad.abs().max()) > 0 for k in train if "conv_offset" in k), "the offsets receive gradients"


def test_zero_conv_offset_is_the_plain_resnet():
    sd = {k: v for k, v in R.dcn_gfl_state_dict(40, 50, seed=0, offset_zero=True).items() if k.startswith("backbone.")}
    x = G.randn(78, 2, 3, 64, 96)
    plain = {k: v for k, v in _double(sd).items() if "conv_offset" not in k}
    refs = O.resnet_forward(plain, x.double(), 50)
    net = _r50_dcn()
    net.load_state_dict({k[len("backbone."):]: v for k, v in sd.items()}, strict=True)
    net = net.cuda().eval()
    with torch.no_grad():
        outs = net(x.cuda())
    for i, (o, r) in enumerate(zip(outs, refs)):
        assert relerr(o.cpu().contiguous().double(), r) < RTOL, i


# ---- whole steps ----------------------------------------------------------------------------------------------------------------------
def dcn_state_dicts(c_old=40, c_all=80):
    tsd = R.dcn_gfl_state_dict(c_old, 50, seed=0, offset_scale=OFFSET_SCALE)
    ssd = O.student_state_from_teacher(tsd, c_all, seed=1)
    for k in sorted(ssd):
        if O.trainable(k) and ssd[k].dim() == 4:
            ssd[k] = ssd[k] + 0.02 * ssd[k].abs().mean() * G.randn(700 + len(k), *ssd[k].shape)
    return tsd, ssd


def build_dcn_erd(tsd, ssd):
    """teacher + student through the registry from the R50-dconv configs"""
    from erd_amd import Config, MODELS
    tcfg, scfg = Config.fromfile(CFG_FIRST), Config.fromfile(CFG_INCRE)
    scfg.model.latest_model_flag = False
    teacher, student = MODELS.build(tcfg.model), MODELS.build(scfg.model)
    teacher.load_state_dict(tsd, strict=True)
    student.load_state_dict(ssd, strict=True)
    student.attach_teacher(teacher, tsd["bbox_head.gfl_cls.bias"].shape[0])
    return student.cuda().train()


def _batch(seed):
    imgs, boxes, labels = O.synthetic_batch(2, 128, 160, 40, seed=seed)
    x, metas = O.preprocess(imgs)
    assert tuple(x.shape[2:]) == (128, 160)
    return x, boxes, labels, metas


def test_erd_step_on_dcn_teacher_and_student_matches_the_restatement():
    tsd, ssd = dcn_state_dicts()
    assert any("conv_offset" in k for k in ssd) and sorted(k for k in tsd if "conv_offset" in k) == sorted(k for k in ssd if "conv_offset" in k)
    model = build_dcn_erd(tsd, ssd)
    assert model.shares_trunk()      # stage 1 has no DCN block
    x, boxes, labels, metas = _batch(0)
    ref, aux = R.erd_step_loss(tsd, ssd, x, boxes, labels, metas, 40, 80, 50, return_aux=True)
    losses = model(x.cuda(), make_samples(boxes, labels, metas), mode="loss")
    L = {k: np.array([float(v.detach()) for v in vs], dtype=np.float64) for k, vs in losses.items()}
    for k, vs in ref.items():
        r = np.array([float(v) for v in vs])
        assert np.allclose(L[k], r, rtol=RTOL, atol=1e-7), (k, L[k], r)
    t_cls, t_bbox, sizes = model.ori_model._forward_cat(x.cuda())
    ers = model.sel_pos_cat(t_cls, t_bbox)
    cnt = ers["counts"].cpu()
    for i in range(2):
        assert torch.equal(ers["idx_cls"][i, :int(cnt[i, 0])].cpu(), aux["ers_cls"][i])
        assert torch.equal(ers["idx_bbox"][i, :int(cnt[i, 1])].cpu(), aux["ers_bbox"][i])


def test_trainer_two_steps_and_checkpoint_round_trip(tmp_path):
    from erd_amd.engine import ERDTrainer
    from erd_amd import runner
    tsd, ssd = dcn_state_dicts()
    model = build_dcn_erd(tsd, ssd)
    tr = ERDTrainer(model, lr=0.02, momentum=0.9, weight_decay=1e-4, batch_size_per_gpu=2, auto_scale_lr=False, warmup_iters=0)
    for it in range(2):
        x, boxes, labels, metas = _batch(it)
        log = tr.train_step(x.cuda(), make_samples(boxes, labels, metas))
        assert np.isfinite(float(torch.as_tensor(log["loss"]).detach()))
    tr.flush()
    torch.cuda.synchronize()
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    assert all(torch.isfinite(v).all() for v in sd.values() if v.dtype == torch.float32)
    offs = sorted(k for k in sd if "conv_offset" in k and not k.startswith("ori_model."))
    assert len(offs) == 26
    assert all(not torch.equal(sd[k], ssd[k]) for k in offs), "every conv_offset parameter was updated"
    assert all(torch.equal(sd["ori_model." + k], tsd[k]) for k in tsd if "conv_offset" in k), "the teacher's stay"
    path = str(tmp_path / "dcn.pth")
    runner.save_checkpoint(path, model, tr)
    on_disk = torch.load(path, map_location="cpu", weights_only=False)["state_dict"]
    assert all(k in on_disk and torch.equal(on_disk[k], sd[k]) for k in offs)
    fresh = build_dcn_erd(tsd, ssd)
    runner.load_checkpoint(path, fresh)
    got = fresh.state_dict()
    for k in offs + ["ori_model." + k for k in offs]:
        assert torch.equal(got[k].cpu(), sd[k]), k


def test_train_py_runs_one_epoch_on_the_dconv_config(tmp_path):
    teacher = tmp_path / "teacher.pth"
    torch.save(dict(state_dict=R.dcn_gfl_state_dict(40, 50, seed=0, offset_scale=OFFSET_SCALE)), teacher)
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train.py"), CFG_INCRE, "--work-dir", str(tmp_path / "w"),
           "--synthetic", "4", "--image-size", "123", "153", "--cfg-options", "train_dataloader.batch_size=2", "train_cfg.max_epochs=1",
           f"model.ori_setting.ori_checkpoint_file={teacher}", f"model.ori_setting.ori_config_file={CFG_FIRST}",
           "default_hooks.logger.interval=1"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "Epoch(train) [1][4/4]" in out.stdout and "loss_dist_bbox" in out.stdout
    ck = torch.load(tmp_path / "w" / "epoch_1.pth", map_location="cpu", weights_only=False)["state_dict"]
    assert tuple(ck["backbone.layer3.5.conv2.conv_offset.weight"].shape) == (18, 256, 3, 3)
