"""GPU: heads whose class count is not a multiple of 4 on the training path (70+10 phase 1, the 50- / 60- / 70-class
students of 40+10x4): the loss kernels at any (c_old, c_all) against the oracle under autograd, the padded gfl_cls
backward against fp64 torch-CPU, and training runs through Runner -- a 70-class base epoch and a 40 -> 50 -> 60 chain
of phases that hands each phase's checkpoint (teacher copy included) to the next."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import golden_inputs as G
from oracle import erd_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFGS = os.path.join(ROOT, "configs", "gfl_increment")
CFG_FIRST = os.path.join(CFGS, "gfl_r50_fpn_1x_coco_first_40_cats.py")
CFG_FIRST70 = os.path.join(CFGS, "gfl_r101_fpn_1x_coco_first_70_cats.py")
CFG_40_50 = os.path.join(CFGS, "gfl_r50_fpn_1x_coco_40_10x4_phase2_40_50_cats.py")
CFG_50_60 = os.path.join(CFGS, "gfl_r50_fpn_1x_coco_40_10x4_phase3_50_60_cats.py")


def _sizes(H, W):
    out, h, w = [], H // 8, W // 8
    for _ in range(5):
        out.append((h, w)); h, w = (h + 1) // 2, (w + 1) // 2
    return out


def _relerr(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-20))


def _maps(seed, N, C, sizes, scale=1.0, shift=0.0):
    return [G.randn(seed + l, N, C, h, w, scale=scale, shift=shift) for l, (h, w) in enumerate(sizes)]


def _gts(seed, N, H, W, cn):
    g = torch.Generator().manual_seed(seed)
    boxes, labels = [], []
    for _ in range(N):
        k = 6
        xy = torch.rand(k, 2, generator=g) * torch.tensor([W * 0.7, H * 0.7])
        wh = 12 + torch.rand(k, 2, generator=g) * torch.tensor([W * 0.4, H * 0.4])
        b = torch.cat([xy, torch.minimum(xy + wh, torch.tensor([W - 1.0, H - 1.0]))], 1)
        boxes.append(b.float())
        labels.append(torch.randint(0, cn, (k,), generator=g))
    return boxes, labels


def _pack_gts(boxes, labels):
    off = [0]
    for b in boxes:
        off.append(off[-1] + b.shape[0])
    return (torch.cat(boxes, 0).cuda(), torch.cat(labels, 0).cuda(), torch.tensor(off, dtype=torch.int32).cuda(),
            max(b.shape[0] for b in boxes))


# (c_old, c_all): the base phases of 70+10 / 50+30, the students of 40+10x4, the 70+10 student
PAIRS = [(0, 70), (0, 50), (40, 50), (50, 60), (60, 70), (70, 80)]


@pytest.mark.parametrize("H,W", [(128, 160), (96, 160)])          # A = 428; A = 323 (odd: row runs start off 16-byte boundaries)
@pytest.mark.parametrize("c_old,c_all", PAIRS)
def test_loss_kernels_at_any_class_count(c_old, c_all, H, W):
    from erd_amd import kernels as K
    N, cn = 2, c_all - c_old
    sizes = _sizes(H, W)
    metas = [dict(pad_shape=(H, W), img_shape=(H, W), batch_input_shape=(H, W)) for _ in range(N)]
    gtb, gtl = _gts(900 + c_all, N, H, W, cn)
    s_cls = [m.requires_grad_(True) for m in _maps(910, N, c_all, sizes, 1.5, -3.0)]
    s_bbox = [m.requires_grad_(True) for m in _maps(920, N, 68, sizes)]
    distill = c_old > 0
    if distill:
        t_cls, t_bbox = _maps(930, N, c_old, sizes, 1.5, -3.0), _maps(940, N, 68, sizes)
        ref = O.erd_head_loss(t_cls, t_bbox, s_cls, s_bbox, gtb, gtl, metas, c_old, c_all)
        keys = ("loss_cls", "loss_bbox", "loss_dfl", "loss_dist_cls", "loss_dist_bbox")
    else:
        ref = O.gfl_head_loss(s_cls, s_bbox, gtb, gtl, metas, c_all)
        keys = ("loss_cls", "loss_bbox", "loss_dfl")
    want = np.concatenate([[float(v) for v in ref[k]] for k in keys])
    O.parse_losses(ref).backward()

    sc = O.flatten_levels([m.detach() for m in s_cls]).contiguous().cuda()
    sb = O.flatten_levels([m.detach() for m in s_bbox]).contiguous().cuda()
    assert sc.shape[1] == sum(h * w for h, w in sizes)
    anchors = K.grid_anchors(sizes, O.STRIDES, "cuda")
    gb, gl, goff, mg = _pack_gts(gtb, gtl)
    lab, lw, bt, npos = K.atss_assign(anchors, None, sizes, gb, gl, goff, N, mg, c_all)
    score, wt, sums = K.gfl_losses_fwd(sc, sb, anchors, lab, lw, bt, sizes, O.STRIDES, c_old, c_all)
    avg = torch.stack([npos.clamp(min=1).sum().float(), sums[:, 3].sum().float()])
    if distill:
        tc = O.flatten_levels(t_cls).contiguous().cuda()
        tb = O.flatten_levels(t_bbox).contiguous().cuda()
        ers = K.ers_select(tc, tb)
        l2s = K.l2_distill(sc, tc, ers["idx_cls"], ers["counts"], c_old)
        keep, _ = K.distill_nms(tc, tb, anchors, ers["idx_bbox"], ers["counts"])
        kds = K.kd_kl(sb, tb, sc, keep, c_old, 10.0)
        fin = (l2s, kds, ers["counts"], 5, N)
    else:
        fin = (None, None, None, 5, 0)
    losses, _ = K.loss_finalize(sums, avg, *fin, c_old, 1.0, 1.0, 2.0, 0.25, 0.25, None, True, False)
    got = losses.cpu().numpy()
    assert np.allclose(got, want, rtol=1e-5, atol=1e-7), (got, want)

    _, coef = K.loss_finalize(sums, avg, *fin, c_old, 1.0, 1.0, 2.0, 0.25, 0.25, torch.ones_like(losses), False, True)
    dcls, dbbox = K.gfl_losses_bwd(sc, sb, anchors, lab, lw, bt, sizes, O.STRIDES, c_old, c_all, score, wt, coef)
    if distill:
        K.l2_distill_bwd_(sc, tc, ers["idx_cls"], ers["counts"], coef[20:], c_old, dcls)
        K.kd_kl_bwd_(sb, tb, sc, keep, coef[20 + N:], c_old, 10.0, dbbox)
    gc = O.flatten_levels([m.grad for m in s_cls])
    gbx = O.flatten_levels([m.grad for m in s_bbox])
    a, b = dcls.cpu(), dbbox.cpu()
    assert float((a - gc).abs().max()) <= 1e-4 * float(gc.abs().max()) + 1e-9
    assert float((b - gbx).abs().max()) <= 1e-4 * float(gbx.abs().max()) + 1e-9


def test_loss_backward_into_a_gradient_buffer_of_another_alignment():
    """the backward write-back when dcls starts at another 16-byte phase than cls (the scalar path): same values"""
    from erd_amd import kernels as K
    from erd_amd._lib import call
    N, c_old, c_all, (H, W) = 2, 0, 70, (96, 160)
    sizes = _sizes(H, W)
    gtb, gtl = _gts(960, N, H, W, c_all)
    sc = O.flatten_levels(_maps(961, N, c_all, sizes, 1.5, -3.0)).contiguous().cuda()
    sb = O.flatten_levels(_maps(962, N, 68, sizes)).contiguous().cuda()
    anchors = K.grid_anchors(sizes, O.STRIDES, "cuda")
    gb, gl, goff, mg = _pack_gts(gtb, gtl)
    lab, lw, bt, npos = K.atss_assign(anchors, None, sizes, gb, gl, goff, N, mg, c_all)
    score, wt, sums = K.gfl_losses_fwd(sc, sb, anchors, lab, lw, bt, sizes, O.STRIDES, c_old, c_all)
    avg = torch.stack([npos.clamp(min=1).sum().float(), sums[:, 3].sum().float()])
    fin = (None, None, None, 5, 0, c_old, 1.0, 1.0, 2.0, 0.25, 0.25)
    losses, _ = K.loss_finalize(sums, avg, *fin, None, True, False)
    _, coef = K.loss_finalize(sums, avg, *fin, torch.ones_like(losses), False, True)
    dcls, dbbox = K.gfl_losses_bwd(sc, sb, anchors, lab, lw, bt, sizes, O.STRIDES, c_old, c_all, score, wt, coef)
    store = torch.full((sc.numel() + 1,), float("nan"), device="cuda")
    d2 = store[1:].view_as(sc)                 # 4 bytes past the allocation's 16-byte boundary
    db2 = torch.empty_like(dbbox)
    call("erd_gfl_losses_bwd", K._p(sc), K._p(sb), K._p(anchors), K._p(lab), K._p(lw), K._p(bt), K._lvl_off(sizes),
         K._iarr(O.STRIDES), 5, N, sc.shape[1], c_old, c_all, K._p(score), K._p(wt), K._p(coef), K._p(d2), K._p(db2),
         K._stream())
    assert torch.equal(d2, dcls) and torch.equal(db2, dbbox)


@pytest.mark.parametrize("C", [50, 70])
def test_head_conv_bias_at_class_counts_not_multiple_of_4(C):
    """gfl_cls forward + backward (padded weight / input gradients) against fp64 torch-CPU, at the head-conv bounds"""
    from erd_amd import functional as Fn
    N = 2
    sizes = [(16, 20), (8, 10), (4, 5), (2, 3), (1, 2)]
    A = sum(h * w for h, w in sizes)
    x = G.randn(80, N, A, 256)
    w = G.randn(81, C, 256, 3, 3, scale=(1.0 / 2304) ** 0.5)
    b = G.randn(82, C, scale=0.1)
    xd, wd, bd = (t.double().requires_grad_(True) for t in (x, w, b))
    outs, off = [], 0
    for h, w_ in sizes:
        xl = xd[:, off:off + h * w_].reshape(N, h, w_, 256).permute(0, 3, 1, 2)
        outs.append(F.conv2d(xl, wd, bd, 1, 1).permute(0, 2, 3, 1).reshape(N, h * w_, C))
        off += h * w_
    ref = torch.cat(outs, 1)
    dy = G.randn(83, N, A, C)
    ref.backward(dy.double())
    xg = x.cuda().requires_grad_(True)
    wg = w.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    bg = b.cuda().requires_grad_(True)
    out = Fn.HeadConvBias.apply(xg, wg, bg, sizes)
    assert out.shape == (N, A, C)
    assert _relerr(out.detach().cpu().double(), ref.detach()) < 2e-5
    out.backward(dy.cuda())
    assert _relerr(xg.grad.cpu().double(), xd.grad) < 1e-4
    assert _relerr(wg.grad.cpu().double(), wd.grad) < 1e-4
    assert _relerr(bg.grad.cpu().double(), bd.grad) < 1e-4


def _cfg(path, work_dir, **over):
    from erd_amd import Config
    cfg = Config.fromfile(path)
    cfg.work_dir = str(work_dir)
    cfg.merge_from_dict({"train_dataloader.batch_size": 2, "train_cfg.max_epochs": 1, "model.backbone.init_cfg": None,
                         "default_hooks.logger.interval": 1, **over})
    return cfg


def _data(num_classes, seed=0):
    from erd_amd.runner import SyntheticDetData
    return SyntheticDetData(2, num_classes, 2, image_hw=(123, 153), seed=seed)


def test_base_training_at_70_classes(tmp_path):
    """70+10 phase 1 (R101, a 70-class head) trains an epoch and writes its checkpoint"""
    from erd_amd.runner import Runner
    torch.manual_seed(0)
    r = Runner.from_cfg(_cfg(CFG_FIRST70, tmp_path / "first70"), data=_data(70), log=lambda *_: None)
    before = r.model.bbox_head.gfl_cls.weight.detach().clone()
    h = r.train()
    assert len(h) == 2 and all(np.isfinite(x["loss"]) for x in h)
    assert (tmp_path / "first70" / "epoch_1.pth").is_file()
    assert not torch.equal(before, r.model.bbox_head.gfl_cls.weight.detach())


def test_phase_chain_40_50_60_then_resume(tmp_path):
    """first-40 -> 40->50 -> 50->60 through Runner, each phase reading the previous phase's checkpoint (teacher copy
    included); the last phase resumes from its work dir"""
    from erd_amd.runner import Runner
    torch.manual_seed(0)
    r0 = Runner.from_cfg(_cfg(CFG_FIRST, tmp_path / "p0"), data=_data(40), log=lambda *_: None)
    r0.train()
    ck0 = tmp_path / "p0" / "epoch_1.pth"
    torch.manual_seed(1)
    over1 = {"model.ori_setting.ori_checkpoint_file": str(ck0), "model.ori_setting.ori_config_file": CFG_FIRST}
    r1 = Runner.from_cfg(_cfg(CFG_40_50, tmp_path / "p1", **over1), data=_data(10, seed=1), log=lambda *_: None)
    h1 = r1.train()
    assert all(np.isfinite(x["loss"]) and "loss_dist_cls" in x for x in h1)
    ck1 = tmp_path / "p1" / "epoch_1.pth"
    sd1 = torch.load(ck1, map_location="cpu", weights_only=False)["state_dict"]
    assert any(k.startswith("ori_model.") for k in sd1)
    over2 = {"model.ori_setting.ori_checkpoint_file": str(ck1), "model.ori_setting.ori_config_file": CFG_40_50,
             "train_cfg.max_epochs": 2}
    torch.manual_seed(2)
    r2 = Runner.from_cfg(_cfg(CFG_50_60, tmp_path / "p2", **over2), data=_data(10, seed=2), log=lambda *_: None)
    sd2 = r2.model.state_dict()
    for k, v in sd1.items():
        if not k.startswith("ori_model."):
            assert torch.equal(sd2["ori_model." + k].cpu(), v), k
    assert torch.equal(sd2["bbox_head.gfl_cls.weight"][:50].cpu(), sd1["bbox_head.gfl_cls.weight"])
    assert r2.model.bbox_head.gfl_cls.weight.shape[0] == 60 and r2.model.ori_num_classes == 50
    h2 = r2.train()
    assert len(h2) == 4 and all(np.isfinite(x["loss"]) and "loss_dist_cls" in x for x in h2)
    # resume inside the last phase: stop after epoch 1, resume from the work dir, finish epoch 2
    torch.manual_seed(2)
    r3 = Runner.from_cfg(_cfg(CFG_50_60, tmp_path / "p2b", **{**over2, "train_cfg.max_epochs": 1}), data=_data(10, seed=2),
                         log=lambda *_: None)
    r3.train()
    r4 = Runner.from_cfg(_cfg(CFG_50_60, tmp_path / "p2b", **over2, resume=True), data=_data(10, seed=2), log=lambda *_: None)
    assert r4.epoch == 1
    h4 = r4.train()
    assert [x["epoch"] for x in h4] == [2, 2]
    assert np.allclose([x["loss"] for x in h4], [x["loss"] for x in h2[2:]], rtol=1e-4)
