"""GPU: the grouped convolution kernels on random data against fp64 at every element, the grouped ConvBNAct / fused ResNeXt bottleneck /
ResLayerFn stage against autograd of the CPU restatement (the bounds the same functions carry at cardinality 1 in
tests/test_gpu_functions.py), the ResNeXt-50 32x4d backbone against the reference fixture tests/golden/f13_resnext.npz, and whole ERD
steps on ResNeXt-50 32x4d teacher / student against the composed restatement of tests/grouped_refs.py."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("oracle_threads")]

import golden_inputs as G
import grouped_refs as R
from e2e_util import ROOT, make_samples
from oracle import erd_oracle as O

U24 = 2.0 ** -24      # unit roundoff of fp32
RTOL = 1e-3           # losses: the bound of tests/test_gpu_e2e.py's F7 test
CFGS = os.path.join(ROOT, "configs", "gfl_increment")
CFG_X_FIRST = os.path.join(CFGS, "gfl_x101_32x4d_fpn_1x_coco_first_40_cats.py")
CFG_X_INCRE = os.path.join(CFGS, "gfl_x101_32x4d_fpn_1x_coco_first_40_incre_last_40_cats.py")


def relerr(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-20))


def cl_weight(w):     # OIHW cpu -> channels_last parameter on the GPU
    return w.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)


def worst(err, bound):
    """largest err / bound over the elements (bound > 0 wherever err > 0)"""
    return float((err / bound.clamp(min=1e-300)).max())


# ------------------------------------------------------------------------------------------------------------------------
# fp64 bounds at every element, random data.
# Derivation.  An output of the forward / input-gradient kernel is ONE fma chain over at most K = 9 * cg products a_i * b_i: each
# fma rounds the running sum once (relative error <= u = 2^-24), and every running sum is bounded by sum |a_i| |b_i|, so the chain is
# off by at most K * u * sum |a_i| |b_i| (first order; Higham, Accuracy and Stability, section 3.1).  The epilogue adds e more
# roundings of values bounded by the same magnitude M once its operands are included: forward e = 3 (times scale, plus shift, plus
# residual) with M = |scale| * sum |x| |w| + |shift| + |res|; input gradient e = 1 (plus residual; the row-scaled weight w * scale is
# the same IEEE product on both sides, so it is an INPUT of the bound, not an operation of it) with M = sum |dz| |w * scale| + |res|.
# A weight-gradient element is a sum of n = N * OH * OW products in SOME order (the split count and the reduce tree): any order
# rounds at most n - 1 times, each below u times the sum of magnitudes: n * u * sum |dz| |x| -- which therefore does not fix S.
# ------------------------------------------------------------------------------------------------------------------------
BOUND_CASES = [(32, 4, 1), (32, 4, 2), (32, 8, 1), (32, 8, 2), (32, 16, 1), (32, 16, 2), (32, 32, 1), (32, 32, 2), (64, 4, 1), (3, 8, 2)]
BN, BH, BW = 2, 13, 17


def _rand_case(card, cg, s, seed):
    Cc = card * cg
    OH, OW = (BH - 1) // s + 1, (BW - 1) // s + 1
    x = G.randn(seed, BN, BH, BW, Cc).abs()
    w = G.randn(seed + 1, Cc, 3, 3, cg, scale=(2.0 / (9 * cg)) ** 0.5)      # He
    dz = G.randn(seed + 2, BN, OH, OW, Cc)
    return Cc, OH, OW, x, w, dz


@pytest.mark.parametrize("card,cg,s", BOUND_CASES)
def test_forward_and_input_gradient_within_the_fma_chain_bound_of_fp64(card, cg, s):
    from erd_amd import kernels as K
    Cc, OH, OW, x, w, dz = _rand_case(card, cg, s, 4000 + 10 * cg + s)
    scale, shift, res = 0.5 + G.rand(11, Cc), G.randn(12, Cc, scale=0.2), G.randn(13, BN, OH, OW, Cc)
    Kp = 9 * cg
    out = torch.full((BN, OH, OW, Cc), float("nan"), device="cuda")
    K.conv_forward([x.cuda()], w.cuda(), [out], 3, s, 1, scale=scale.cuda(), shift=shift.cuda(), res=[res.cuda()], relu=False)
    want = R.conv_g(x, w, s, card) * scale.double() + shift.double() + res.double()
    mag = R.conv_g_abs(x, w, s, card) * scale.double().abs() + shift.double().abs() + res.double().abs()
    ratio = worst((out.cpu().double() - want).abs(), (Kp + 3) * U24 * mag)
    print(f"forward {card}x{cg} s{s}: worst err / bound {ratio:.3f}")
    assert ratio <= 1.0

    ws = w * scale.view(Cc, 1, 1, 1)        # fp32, the product the kernel forms while staging
    resx = G.randn(14, BN, BH, BW, Cc)
    dx = torch.full((BN, BH, BW, Cc), float("nan"), device="cuda")
    K.conv_dgrad([dz.cuda()], w.cuda(), [dx], 3, s, 1, res=[resx.cuda()], cardinality=card, rowscale=scale.cuda())
    want = R.conv_g_dgrad(dz, ws, (BH, BW), s, card) + resx.double()
    mag = R.conv_g_dgrad(dz.abs(), ws.abs(), (BH, BW), s, card) + resx.double().abs()
    ratio = worst((dx.cpu().double() - want).abs(), (Kp + 1) * U24 * mag)
    print(f"input gradient {card}x{cg} s{s}: worst err / bound {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("card,cg,s", BOUND_CASES)
def test_weight_gradient_within_the_any_order_bound_of_fp64(card, cg, s):
    from erd_amd import kernels as K
    Cc, OH, OW, x, w, dz = _rand_case(card, cg, s, 5000 + 10 * cg + s)
    part, S = K.conv_wgrad_partials([x.cuda()], [dz.cuda()], 3, s, 1, cardinality=card)
    dW = torch.full((Cc, 3, 3, cg), float("nan"), device="cuda")
    K.wgrad_reduce(part, S, w.cuda(), None, dW, False, None)
    n = BN * OH * OW
    ratio = worst((dW.cpu().double() - R.conv_g_wgrad(x, dz, s, card)).abs(), n * U24 * R.conv_g_wgrad(x.abs(), dz.abs(), s, card))
    print(f"weight gradient {card}x{cg} s{s} S{S}: worst err / bound {ratio:.3f}")
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------------------------------
# module level: the bounds of tests/test_gpu_functions.py
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,W,Cc,cg,s,res", [(2, 8, 10, 128, 4, 1, False), (2, 7, 9, 256, 8, 2, True), (2, 8, 10, 512, 16, 1, True),
                                                (2, 7, 9, 1024, 32, 2, False), (2, 16, 20, 256, 4, 2, False)])
def test_grouped_conv_bn_act(N, H, W, Cc, cg, s, res):
    from erd_amd import functional as Fn
    card = Cc // cg
    x = G.randn(1, N, Cc, H, W).requires_grad_(True)
    w = G.randn(2, Cc, cg, 3, 3, scale=(2.0 / (cg * 9)) ** 0.5).requires_grad_(True)
    gamma = (0.5 + G.rand(3, Cc)).requires_grad_(True)
    beta = G.randn(4, Cc, scale=0.2).requires_grad_(True)
    mean, var = G.randn(5, Cc, scale=0.2), 0.5 + G.rand(6, Cc)
    y = F.batch_norm(F.conv2d(x, w, None, s, 1, 1, card), mean, var, gamma, beta, False, 0.0, 1e-5)
    r = None
    if res:
        r = G.randn(7, *y.shape).requires_grad_(True)
        y = y + r
    y = F.relu(y)
    dy = G.randn(8, *y.shape)
    y.backward(dy)
    xg = x.detach().permute(0, 2, 3, 1).contiguous().cuda().requires_grad_(True)
    wg = cl_weight(w.detach())
    gg, bg = gamma.detach().cuda().requires_grad_(True), beta.detach().cuda().requires_grad_(True)
    rg = r.detach().permute(0, 2, 3, 1).contiguous().cuda().requires_grad_(True) if res else None
    out = Fn.ConvBNAct.apply(xg, wg, gg, bg, mean.cuda(), var.cuda(), rg, 3, s, 1, True, 1e-5)
    assert relerr(out.detach().permute(0, 3, 1, 2).cpu(), y.detach()) < 2e-5
    out.backward(dy.permute(0, 2, 3, 1).contiguous().cuda())
    assert relerr(xg.grad.permute(0, 3, 1, 2).cpu(), x.grad) < 5e-5
    assert tuple(wg.grad.shape) == (Cc, cg, 3, 3) and relerr(wg.grad.cpu(), w.grad) < 5e-5
    assert relerr(gg.grad.cpu(), gamma.grad) < 2e-4
    assert relerr(bg.grad.cpu(), beta.grad) < 5e-5
    if res:
        assert relerr(rg.grad.permute(0, 3, 1, 2).cpu(), r.grad) < 1e-6


@pytest.mark.parametrize("cin,planes,stride,down", [(256, 64, 1, False), (256, 128, 2, True), (512, 128, 1, False), (1024, 512, 2, True)])
def test_fused_resnext_bottleneck_block(cin, planes, stride, down):
    """the hand-scheduled bottleneck backward with a grouped conv2 (32x4d: 4, 8, 8 and 32 channels per group) against torch
    autograd of the reference block in fp64 (resnext.py:12-96 on resnet.py:263-302)"""
    from erd_amd.modules import Bottleneck
    N, H, W, groups = 2, 12, 14, 32
    blk = Bottleneck(cin, planes, stride, down, groups=groups, base_width=4)
    assert blk.conv2.weight.shape[1] * groups == blk.conv2.weight.shape[0] == R.resnext_width(planes, groups, 4)
    sd = {}
    for i, (k, v) in enumerate(blk.state_dict().items()):
        leaf = k.rsplit(".", 1)[-1]
        if leaf == "num_batches_tracked":
            sd[k] = v
        elif leaf == "running_var" or (leaf == "weight" and v.dim() == 1):
            sd[k] = 0.5 + G.rand(100 + i, *v.shape)
        elif v.dim() == 4:
            sd[k] = G.randn(100 + i, *v.shape, scale=(2.0 / (v.shape[1] * v.shape[2] * v.shape[3])) ** 0.5)
        else:
            sd[k] = G.randn(100 + i, *v.shape, scale=0.2)
    blk.load_state_dict(sd)
    blk = blk.cuda()
    x = G.randn(90, N, cin, H, W).double().requires_grad_(True)
    ref = {k: v.double().requires_grad_(True) if v.dtype == torch.float32 and "running" not in k else
           (v.double() if v.dtype == torch.float32 else v) for k, v in sd.items()}

    def bn(t, p):
        return F.batch_norm(t, ref[p + ".running_mean"], ref[p + ".running_var"], ref[p + ".weight"], ref[p + ".bias"], False, 0.0, 1e-5)
    o = F.relu(bn(F.conv2d(x, ref["conv1.weight"]), "bn1"))
    o = F.relu(bn(F.conv2d(o, ref["conv2.weight"], None, stride, 1, 1, groups), "bn2"))
    o = bn(F.conv2d(o, ref["conv3.weight"]), "bn3")
    idn = bn(F.conv2d(x, ref["downsample.0.weight"], None, stride), "downsample.1") if down else x
    y = F.relu(o + idn)
    dy = G.randn(91, *y.shape)
    y.backward(dy.double())
    xg = x.detach().float().permute(0, 2, 3, 1).contiguous().cuda().requires_grad_(True)
    out = blk(xg)
    assert relerr(out.detach().permute(0, 3, 1, 2).cpu(), y.detach()) < 2e-5
    out.backward(dy.permute(0, 2, 3, 1).contiguous().cuda())
    assert relerr(xg.grad.permute(0, 3, 1, 2).cpu(), x.grad) < 1e-4
    for k, p in blk.named_parameters():
        assert relerr(p.grad.cpu(), ref[k].grad) < 3e-4, k


def _x50(**kw):
    from erd_amd.modules import ResNeXt
    return ResNeXt(groups=32, base_width=4, depth=50, frozen_stages=1, norm_eval=True, **kw)


@pytest.mark.parametrize("sink", [False, True])
def test_resnext_res_layer_node_equals_the_chain_of_bottleneck_nodes(sink, monkeypatch):
    """ResLayerFn on ResNeXt stages: same outputs bit for bit and the same gradients (float-atomic order only) as the chain of per-block
    nodes, with plain autograd accumulation and with the trainer's flat gradient slots; conv2's weight gradients are launched per
    block (no grouped launch takes a cardinality > 1)"""
    from erd_amd import functional as Fn
    from erd_amd.engine import FlatParams

    def build():
        torch.manual_seed(5)
        net = _x50().cuda().train()
        with torch.no_grad():
            for m in net.modules():
                if hasattr(m, "running_var"):
                    m.running_var.uniform_(0.5, 1.5); m.running_mean.normal_(0, 0.1); m.weight.uniform_(0.5, 1.5); m.bias.normal_(0, 0.1)
        return net

    x = G.randn(7, 2, 3, 96, 128).cuda()
    res = {}
    for node in (False, True):
        monkeypatch.setattr(Fn, "RES_LAYER_NODE", node)
        net = build()
        if sink:
            named = [(n, p) for n, p in net.named_parameters() if p.requires_grad]
            named.reverse()
            flat = FlatParams(named, x.device)
            flat.zero_grad()
        outs = net(x)
        loss = sum((o.float() * G.randn(20 + i, *o.shape).cuda()).sum() for i, o in enumerate(outs))
        loss.backward()
        Fn.trail_join(x.device)
        torch.cuda.synchronize()
        res[node] = ([o.detach().clone() for o in outs], {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None})
    for a, b in zip(res[False][0], res[True][0]):
        assert torch.equal(a, b)
    assert res[False][1].keys() == res[True][1].keys() and len(res[True][1]) > 100
    for k, g in res[False][1].items():
        assert relerr(res[True][1][k].cpu(), g.cpu()) < 2e-5, k


def test_resnext50_backbone_matches_the_reference_fixture(golden):
    """stage outputs and sampled parameter gradients of the REAL reference ResNeXt-50 32x4d (tools/gen_resnext_golden.py).  Outputs: the
    activation bound of the e2e tests (1e-3 relative to the map's largest value, observed ~1e-5); gradients of the fixed weighted-sum
    loss: per tensor, the sampled entries within 5e-2 of the tensor's largest gradient entry (the per-tensor bound of test_gpu_e2e.py)."""
    g = golden("f13_resnext.npz")
    shapes = R.resnext_param_shapes(50, 32, 4)
    net = _x50()
    net.load_state_dict({k: O.procedural_tensor(0, "backbone." + k, shp) for k, shp in shapes.items()}, strict=True)
    net = net.cuda().train()
    x = torch.from_numpy(g["x"]).cuda()
    outs = net(x)
    refs = [torch.from_numpy(g[f"out{i}"]) for i in range(4)]
    for i, (o, r) in enumerate(zip(outs, refs)):
        assert tuple(o.shape) == tuple(r.shape)
        assert relerr(o.detach().cpu().contiguous(), r) < RTOL, i
    ws = R.stage_loss_weights(refs)
    sum((o * w.cuda()).sum() for o, w in zip(outs, ws)).backward()
    from erd_amd import functional as Fn
    Fn.trail_join(x.device)
    torch.cuda.synchronize()
    params = dict(net.named_parameters())
    names = [str(n) for n in g["grad_names"]]
    assert sorted(names) == sorted(k for k, p in params.items() if p.requires_grad)
    errs = []
    for n in names:
        got = params[n].grad.detach().cpu().reshape(-1)[torch.from_numpy(g["gidx." + n])]
        errs.append(float((got - torch.from_numpy(g["gval." + n])).abs().max()) / max(float(g["gmax." + n]), 1e-30))
        assert errs[-1] < 5e-2, (n, errs[-1])
    print("sampled gradient error / largest entry: median %.2e max %.2e" % (float(np.median(errs)), max(errs)))
    assert float(np.median(errs)) < 1e-3


# ------------------------------------------------------------------------------------------------------------------------
# whole steps: ResNeXt-50 32x4d teacher and student, the shapes of fixture F7's test
# ------------------------------------------------------------------------------------------------------------------------
def x50_state_dicts(c_old=40, c_all=80):
    tsd = R.resnext_gfl_state_dict(c_old, 50, 32, 4, seed=0)
    ssd = O.student_state_from_teacher(tsd, c_all, seed=1)
    for k in sorted(ssd):
        if O.trainable(k) and ssd[k].dim() == 4:
            ssd[k] = ssd[k] + 0.02 * ssd[k].abs().mean() * G.randn(700 + len(k), *ssd[k].shape)
    return tsd, ssd


def build_x50_erd(tsd, ssd):
    """teacher + student through the registry from the X-101 configs, at depth 50"""
    from erd_amd import Config, MODELS
    tcfg, scfg = Config.fromfile(CFG_X_FIRST), Config.fromfile(CFG_X_INCRE)
    tcfg.model.backbone.depth = scfg.model.backbone.depth = 50
    scfg.model.latest_model_flag = False
    teacher, student = MODELS.build(tcfg.model), MODELS.build(scfg.model)
    teacher.load_state_dict(tsd, strict=True)
    student.load_state_dict(ssd, strict=True)
    student.attach_teacher(teacher, tsd["bbox_head.gfl_cls.bias"].shape[0])
    return student.cuda().train()


def _batch(seed):
    imgs, boxes, labels = O.synthetic_batch(2, 123, 153, 40, seed=seed)
    x, metas = O.preprocess(imgs)
    return x, boxes, labels, metas


def _lossdict_to_np(d):
    return {k: np.array([float(v) for v in vs], dtype=np.float64) for k, vs in d.items()}


def test_tiny_erd_step_on_resnext50_matches_the_restatement():
    from erd_amd import kernels as K
    tsd, ssd = x50_state_dicts()
    model = build_x50_erd(tsd, ssd)
    x, boxes, labels, metas = _batch(0)
    ref, aux = R.erd_step_loss(tsd, ssd, x, boxes, labels, metas, 40, 80, 50, 32, 4, return_aux=True)
    losses = model(x.cuda(), make_samples(boxes, labels, metas), mode="loss")
    L = _lossdict_to_np(losses)
    for k, vs in ref.items():
        r = np.array([float(v) for v in vs])
        assert np.allclose(L[k], r, rtol=RTOL, atol=1e-7), (k, L[k], r)
    t_cls, t_bbox, sizes = model.ori_model._forward_cat(x.cuda())
    ers = model.sel_pos_cat(t_cls, t_bbox)
    cnt = ers["counts"].cpu()
    for i in range(2):
        assert torch.equal(ers["idx_cls"][i, :int(cnt[i, 0])].cpu(), aux["ers_cls"][i])
        assert torch.equal(ers["idx_bbox"][i, :int(cnt[i, 1])].cpu(), aux["ers_bbox"][i])
    # conv2 (and with it the whole forward) is bit-identical in the modes "f32" and "f32x3" only where no other launch differs: compare
    # the grouped layer itself on the model's own tensors
    blk = model.backbone.layer2[1]
    from erd_amd import functional as Fn
    h = torch.randn(2, 16, 20, blk.conv2.weight.shape[0], device="cuda")
    outs = {}
    try:
        for mode in ("f32", "f32x3"):
            K.set_compute(mode)
            with torch.no_grad():
                outs[mode] = blk._cba(h, blk.conv2, blk.bn2, None, True)
        assert torch.equal(outs["f32"], outs["f32x3"])
        K.set_compute("bf16")
        with pytest.raises(NotImplementedError, match="bf16"):
            with torch.no_grad():
                model.backbone(x.cuda())
    finally:
        K.set_compute(K.DEFAULT_COMPUTE)


def test_trainer_two_steps_on_resnext50_follow_the_sgd_trajectory(tmp_path):
    """ERDTrainer (flat buffers, buckets, BN prefold, prepared weights, trailing weight gradients) for two steps against the
    restatement's SGD trajectory: the second step's loss is computed from the UPDATED conv2 weights (the grouped input gradient
    reads the parameter itself: there is no prepared copy to go stale).  Then predict and a checkpoint round trip on the same model."""
    from erd_amd.engine import ERDTrainer
    from erd_amd import runner
    tsd, ssd = x50_state_dicts()
    batches = [_batch(0), _batch(1)]
    names = [k for k, v in ssd.items() if O.trainable(k) and v.dtype == torch.float32]
    model = build_x50_erd(tsd, ssd)
    tr = ERDTrainer(model, lr=0.02, momentum=0.9, weight_decay=1e-4, batch_size_per_gpu=2, auto_scale_lr=False, warmup_iters=0)
    sd = {k: v.clone() for k, v in ssd.items()}
    bufs, ref_loss = {}, []
    for it in range(2):
        x, boxes, labels, metas = batches[it]
        leaf = {k: (sd[k].clone().requires_grad_(True) if k in names else sd[k]) for k in sd}
        total = O.parse_losses(R.erd_step_loss(tsd, leaf, x, boxes, labels, metas, 40, 80, 50, 32, 4))
        total.backward()
        ref_loss.append(float(total))
        O.sgd_momentum_step({k: sd[k] for k in names}, {k: leaf[k].grad for k in names}, bufs, tr.lr_at(it), 0.9, 1e-4)
    got = []
    for it in range(2):
        x, boxes, labels, metas = batches[it]
        got.append(float(tr.train_step(x.cuda(), make_samples(boxes, labels, metas))["loss"]))
    tr.flush()
    torch.cuda.synchronize()
    assert np.allclose(got, ref_loss, rtol=2e-3), (got, ref_loss)        # per-step losses: the bound of the ResNet trajectory test
    params = dict(model.named_parameters())
    for sel, what in ((lambda k: True, "all parameters"), (lambda k: ".conv2.weight" in k, "conv2 weights")):
        ks = [k for k in names if sel(k)]
        den = sum(float((sd[k] - ssd[k]).double().pow(2).sum()) for k in ks)
        num = sum(float(((params[k].detach().cpu() - ssd[k]).double() - (sd[k] - ssd[k]).double()).pow(2).sum()) for k in ks)
        err = (num / den) ** 0.5
        print(f"2-step displacement rel L2 err, {what}: {err:.2e}")
        assert den > 0 and err < 3e-2, (what, err)      # the "f32" bound of the ResNet trajectory test
    for k, v in ssd.items():
        if k not in names and v.dtype == torch.float32:
            assert torch.equal(dict(model.state_dict())[k].cpu(), v), k

    # predict on the same model = post-processing of its own head outputs
    model.eval()
    x, boxes, labels, metas = batches[0]
    for m in metas:
        m["scale_factor"] = (0.8, 0.8)
    samples = make_samples(boxes, labels, metas)
    with torch.no_grad():
        cls, bbox = model(x.cuda(), samples, mode="tensor")
        cls, bbox = [c.clone() for c in cls], [b.clone() for b in bbox]
    out = model(x.cuda(), samples, mode="predict")
    want = O.predict_by_feat([c.cpu() for c in cls], [b.cpu() for b in bbox], metas, rescale=True)
    for d, (wb, ws_, wl) in zip(out, want):
        p = d.pred_instances
        assert len(p.scores) == len(ws_)
        assert torch.allclose(p.scores.cpu().sort(descending=True)[0], torch.as_tensor(ws_).sort(descending=True)[0], atol=1e-6)
        assert torch.equal(p.labels.cpu().sort()[0], torch.as_tensor(wl).sort()[0])

    # a checkpoint saved and reloaded gives bit-equal outputs
    path = str(tmp_path / "x50.pth")
    runner.save_checkpoint(path, model, tr)
    fresh = build_x50_erd(tsd, ssd).eval()
    runner.load_checkpoint(path, fresh)
    with torch.no_grad():
        cls2, bbox2 = fresh(x.cuda(), samples, mode="tensor")
    for a, b in zip(list(cls) + list(bbox), list(cls2) + list(bbox2)):
        assert torch.equal(a, b)


def test_resnext_teacher_hipgraph_replay_equals_eager():
    """the grouped launches inside the captured teacher (engine.TeacherGraphs): replays on new pixels give the eager pass's teacher
    logits and ERS index lists bit for bit"""
    from erd_amd.engine import TeacherGraphs
    tsd, ssd = x50_state_dicts()
    model = build_x50_erd(tsd, ssd)
    tg = TeacherGraphs(model)
    side = torch.cuda.Stream()
    for i in range(3):
        x = G.randn(40 + i, 2, 3, 96, 128).cuda()
        with torch.no_grad():
            ref = model.teacher_pass(x)
        want = [t.clone() for t in ref.tensors()]
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            got = tg.run(x)
        torch.cuda.current_stream().wait_stream(side)
        assert got.sizes == ref.sizes
        for a, b in zip(got.tensors(), want):
            if a.dtype == torch.int64 and a.dim() == 2:       # ERS index lists: only the first count entries are defined
                continue
            assert torch.equal(a, b), i
        cnt = got.ers["counts"].cpu()
        for n in range(2):
            for k, name in enumerate(("idx_cls", "idx_bbox")):
                assert torch.equal(got.ers[name][n, :int(cnt[n, k])], ref.ers[name][n, :int(cnt[n, k])])
    assert len(tg.graphs) == 1
