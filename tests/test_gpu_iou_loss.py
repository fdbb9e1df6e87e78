"""GPU: IoULoss / DIoULoss / CIoULoss as the head's loss_bbox -- the stand-alone operator erd_iou_loss (C ABI and the registered
modules), the fused chain of a training step through erd_gfl_losses_fwd_box / _bwd_box on given targets, a whole tiny step against
the oracle under iou_refs.swap_box_loss, and two optimisation steps of the _ciou config.  References, row scales, case tables, the
exclusion condition and the rule (FACTOR = 4 x E32 per kind) are tests/iou_refs.py, proved on the CPU by tests/test_iou_refs_cpu.py.
Every output starts NaN-filled; every figure is printed before it is asserted.

Measured on an MI355X (kernel figure / E32): see the lines this file prints; EXPERIMENTS.md records them."""
import ctypes as C
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import iou_refs as IR
import leaf_refs as R
import loss_refs as LR
from e2e_util import CFG_FIRST, CFG_INCRE, ROOT, build_erd, f7_state_dicts, make_samples
from oracle import erd_oracle as O
from test_gpu_loss_exact import _iarr, _same_sums, dev, nan, shifted

F32, F64 = R.F32, R.F64
HALF_ULP = 2.0 ** -24
CFG_CIOU = os.path.join(ROOT, "configs", "gfl_increment", "gfl_r50_fpn_1x_coco_first_40_incre_last_40_cats_ciou.py")
MODULE_OF = {"iou_log": dict(type="IoULoss", mode="log"), "iou_linear": dict(type="IoULoss", mode="linear"),
             "iou_square": dict(type="IoULoss", mode="square"), "diou": dict(type="DIoULoss"), "ciou": dict(type="CIoULoss")}


@pytest.fixture(scope="module")
def L():
    from erd_amd import MODELS, _lib, functional, leaf
    from erd_amd import kernels as K
    _lib.load()
    return NS(call=_lib.call, p=K._p, s=K._stream, Err=_lib.ErdHipError, K=K, MODELS=MODELS, leaf=leaf, functional=functional)


def _report(what, kind, part, e, got):
    print(f"\n[iou] {what:10s} {kind:11s} {part:9s} E32 {e:.3e}  kernel {got:.3e}  ratio {got / e if e else float('inf'):.2f}")


# ---- the stand-alone operator --------------------------------------------------------------------------------------------
def _abi(L, kind, c, eps=IR.EPS):
    """rows only, dpred only and both: the same bits each way"""
    pred, target, coef = dev(c.pred), dev(c.target), dev(c.coef)
    kid = IR.KIND_ID[kind]
    rows_f, rows_b, d_g, d_b = nan(c.n), nan(c.n), nan(c.n, 4), nan(c.n, 4)
    L.call("erd_iou_loss", L.p(pred), L.p(target), None, c.n, kid, eps, L.p(rows_f), None, L.s())
    L.call("erd_iou_loss", L.p(pred), L.p(target), L.p(coef), c.n, kid, eps, None, L.p(d_g), L.s())
    L.call("erd_iou_loss", L.p(pred), L.p(target), L.p(coef), c.n, kid, eps, L.p(rows_b), L.p(d_b), L.s())
    torch.cuda.synchronize()
    same = lambda a, b: torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0)) and torch.equal(torch.isnan(a), torch.isnan(b))
    assert same(rows_f, rows_b) and same(d_g, d_b), (kind, c.name)
    return rows_b.cpu(), d_b.cpu()


@pytest.mark.parametrize("kind", IR.KINDS)
def test_iou_loss_rows_and_gradient_through_the_abi(L, kind):
    got = {}

    def run(c):
        got[c.name] = _abi(L, kind, c)
        return got[c.name]
    er, eg = IR.e32(kind)
    fr, fg = IR.figures(kind, run)
    _report("erd_iou_loss", kind, "rows", er, fr)
    _report("erd_iou_loss", kind, "gradient", eg, fg)
    for c, rows, grad, rs, gs, excl in IR.ref64(kind):
        r, g = got[c.name]
        # the exclusion condition: not finite on the GPU exactly where the CPU fp32 evaluation is not finite
        assert torch.equal(~torch.isfinite(r), excl) and torch.equal(~torch.isfinite(g).all(1), excl), (kind, c.name)
        zero = (c.coef == 0) & ~excl
        assert bool((g[zero] == 0).all()), (kind, c.name)                  # zero coef rows: an exact zero gradient
    assert fr <= R.FACTOR * er, (kind, "rows", fr, er)
    assert fg <= R.FACTOR * eg, (kind, "gradient", fg, eg)


def test_iou_loss_refusals_and_zero_rows(L):
    b = nan(8)
    for kid, eps in ((0, 1e-6), (6, 1e-6), (-1, 1e-6), (5, -1.0)):        # GIoU is erd_giou; unknown kinds; a negative eps
        with pytest.raises(L.Err):
            L.call("erd_iou_loss", L.p(b), L.p(b), L.p(b), 1, kid, eps, L.p(b), L.p(b), L.s())
    with pytest.raises(L.Err):
        L.call("erd_iou_loss", None, L.p(b), None, 1, 1, 1e-6, L.p(b), None, L.s())
    L.call("erd_iou_loss", None, None, None, 0, 1, 1e-6, None, None, L.s())                 # zero rows: nothing to do
    torch.cuda.synchronize()
    assert bool(torch.isnan(b).all())
    # a module eps that is not the default reaches the kernel
    c = IR.cases()[3]
    for kind, eps in (("iou_log", 0.3), ("diou", 0.5), ("ciou", 0.25)):
        rows, grad = _abi(L, kind, c, eps)
        r64, g64 = IR.restate(kind, c, F64, eps=eps)
        rs, gs = IR.scales(kind, c, eps)
        er, eg = IR.e32(kind)
        assert R.nerr(rows, r64, rs) <= R.FACTOR * er and R.nerr(grad, g64, gs) <= R.FACTOR * eg, (kind, eps)
        assert not torch.equal(rows, _abi(L, kind, c)[0])


@pytest.mark.parametrize("kind", IR.KINDS)
def test_modules_forward_and_backward(L, kind):
    """reductions none / mean / sum, with and without avg_factor, [n] and [n, 4] weights, the all-zero weight: value and gradient
    against the fp64 restatement of the module's forward.  A reduced value may deviate by 4 x E32 x the weighted sum of its rows'
    scales (the triangle inequality) plus the half ulp of its one rounding to fp32."""
    lw = 2.0
    mod = L.MODELS.build(dict(MODULE_OF[kind], loss_weight=lw))
    er, eg = IR.e32(kind)
    worst_v = worst_g = 0.0
    for c, rows64, grad64, rs, gs, excl in IR.ref64(kind):
        for reduction, avg_factor, form in IR.MODULE_RUNS:
            w = IR.module_weight(c, form)
            tag = (kind, c.name, reduction, avg_factor, form)
            p = dev(c.pred).requires_grad_(True)
            out = mod(p, dev(c.target), weight=dev(w), avg_factor=avg_factor, reduction_override=reduction)
            p64 = R._leaf(c.pred, F64)
            ref = IR.module_forward(kind, p64, c.target.double(), None if w is None else w.double(), avg_factor, reduction, lw)
            assert out.shape == ref.shape, tag
            up = torch.randn(ref.shape, generator=R._gen(8800), dtype=F64) if ref.dim() else torch.tensor(1.7, dtype=F64)
            out.backward(dev(up.float()))
            (ref * up).sum().backward()
            got, g = out.detach().cpu(), p.grad.cpu()
            if form in ("zero", "zero4") and (reduction != "none" or not kind.startswith("iou_")):
                assert got.dim() == 0 and float(got) == 0.0 and bool((g == 0).all()), tag          # exact 0, an all-zero gradient
                continue
            w1 = torch.ones(c.n, dtype=F64) if w is None else (w.double().mean(-1) if w.dim() > 1 else w.double())
            scale = R.reduce_scale(reduction, avg_factor, c.n, lw)
            keep = ~excl
            if scale is None:                                                        # reduction='none': rows
                assert torch.equal(~torch.isfinite(got), excl), tag
                fv = R.nerr(got[keep], ref.detach()[keep], lw * w1[keep] * rs[keep])
                coef = up * lw * w1
            else:
                if bool(excl.any()):
                    assert not bool(torch.isfinite(got)), tag                         # a row that is not finite makes the sum so
                    continue
                mag = float((rs * w1.abs()).sum()) * abs(scale)
                fv = max(0.0, abs(float(got) - float(ref)) - HALF_ULP * abs(float(ref))) / max(mag, R.TINY)
                coef = float(up) * scale * w1
            gscale = IR.scales(kind, NS(pred=c.pred, target=c.target, coef=coef, n=c.n))[1]
            fg = R.nerr(g[keep], p64.grad[keep], gscale[keep])
            worst_v, worst_g = max(worst_v, fv), max(worst_g, fg)
            assert fv <= R.FACTOR * er and fg <= R.FACTOR * eg, tag + (fv, er, fg, eg)
    _report("module", kind, "value", er, worst_v)
    _report("module", kind, "gradient", eg, worst_g)


# ---- the fused chain on given targets ---------------------------------------------------------------------------------------
def run_chain(L, c, kind, new_entries=True):
    """test_gpu_loss_exact.run_chain with the box-loss kind: erd_gfl_losses_fwd_box, erd_loss_avg, erd_l2_distill, erd_kd_kl,
    erd_loss_finalize (losses), erd_loss_finalize (coefficients under `up`), erd_gfl_losses_bwd_box, erd_l2_distill_bwd,
    erd_kd_kl_bwd; `new_entries=False` (GIoU only): the entries without the kind"""
    N, A, nl, c_old, c_all = c.N, c.A, c.nlvl, c.c_old, c.c_all
    p, s = L.p, L.s
    kid = IR.KIND_ID[kind]
    tail = (kid, IR.EPS) if new_entries else ()
    sfx = "_box" if new_entries else ""
    assert new_entries or kind == "giou"
    cls, bbox = shifted(c.cls, c.cls_shift), dev(c.bbox)
    anchors, labels, lw, bt = dev(c.anchors), dev(c.labels), dev(c.lw), dev(c.bt)
    off, strides = _iarr(LR.lvl_off(c.sizes), C.c_int64), _iarr(c.strides, C.c_int)
    lw_cls, lw_bbox, lw_dfl, lw_ld, w_dist = c.weights
    score, wt, sums = nan(N, A), nan(N, A), nan(nl, 4, dtype=F64)
    fwd = lambda: L.call("erd_gfl_losses_fwd" + sfx, p(cls), p(bbox), p(anchors), p(labels), p(lw), p(bt), off, strides, nl, N, A, c_old,
                         c_all, p(score), p(wt), p(sums), *tail, s())
    fwd()
    once = sums.clone()
    fwd()
    assert _same_sums(once, sums), c.name
    avg, npos = nan(2), dev(c.num_pos)
    L.call("erd_loss_avg", p(npos), N, p(sums), nl, p(avg), s())
    nd = N if c.distill else 0
    l2s = kds = counts = None
    if c.distill:
        t_cls, t_bbox, idx, counts, keep = dev(c.t_cls), dev(c.t_bbox), dev(c.idx_cls), dev(c.counts), dev(c.keep)
        l2s, kds = nan(N, dtype=F64), nan(N, dtype=F64)
        L.call("erd_l2_distill", p(cls), p(t_cls), p(idx), p(counts), N, A, c_all, c.c_t, c_old, p(l2s), s())
        L.call("erd_kd_kl", p(bbox), p(t_bbox), p(cls), p(keep), N, A, c_all, c_old, c.T, p(kds), s())
    losses, coef = nan(3 * nl + 2 * nd), nan(4 * nl + 2 * nd)
    up = dev(c.up)
    fin = lambda upv, lo, co: L.call("erd_loss_finalize", p(sums), p(avg), p(l2s), p(kds), p(counts), nl, nd, c_old, w_dist, lw_cls, lw_bbox,
                                     lw_dfl, lw_ld, p(upv), p(lo), p(co), s())
    fin(None, losses, None)
    fin(up, None, coef)
    dcls = shifted(torch.full(c.cls.shape, float("nan")), c.cls_shift)
    dbbox = nan(N, A, 68)
    L.call("erd_gfl_losses_bwd" + sfx, p(cls), p(bbox), p(anchors), p(labels), p(lw), p(bt), off, strides, nl, N, A, c_old, c_all, p(score),
           p(wt), p(coef), p(dcls), p(dbbox), *tail, s())
    if c.distill:
        L.call("erd_l2_distill_bwd", p(cls), p(t_cls), p(idx), p(counts), p(coef[4 * nl:]), N, A, c_all, c.c_t, c_old, p(dcls), s())
        L.call("erd_kd_kl_bwd", p(bbox), p(t_bbox), p(cls), p(keep), p(coef[4 * nl + N:]), N, A, c_all, c_old, c.T, p(dbbox), s())
    torch.cuda.synchronize()
    g = NS()
    for k, v in (("score", score), ("wt", wt), ("sums", sums), ("avg", avg), ("losses", losses), ("coef", coef), ("dcls", dcls), ("dbbox", dbbox),
                 ("l2s", l2s), ("kds", kds)):
        setattr(g, k, None if v is None else v.cpu().clone())
    return g


def _same_run(a, b, c, box=True):
    """two runs of the chain agree: bit for bit, but for what hangs on an f64 atomic sum of many rows (the QFL, L2 and KD-KL sums and
    the loss entries made of them), where two runs of the SAME entry agree only to the reassociation of f64.  box=False: the box term
    (sums[:, 1], loss_bbox, dbbox) is left out"""
    nl = c.nlvl
    for k in ("score", "wt", "avg", "dcls") + (("dbbox", "coef") if box else ()):
        assert torch.equal(getattr(a, k), getattr(b, k)), (c.name, k)
    cols = [1, 2, 3] if box else [2, 3]
    assert torch.equal(a.sums[:, cols], b.sums[:, cols]) and _same_sums(a.sums[:, 0], b.sums[:, 0]), c.name
    exact = list(range(nl, 3 * nl)) if box else list(range(2 * nl, 3 * nl))
    assert torch.equal(a.losses[exact], b.losses[exact]), c.name
    rest = [j for j in range(len(a.losses)) if not nl <= j < 3 * nl]
    assert torch.allclose(a.losses[rest], b.losses[rest], rtol=2.0 ** -22, atol=0), c.name
    if c.distill:
        assert _same_sums(a.l2s, b.l2s) and _same_sums(a.kds, b.kds), c.name


@pytest.fixture(scope="module")
def giou_runs(L):
    """GIoU through the entries without the kind: the run every other kind is compared with, computed once"""
    return [run_chain(L, c, "giou", new_entries=False) for c in IR.chain_cases()]


def test_giou_through_the_new_entries_is_the_old_entries_bit_for_bit(L, giou_runs):
    for c, old in zip(IR.chain_cases(), giou_runs):
        new = run_chain(L, c, "giou")
        _same_run(old, new, c)
    b = nan(4 * 68)
    off, strides = _iarr([0, 1], C.c_int64), _iarr([8], C.c_int)
    il, dd, z = L.p(nan(8, dtype=torch.int64)), L.p(nan(8, dtype=F64)), L.p(b)
    for kid, eps in ((0, 1e-7), (6, 1e-6), (-1, 1e-6), (4, -1.0)):         # GIoU at another eps, unknown kinds, a negative eps
        with pytest.raises(L.Err):
            L.call("erd_gfl_losses_fwd_box", z, z, z, il, z, z, off, strides, 1, 1, 1, 0, 4, z, z, dd, kid, eps, L.s())
        with pytest.raises(L.Err):
            L.call("erd_gfl_losses_bwd_box", z, z, z, il, z, z, off, strides, 1, 1, 1, 0, 4, z, z, z, z, z, kid, eps, L.s())
    torch.cuda.synchronize()
    assert bool(torch.isnan(b).all())


@pytest.mark.parametrize("kind", IR.KINDS)
def test_the_chain_of_a_step_under_each_kind(L, giou_runs, kind):
    E = IR.chain_e32(kind)
    worst = {"giou": 0.0, "dbbox": 0.0, "loss_bbox": 0.0}
    for i, (c, base) in enumerate(zip(IR.chain_cases(), giou_runs)):
        g = run_chain(L, c, kind)
        r = IR.chain_ref64(kind, i)
        nl, N = c.nlvl, c.N
        # the kind leaks into nothing but the box term: bit-equal to the GIoU run of the same case
        _same_run(base, g, c, box=False)
        f = LR._row_figures(c, r, g)
        worst["giou"], worst["dbbox"] = max(worst["giou"], f["giou"]), max(worst["dbbox"], f["dbbox"])
        a2 = max(float(r.avg[1]), 1.0)
        for l in range(nl):
            cb = c.weights[1] / (1.0 + R.EPS32) / a2
            mag = float(r.scale.sums[l, 1]) * cb
            err = abs(float(g.losses[nl + l]) - float(r.losses[nl + l]))
            # loss_bbox[l] is four fp32 roundings of the f64 sum (cast, two divisions, one product): 4 half ulps beside the rule
            assert err <= R.FACTOR * E["giou"] * mag + 4 * HALF_ULP * abs(float(r.losses[nl + l])), (kind, c.name, l, err, mag)
            worst["loss_bbox"] = max(worst["loss_bbox"], max(0.0, err - 4 * HALF_ULP * abs(float(r.losses[nl + l]))) / max(mag, R.TINY))
        if int(c.num_pos.sum()) == 0:          # no positive: exact zeros
            assert bool((g.sums[:, 1:] == 0).all()) and bool((g.losses[nl:3 * nl] == 0).all()), (kind, c.name)
            assert bool((g.score == 0).all()) and bool((g.wt == 0).all()), (kind, c.name)
            untouched = (c.keep == 0) if c.distill else torch.ones(N, c.A, dtype=torch.bool)
            assert bool((g.dbbox[untouched] == 0).all()), (kind, c.name)
        else:
            assert not torch.equal(g.sums[:, 1], base.sums[:, 1]) and not torch.equal(g.dbbox, base.dbbox), (kind, c.name)
        assert f["giou"] <= R.FACTOR * E["giou"] and f["dbbox"] <= R.FACTOR * E["dbbox"], (kind, c.name, f["giou"], f["dbbox"], E)
    _report("chain", kind, "box sums", E["giou"], worst["giou"])
    _report("chain", kind, "loss_bbox", E["giou"], worst["loss_bbox"])
    _report("chain", kind, "dbbox", E["dbbox"], worst["dbbox"])


def test_erdlossfn_carries_the_kind(L):
    """functional.ERDLossFn with `box_loss` on the targets namespace runs the chain of that kind; without it, GIoU"""
    c = IR.chain_cases()[0]
    for kind in ("giou", "ciou"):
        s_cls, s_bbox = dev(c.cls).requires_grad_(True), dev(c.bbox).requires_grad_(True)
        t = NS(sizes=c.sizes, strides=c.strides, anchors=dev(c.anchors), labels=dev(c.labels), label_weights=dev(c.lw), bbox_targets=dev(c.bt),
               c_old=c.c_old, num_pos=dev(c.num_pos), world_size=1, distill=True, t_cls=dev(c.t_cls), t_bbox=dev(c.t_bbox),
               ers=dict(idx_cls=dev(c.idx_cls), counts=dev(c.counts)), keep=dev(c.keep), T=c.T, dist_loss_weight=c.weights[4], lw_cls=c.weights[0],
               lw_bbox=c.weights[1], lw_dfl=c.weights[2], lw_ld=c.weights[3])
        if kind != "giou":
            t.box_loss = (IR.KIND_ID[kind], IR.EPS)
        losses = L.functional.ERDLossFn.apply(s_cls, s_bbox, t)
        losses.backward(gradient=dev(c.up))
        g = run_chain(L, c, kind)
        nl = c.nlvl
        assert torch.equal(losses.detach().cpu()[nl:3 * nl], g.losses[nl:3 * nl]) and torch.equal(s_bbox.grad.cpu(), g.dbbox), kind


# ---- a whole tiny step ---------------------------------------------------------------------------------------------------------
@pytest.mark.usefixtures("oracle_threads")
@pytest.mark.parametrize("name,kind", [("IoULoss", "iou_log"), ("DIoULoss", "diou"), ("CIoULoss", "ciou")])
def test_tiny_step_against_the_oracle_under_swap_box_loss(tmp_path, name, kind):
    """the F7 state dicts, the ragged batch and the bounds of tests/test_gpu_e2e.py::test_live_oracle_ragged_batch (its GIoU step),
    with the student's loss_bbox set to each type: LossDict and all parameter gradients against O.erd_step_loss"""
    from erd_amd import parse_losses
    from test_gpu_e2e import RTOL, _lossdict_to_np
    import golden_inputs as G
    cfg = tmp_path / f"incre_{kind}.py"
    cfg.write_text(f"_base_ = [{CFG_INCRE!r}]\nmodel = dict(bbox_head=dict(loss_bbox=dict(_delete_=True, type={name!r}, loss_weight=2.0)))\n")
    tsd, ssd = f7_state_dicts()
    model = build_erd(tsd, ssd, cfg_incre=str(cfg))
    assert type(model.bbox_head.loss_bbox).__name__ == name
    rng = np.random.RandomState(5)
    imgs = [torch.from_numpy(rng.randint(0, 255, size=(3, h, w), dtype=np.uint8)) for h, w in [(150, 200), (131, 217), (160, 180)]]
    boxes = [G.rand_boxes(900 + i, 2 + i, 170.0, 125.0, min_size=10.0) for i in range(3)]
    labels = [G.randint(910 + i, 0, 40, 2 + i) for i in range(3)]
    x, metas = O.preprocess(imgs)
    sd = {k: (v.clone().requires_grad_(True) if O.trainable(k) and v.dtype == torch.float32 else v) for k, v in ssd.items()}
    with IR.swap_box_loss(kind):
        ref_losses = O.erd_step_loss(tsd, sd, x, boxes, labels, metas, 40, 80)
        O.parse_losses(ref_losses).backward()
    losses = model(x.cuda(), make_samples(boxes, labels, metas), mode="loss")
    Ld = _lossdict_to_np(losses)
    for k, vs in ref_losses.items():
        r = np.array([float(v) for v in vs])
        print(f"\n[iou] step {kind} {k}: hip {Ld[k]} oracle {r}")
        assert np.allclose(Ld[k], r, rtol=RTOL, atol=1e-7), (k, Ld[k], r)
    total, _ = parse_losses(losses)
    total.backward()
    params = dict(model.named_parameters())
    errs, num, den = [], 0.0, 0.0
    for k, v in sd.items():
        if not (O.trainable(k) and v.dtype == torch.float32):
            continue
        a, b = params[k].grad.cpu().double(), v.grad.double()
        num += float((a - b).pow(2).sum())
        den += float(b.pow(2).sum())
        if float(b.norm()) > 1e-12:
            errs.append(float((a - b).norm() / b.norm()))
            assert errs[-1] < 5e-2, (k, errs[-1])
    print("\n[iou] step %s grad rel L2: median %.2e max %.2e global %.2e" % (kind, float(np.median(errs)), max(errs), (num / den) ** 0.5))
    assert float(np.median(errs)) < 1e-3 and (num / den) ** 0.5 < 2e-2, (float(np.median(errs)), (num / den) ** 0.5)
    # the fp64 anchor of that test: as close to fp64 as the reference's own fp32 arithmetic is
    t64 = {k: (v.double() if v.is_floating_point() else v) for k, v in tsd.items()}
    s64 = {k: (v.double() if v.is_floating_point() else v) for k, v in ssd.items()}
    s64 = {k: (v.clone().requires_grad_(True) if O.trainable(k) and v.is_floating_point() else v) for k, v in s64.items()}
    with IR.swap_box_loss(kind):
        O.parse_losses(O.erd_step_loss(t64, s64, x.double(), boxes, labels, metas, 40, 80)).backward()

    def to64(g):
        errs, num, den = [], 0.0, 0.0
        for k, v in s64.items():
            if v.grad is None or float(v.grad.norm()) < 1e-12:
                continue
            a, b = g(k), v.grad
            errs.append(float((a - b).norm() / b.norm()))
            num += float((a - b).pow(2).sum()); den += float(b.pow(2).sum())
        return float(np.median(errs)), (num / den) ** 0.5, max(errs)

    hip64 = to64(lambda k: params[k].grad.cpu().double())
    cpu64 = to64(lambda k: sd[k].grad.double())
    print("\n[iou] step %s rel L2 to fp64 (median / all elements / worst tensor): cpu fp32 %.2e %.2e %.2e | hip %.2e %.2e %.2e" % ((kind,) + cpu64 + hip64))
    assert hip64[1] <= max(1e-3, 1.5 * cpu64[1]) and hip64[0] <= max(1e-3, 1.5 * cpu64[0]) and hip64[2] <= max(1e-2, 1.5 * cpu64[2]), (hip64, cpu64)


# ---- the trainer ---------------------------------------------------------------------------------------------------------------
def test_two_optimisation_steps_of_the_ciou_config(tmp_path):
    """the _ciou config through the Runner on synthetic data (what tools/train.py --synthetic builds) at the F7 size: finite
    losses, a loss_bbox that is not the GIoU run's of the same seed, and a checkpoint whose keys are the GIoU config's (loss
    modules hold no parameters) and that loads back"""
    from erd_amd import Config
    from erd_amd.runner import Runner, SyntheticDetData, load_checkpoint
    teacher = tmp_path / "teacher.pth"
    torch.save(dict(state_dict=O.procedural_state_dict(40, seed=0)), teacher)

    def run(path, work):
        cfg = Config.fromfile(path)
        cfg.work_dir = str(tmp_path / work)
        cfg.merge_from_dict({"train_dataloader.batch_size": 2, "train_cfg.max_epochs": 1, "model.backbone.init_cfg": None,
                             "default_hooks.logger.interval": 1, "model.ori_setting.ori_checkpoint_file": str(teacher),
                             "model.ori_setting.ori_config_file": CFG_FIRST})
        torch.manual_seed(5)
        r = Runner.from_cfg(cfg, data=SyntheticDetData(2, 40, 2, image_hw=(150, 200), seed=1), log=lambda *_: None)
        return r, r.train()

    rc, hc = run(CFG_CIOU, "ciou")
    rg, hg = run(CFG_INCRE, "giou")
    assert type(rc.model.bbox_head.loss_bbox).__name__ == "CIoULoss" and type(rg.model.bbox_head.loss_bbox).__name__ == "GIoULoss"
    assert len(hc) == 2 and len(hg) == 2
    for rec in hc:
        print("\n[iou] trainer ciou", {k: round(v, 5) for k, v in rec.items() if "loss" in k})
        assert all(np.isfinite(v) for k, v in rec.items() if "loss" in k)
    assert hc[0]["loss_bbox"] != hg[0]["loss_bbox"] and abs(hc[0]["loss_bbox"] - hg[0]["loss_bbox"]) > 1e-4 * abs(hg[0]["loss_bbox"])
    assert hc[0]["loss_cls"] == pytest.approx(hg[0]["loss_cls"], rel=1e-5) and hc[0]["loss_dfl"] == pytest.approx(hg[0]["loss_dfl"], rel=1e-5)
    ck = torch.load(tmp_path / "ciou" / "epoch_1.pth", map_location="cpu", weights_only=False)
    ckg = torch.load(tmp_path / "giou" / "epoch_1.pth", map_location="cpu", weights_only=False)
    assert list(ck["state_dict"]) == list(ckg["state_dict"])
    load_checkpoint(str(tmp_path / "ciou" / "epoch_1.pth"), rg.model)                       # round trip into the GIoU model: same keys
    for k, v in rg.model.state_dict().items():
        assert torch.equal(v.cpu(), ck["state_dict"][k]), k
