"""GPU: the 14 kernels of erd_amd/csrc/leaf_ops.hip at their edges, through the C ABI and through erd_amd/leaf.py and the
registered modules.  References, row scales, case tables and the rule are tests/leaf_refs.py (proved on the CPU by
tests/test_leaf_refs_cpu.py); tests/test_gpu_modules.py stays the tie to the real reference's fixture.

  * QFL, DFL, KD-KL, Integral (forward and backward) and the GIoU gradient: the kernel's worst row-normalised error against the
    fp64 oracle is at most 4 x E32, the same figure of the fp32 oracle on the CPU.  Both are printed.
  * overlaps, GIoU rows, distance2bbox (forward and backward), bbox2distance, rows_mul, loss_coef, atss_result: bit-equal to the
    fp32 expression in the kernel's operation order; weighted_sum: the one right fp32 value of an exact f64 sum.
  * every output the test allocates starts NaN-filled.
  * zero rows: null pointers are legal exactly when there is nothing to do.  A launch of zero blocks is an invalid configuration,
    which the entry point would report: a zero return with null pointers therefore also says that nothing was launched."""
import copy
from types import SimpleNamespace as NS

import pytest
import torch

pytestmark = pytest.mark.gpu

import leaf_refs as R

F32, F64 = R.F32, R.F64
NAN = float("nan")


@pytest.fixture(scope="module")
def L():
    from erd_amd import MODELS, TASK_UTILS, _lib, leaf
    from erd_amd import kernels as K
    _lib.load()
    return NS(call=_lib.call, p=K._p, s=K._stream, Err=_lib.ErdHipError, MODELS=MODELS, TASK_UTILS=TASK_UTILS, leaf=leaf)


def nan(*shape, dtype=F32):
    if dtype == torch.int64:
        return torch.full(shape, -7777, dtype=dtype, device="cuda")
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


def dev(t):
    return None if t is None else t.contiguous().cuda()


def _report(op, what, e, got):
    print(f"\n[leaf] {op:8s} {what:5s} E32 {e:.3e}  kernel {got:.3e}  ratio {got / e if e else float('inf'):.2f}")


def _rule(op, fn, rows_rule=True):
    er, eg = R.e32(op)
    fr, fg = R.figures(op, fn)
    _report(op, "rows", er, fr)
    _report(op, "grad", eg, fg)
    torch.cuda.synchronize()
    if rows_rule:
        assert fr <= R.FACTOR * er, (op, "rows", fr, er)
    assert fg <= R.FACTOR * eg, (op, "grad", fg, eg)


# ---- through the C ABI: the operators under the 4 x E32 rule ---------------------------------------------------------
def test_qfl_rows_and_bwd(L):
    def run(c):
        pred, label, score, coef = dev(c.pred), dev(c.label), dev(c.score), dev(c.coef)
        rows, d = nan(c.n), nan(c.n, c.C)
        L.call("erd_qfl_rows", L.p(pred), L.p(label), L.p(score), c.n, c.C, L.p(rows), L.s())
        L.call("erd_qfl_bwd", L.p(pred), L.p(label), L.p(score), L.p(coef), c.n, c.C, L.p(d), L.s())
        return rows.cpu(), d.cpu()
    _rule("qfl", run)


def _three_ways(call3, n_rows, grad_shape):
    """forward only, backward only and both pointers of an entry point with the rows / dpred pair: the same bits each way"""
    rows_f, rows_b, d_g, d_b = nan(n_rows), nan(n_rows), nan(*grad_shape), nan(*grad_shape)
    call3(rows_f, None)
    call3(None, d_g)
    call3(rows_b, d_b)
    assert torch.equal(rows_f, rows_b) and torch.equal(d_g, d_b) and not torch.isnan(rows_b).any() and not torch.isnan(d_b).any()
    return rows_b.cpu(), d_b.cpu()


def test_dfl(L):
    def run(c):
        pred, target, coef = dev(c.pred), dev(c.target), dev(c.coef)
        return _three_ways(lambda rows, d: L.call("erd_dfl", L.p(pred), L.p(target), L.p(coef if d is not None else None), c.m, c.nb,
                                                  L.p(rows), L.p(d), L.s()), c.m, (c.m, c.nb))
    _rule("dfl", run)


def test_kd_kl_rows(L):
    def run(c):
        pred, soft, coef = dev(c.pred), dev(c.soft), dev(c.coef)
        rows, d = _three_ways(lambda rows, d: L.call("erd_kd_kl_rows", L.p(pred), L.p(soft), L.p(coef if d is not None else None), c.m,
                                                     c.nb, c.T, L.p(rows), L.p(d), L.s()), c.m, (c.m, c.nb))
        same = (c.pred == c.soft).all(1)             # soft == pred: the row and its gradient are exactly 0
        assert bool((d[same] == 0).all()) and bool((rows[same] == 0).all())
        return rows, d
    _rule("kd", run)


def test_integral(L):
    def run(c):
        x, dy = dev(c.x), dev(c.dy)
        return _three_ways(lambda y, dx: L.call("erd_integral", L.p(x), L.p(dy if dx is not None else None), c.m, c.nb, L.p(y),
                                                L.p(dx), L.s()), c.m, (c.m, c.nb))
    _rule("integral", run)


def test_giou_rows_equal_and_gradient(L):
    def run(c):
        pred, target, coef = dev(c.pred), dev(c.target), dev(c.coef)
        rows, d = _three_ways(lambda rows, d: L.call("erd_giou", L.p(pred), L.p(target), L.p(coef if d is not None else None), c.n,
                                                     c.eps, L.p(rows), L.p(d), L.s()), c.n, (c.n, 4))
        assert torch.equal(rows, R.giou_restate(c)[0]), c.name
        return rows, d
    _rule("giou", run, rows_rule=False)


# ---- through the C ABI: the operators under the equality rule -------------------------------------------------------
def _overlaps(L, a, b, aligned, mode):
    m, n = a.shape[0], b.shape[0]
    out = nan(m) if aligned else nan(m, n)
    A, Bx = dev(a), dev(b)
    L.call("erd_bbox_overlaps", L.p(A), L.p(Bx), m, n, int(aligned), int(mode == "giou"), R.BOX_EPS, L.p(out), L.s())
    return out.cpu()


def test_overlaps_aligned_and_pairwise_equal(L):
    for c in R.giou_cases():
        for mode in ("iou", "giou"):
            assert torch.equal(_overlaps(L, c.pred, c.target, True, mode), R.overlaps_restate(c.pred, c.target, mode, True)), (c.name, mode)
    for m, n in R.PAIR_SHAPES:
        a, b = R.pair_boxes(m, n)
        for mode in ("iou", "giou"):
            got = _overlaps(L, a, b, False, mode)
            assert got.shape == (m, n) and torch.equal(got, R.overlaps_restate(a, b, mode, False)), (m, n, mode)


@pytest.mark.parametrize("max_shape", [None, R.MAX_SHAPE])
def test_distance2bbox_forward_and_backward_equal(L, max_shape):
    mh, mw = (-1.0, -1.0) if max_shape is None else (float(max_shape[0]), float(max_shape[1]))
    for n in R.CODER_N:
        c = R.d2b_case(n)
        box, grad = R.d2b_oracle(c, max_shape, F32)
        pts, dist, dout = dev(c.pts), dev(c.dist), dev(c.dout)
        for fwd, bwd in ((1, 0), (0, 1), (1, 1)):
            out, dd = (nan(n, 4) if fwd else None), (nan(n, 4) if bwd else None)
            L.call("erd_distance2bbox", L.p(pts), L.p(dist), L.p(dout if bwd else None), n, mh, mw, L.p(out), L.p(dd), L.s())
            assert not fwd or torch.equal(out.cpu(), box), (n, max_shape)
            assert not bwd or torch.equal(dd.cpu(), grad), (n, max_shape)


@pytest.mark.parametrize("max_dis,eps", R.B2D_PARAMS)
def test_bbox2distance_equal(L, max_dis, eps):
    for n in R.CODER_N:
        c = R.b2d_case(n, max_dis, eps)
        pts, box, out = dev(c.pts), dev(c.box), nan(n, 4)
        L.call("erd_bbox2distance", L.p(pts), L.p(box), n, -1.0 if max_dis is None else max_dis, eps, L.p(out), L.s())
        assert torch.equal(out.cpu(), R.b2d_oracle(c, F32)), (n, max_dis)


def test_rows_mul_and_loss_coef_equal(L):
    for n in R.SMALL_N:
        for weighted in (False, True):
            c = R.small_case(n, weighted)
            rows, w, up = dev(c.rows), dev(c.weight), dev(c.upstream)
            out, coef = nan(n), nan(n)
            L.call("erd_rows_mul", L.p(rows), L.p(w), n, c.scale, L.p(out), L.s())
            L.call("erd_loss_coef", L.p(up), L.p(w), n, c.scale, L.p(coef), L.s())
            assert torch.equal(out.cpu(), R.rows_mul_restate(c)) and torch.equal(coef.cpu(), R.loss_coef_restate(c)), (n, weighted)


def test_atss_result_equal(L):
    for A in R.ATSS_A:
        c = R.atss_case(A)
        keys, gl = dev(c.keys), dev(c.gt_labels)
        gi, ov, lb = nan(A, dtype=torch.int64), nan(A), nan(A, dtype=torch.int64)
        L.call("erd_atss_result", L.p(keys), L.p(gl), A, L.p(gi), L.p(ov), L.p(lb), L.s())
        assert torch.equal(gi.cpu(), c.gt_inds) and torch.equal(ov.cpu(), c.max_ov) and torch.equal(lb.cpu(), c.labels), A


def _wsum(L, c):
    import ctypes as C
    rows, w, out = dev(c.rows), dev(c.weight), nan(1)
    L.call("erd_weighted_sum", L.p(rows), L.p(w), c.n, C.c_double(c.scale), L.p(out), L.s())
    return float(out.cpu())


def test_weighted_sum_exact(L):
    for n in R.WSUM_N:
        for weighted in (False, True):
            c = R.wsum_case(n, weighted)
            assert _wsum(L, c) == c.want, (n, weighted)
    c = R.wsum_real_case()              # the f64 sum in another order, rounded to fp32 once: half an ulp (and 2^-40 for the order)
    assert abs(_wsum(L, c) - c.want) <= (2.0 ** -24 + 2.0 ** -40) * abs(c.want)


# ---- zero rows and null pointers at the C ABI ---------------------------------------------------------------------------
def _null_calls(L, n, buf):
    """every entry point that checks its pointers, with null for all of them (n == 0) or for the first input only (n > 0)"""
    z, b, s = L.p(None), (L.p(None) if n == 0 else L.p(buf)), L.s()
    return {
        "erd_qfl_rows": lambda: L.call("erd_qfl_rows", z, b, b, n, 80, b, s),
        "erd_qfl_bwd": lambda: L.call("erd_qfl_bwd", z, b, b, b, n, 80, b, s),
        "erd_dfl": lambda: L.call("erd_dfl", z, b, b, n, 17, b, b, s),
        "erd_kd_kl_rows": lambda: L.call("erd_kd_kl_rows", z, b, b, n, 17, 10.0, b, b, s),
        "erd_integral": lambda: L.call("erd_integral", z, b, n, 17, b, b, s),
        "erd_giou": lambda: L.call("erd_giou", z, b, b, n, 1e-6, b, b, s),
        "erd_distance2bbox": lambda: L.call("erd_distance2bbox", z, b, b, n, -1.0, -1.0, b, b, s),
        "erd_bbox2distance": lambda: L.call("erd_bbox2distance", z, b, n, 16.0, 0.1, b, s),
        "erd_bbox_overlaps": lambda: L.call("erd_bbox_overlaps", z, b, n, n, 1, 0, 1e-6, b, s),
        "erd_rows_mul": lambda: L.call("erd_rows_mul", z, b, n, 1.0, b, s),
    }


def test_null_pointers_are_legal_exactly_when_there_is_nothing_to_do(L):
    buf = nan(8 * 80)
    for name, f in _null_calls(L, 0, buf).items():
        f()                                              # raises on a non-zero return
    for name, f in _null_calls(L, 8, buf).items():       # refused before any launch
        with pytest.raises(L.Err, match="bad args"):
            f()
    with pytest.raises(L.Err, match="bad args"):         # neither output pointer
        L.call("erd_dfl", L.p(buf), L.p(buf), L.p(None), 8, 17, L.p(None), L.p(None), L.s())
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())


# ---- through erd_amd/leaf.py and the registered modules ---------------------------------------------------------------
ULP = 2.0 ** -23
REDUCTIONS = [("none", None), ("none", 5.0), ("mean", None), ("mean", 5.0), ("sum", None)]


def _noncontiguous(t):
    """(storage, view): a leaf whose transposed view is the operator's input"""
    st = t.t().contiguous().cuda().requires_grad_(True)
    return st, st.t()


def _check_row_loss(op, c, forward, loss_weight, weight):
    """value and gradient (arriving at the original tensor of a transposed view) for all reductions, against the fp64 oracle
    reduced by the reference's rules.  Tolerances: the 4 x E32 share of each row's scale, plus two ulp for the fp32 roundings
    of the coefficient loss_weight * scale * weight (value) and four for coefficient times upstream (gradient)"""
    _, oracle, scales, _ = R.RULE_OPS[op]
    er, eg = R.e32(op)
    n = c.pred.shape[0]
    w64 = None if weight is None else weight.double()
    for red, af in REDUCTIONS:
        st, view = _noncontiguous(c.pred)
        assert not view.is_contiguous() or min(view.shape) == 1
        out = forward(view, dev(weight), af, red)
        f = R.reduce_scale(red, af, n, loss_weight)
        up = torch.randn(n, generator=torch.Generator().manual_seed(11)) if red == "none" else torch.ones(())
        cc = copy.copy(c)
        cc.coef = ((loss_weight if f is None else f) * up.double() * (1.0 if w64 is None else w64) * torch.ones(n, dtype=F64))
        rows64, grad64 = oracle(cc, F64)
        rs, gs = scales(cc)
        ref = R.reduce_ref(rows64, w64, red, af, loss_weight)
        wabs = torch.ones(n, dtype=F64) if w64 is None else w64.abs()
        if red == "none":
            assert out.shape == (n,)
            tol = (R.FACTOR * er + 2 * ULP) * rs * wabs * loss_weight
            assert bool(((out.detach().cpu().double() - ref).abs() <= tol).all()), (op, red, af)
            out.backward(dev(up))
        else:
            assert out.shape == ()
            tol = R.FACTOR * er * abs(f) * float((rs * wabs).sum()) + 2 * ULP * abs(float(ref))
            assert abs(float(out) - float(ref)) <= tol, (op, red, af, float(out), float(ref), tol)
            out.backward()
        got = R.nerr(st.grad.t().cpu(), grad64, gs)
        assert got <= R.FACTOR * eg + 4 * ULP, (op, red, af, got, eg)
    with pytest.raises(ValueError):
        forward(_noncontiguous(c.pred)[1], dev(weight), 5.0, "sum")
    with pytest.raises(TypeError):
        forward(dev(c.pred).double(), dev(weight), None, "mean")


def _weights(n, seed):
    w = torch.rand(n, generator=torch.Generator().manual_seed(seed))
    w[1::5] = 0.0
    return w


def test_quality_focal_loss_module(L):
    c = R.qfl_cases()[4]                 # (9, 80)
    m = L.MODELS.build(dict(type="QualityFocalLoss", use_sigmoid=True, beta=2.0, loss_weight=0.7))
    tgt = (dev(c.label), dev(c.score))
    for w in (None, _weights(c.n, 21)):
        _check_row_loss("qfl", c, lambda p, wt, af, red: m(p, tgt, weight=wt, avg_factor=af, reduction_override=red), 0.7, w)
    with pytest.raises(NotImplementedError):
        L.leaf.quality_focal_loss(dev(c.pred), tgt, beta=1.0)
    with pytest.raises(NotImplementedError):
        L.MODELS.build(dict(type="QualityFocalLoss", use_sigmoid=True, beta=1.0))


def test_distribution_focal_loss_module(L):
    c = R.dfl_cases()[2]                 # (257, 8)
    m = L.MODELS.build(dict(type="DistributionFocalLoss", loss_weight=0.25))
    tgt = dev(c.target)
    for w in (None, _weights(c.m, 22)):
        _check_row_loss("dfl", c, lambda p, wt, af, red: m(p, tgt, weight=wt, avg_factor=af, reduction_override=red), 0.25, w)


def test_kd_kl_div_loss_module(L):
    for c in (R.kd_cases()[4], R.kd_cases()[5]):          # (257, 8) at T = 1 and T = 10
        m = L.MODELS.build(dict(type="KnowledgeDistillationKLDivLoss", loss_weight=0.25, T=c.T))
        soft = dev(c.soft)
        _check_row_loss("kd", c, lambda p, wt, af, red: m(p, soft, weight=wt, avg_factor=af, reduction_override=red), 0.25,
                        _weights(c.m, 23))


def test_giou_loss_module_with_per_coordinate_weights(L):
    c = R.giou_cases()[2]                # the family at n = 257
    m = L.MODELS.build(dict(type="GIoULoss", loss_weight=2.0))
    tgt = dev(c.target)
    _check_row_loss("giou", c, lambda p, wt, af, red: m(p, tgt, weight=wt, avg_factor=af, reduction_override=red), 2.0, _weights(c.n, 24))
    # [n, 4] weights are averaged per box (iou_loss.py:511-515); quarters, so that the mean is exact
    w4 = torch.randint(0, 5, (c.n, 4), generator=torch.Generator().manual_seed(25)).float() / 4.0
    _check_row_loss("giou", c, lambda p, wt, af, red: m(p, tgt, weight=None if wt is None else dev(w4), avg_factor=af,
                                                        reduction_override=red), 2.0, w4.mean(-1))


def test_integral_module(L):
    from erd_amd.modules import Integral
    c = R.integral_cases()[1]            # (1028, 17) = [257, 4 x 17]
    er, eg = R.e32("integral")
    y64, g64 = R.integral_oracle(c, F64)
    rs, gs = R.integral_scales(c)
    st, view = _noncontiguous(c.x.reshape(257, 68))
    y = Integral(16).cuda()(view)
    assert y.shape == (257, 4)
    y.backward(dev(c.dy.reshape(257, 4)))
    assert R.nerr(y.detach().cpu().reshape(-1), y64, rs) <= R.FACTOR * er
    assert R.nerr(st.grad.t().cpu().reshape(1028, 17), g64, gs) <= R.FACTOR * eg
    with pytest.raises(TypeError):
        Integral(16).cuda()(dev(c.x.reshape(257, 68)).double())


def test_coder_and_overlaps_modules(L):
    coder = L.TASK_UTILS.build(dict(type="DistancePointBBoxCoder"))
    c = R.d2b_case(257)
    pts3 = dev(torch.cat([c.pts, torch.full((c.n, 1), 8.0)], 1))[:, :2]              # a strided view: [n, 3] points with their stride
    for ms in (None, R.MAX_SHAPE):
        box, grad = R.d2b_oracle(c, ms, F32)
        st, view = _noncontiguous(c.dist)
        out = coder.decode(pts3, view, max_shape=ms)
        out.backward(dev(c.dout))
        assert torch.equal(out.detach().cpu(), box) and torch.equal(st.grad.t().cpu(), grad), ms
    for max_dis, eps in R.B2D_PARAMS:
        b = R.b2d_case(257, max_dis, eps)
        assert torch.equal(coder.encode(dev(b.pts), dev(b.box), max_dis, eps).cpu(), R.b2d_oracle(b, F32)), max_dis
    ov = L.TASK_UTILS.build(dict(type="BboxOverlaps2D"))
    a, b = R.pair_boxes(17, 31)
    a5, b5 = dev(torch.cat([a, torch.rand(17, 1)], 1)), dev(torch.cat([b, torch.rand(31, 1)], 1))          # [n, 5]: a score column
    for mode in ("iou", "giou"):
        assert torch.equal(ov(a5, b5, mode).cpu(), R.overlaps_restate(a, b, mode, False))
        assert torch.equal(ov(a5, b5[:17], mode, True).cpu(), R.overlaps_restate(a, b[:17], mode, True))
    with pytest.raises(NotImplementedError):
        ov(a5[None], b5[None])                                                       # 3-D boxes
    with pytest.raises(TypeError):
        ov(a5.double(), b5.double())


# ---- zero rows through the modules ----------------------------------------------------------------------------------------
def _empty(*shape):
    return torch.empty(shape, device="cuda").requires_grad_(True)


@pytest.mark.parametrize("op", ["qfl", "dfl", "kd", "giou"])
def test_losses_over_zero_rows(L, op):
    width = {"qfl": 80, "dfl": 17, "kd": 17, "giou": 4}[op]
    cfg = {"qfl": dict(type="QualityFocalLoss", use_sigmoid=True, beta=2.0), "dfl": dict(type="DistributionFocalLoss"),
           "kd": dict(type="KnowledgeDistillationKLDivLoss", T=10), "giou": dict(type="GIoULoss")}[op]
    m = L.MODELS.build(cfg)
    tgt = {"qfl": (torch.empty(0, dtype=torch.int64, device="cuda"), torch.empty(0, device="cuda")),
           "dfl": torch.empty(0, device="cuda"), "kd": torch.empty(0, 17, device="cuda"), "giou": torch.empty(0, 4, device="cuda")}[op]
    for w in (None, torch.empty(0, device="cuda")):
        for red, af in (("none", None), ("sum", None), ("mean", 3.0)):
            p = _empty(0, width)
            out = m(p, tgt, weight=w, avg_factor=af, reduction_override=red)
            if red == "none":
                assert out.shape == (0,)
                out.backward(torch.empty(0, device="cuda"))
            else:
                assert out.shape == () and float(out) == 0.0
                out.backward()
            assert p.grad is not None and p.grad.shape == (0, width)


def test_integral_coder_and_overlaps_over_zero_rows(L):
    from erd_amd.modules import Integral
    x = _empty(0, 68)
    y = Integral(16).cuda()(x)
    assert y.shape == (0, 4)
    y.backward(torch.empty(0, 4, device="cuda"))
    assert x.grad.shape == (0, 68)
    coder = L.TASK_UTILS.build(dict(type="DistancePointBBoxCoder"))
    pts = torch.rand(5, 2, device="cuda")
    for ms in (None, R.MAX_SHAPE):
        d = _empty(0, 4)
        box = coder.decode(pts[:0], d, max_shape=ms)
        assert box.shape == (0, 4)
        box.backward(torch.empty(0, 4, device="cuda"))
        assert d.grad.shape == (0, 4)
    assert coder.encode(pts[:0], torch.empty(0, 4, device="cuda"), 16, 0.1).shape == (0, 4)
    ov = L.TASK_UTILS.build(dict(type="BboxOverlaps2D"))
    b = torch.rand(8, 4, device="cuda")
    assert ov(b[:0], b).shape == (0, 8) and ov(b, b[:0]).shape == (8, 0) and ov(b[:0], b[:0], "giou", True).shape == (0,)
