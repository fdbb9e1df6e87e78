"""GPU: the fused training-loss kernels of erd_amd/csrc/losses.hip row by row at their edges, through the C ABI and through
functional.ERDLossFn.  Reference, row scales, restatement, case tables and the rule are tests/loss_refs.py (proved on the CPU by
tests/test_loss_refs_cpu.py); tests/test_gpu_losses.py stays the tie to the real reference's fixture.

  * every case runs the chain of a training step on GIVEN targets: erd_gfl_losses_fwd, erd_loss_avg, erd_l2_distill, erd_kd_kl,
    erd_loss_finalize (losses), erd_loss_finalize (coefficients under `up`), erd_gfl_losses_bwd, erd_l2_distill_bwd, erd_kd_kl_bwd
  * score_ws, wt_ws and every row of dcls and dbbox read at most 4 x E32 of their kind (E32: the fp32 composition of the oracle on
    the CPU against the fp64 one, computed here from the reference alone); a level or image sum at most 4 x E32 x the sum of its
    rows' scales.  E32, the kernel's figure and the ratio are printed.
  * bit-equal to the restatement: erd_loss_avg, erd_loss_finalize, the old-channel zeros of dcls, the zero dbbox rows and
    score == wt == 0 of non-positives; bit-equal to their fill: what the two distillation backward kernels do not own
  * every output starts filled with NaN (-7777 for integers, 0xFF for masks); every forward entry point is called twice into the
    same sum buffer"""
import ctypes as C
from types import SimpleNamespace as NS

import pytest
import torch

pytestmark = pytest.mark.gpu

import loss_refs as LR
from oracle import erd_oracle as O

F32, F64 = LR.F32, LR.F64
NAN = float("nan")
HALF_ULP = 2.0 ** -24


@pytest.fixture(scope="module")
def L():
    from erd_amd import _lib, functional
    from erd_amd import kernels as K
    _lib.load()
    return NS(call=_lib.call, p=K._p, s=K._stream, Err=_lib.ErdHipError, K=K, functional=functional)


def nan(*shape, dtype=F32):
    if dtype in (torch.int64, torch.int32):
        return torch.full(shape, -7777, dtype=dtype, device="cuda")
    if dtype == torch.uint8:
        return torch.full(shape, 0xFF, dtype=dtype, device="cuda")
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


def dev(t):
    return None if t is None else t.contiguous().cuda()


def shifted(t, k):
    """a contiguous device copy of t whose first element lies k floats past a 16-byte boundary (a view into a larger buffer)"""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[k:k + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * k
    return v


def _iarr(vals, ct):
    return (ct * len(vals))(*[int(v) for v in vals])


def _report(op, what, e, got):
    print(f"\n[loss] {op:22s} {what:9s} E32 {e:.3e}  kernel {got:.3e}  ratio {got / e if e else float('inf'):.2f}")


def _same_sums(a, b):
    """two runs of f64 atomic adds agree to the reassociation of f64 (2^-40 of the value is ample); a buffer that was not zeroed
    would read twice the value"""
    return bool(((a - b).abs() <= 2.0 ** -40 * a.abs()).all())


def run_chain(L, c):
    """the step's chain on case c through the C ABI; every output NaN-filled before its call"""
    N, A, nl, c_old, c_all = c.N, c.A, c.nlvl, c.c_old, c.c_all
    p, s = L.p, L.s
    cls, bbox = shifted(c.cls, c.cls_shift), dev(c.bbox)
    anchors, labels, lw, bt = dev(c.anchors), dev(c.labels), dev(c.lw), dev(c.bt)
    off, strides = _iarr(LR.lvl_off(c.sizes), C.c_int64), _iarr(c.strides, C.c_int)
    lw_cls, lw_bbox, lw_dfl, lw_ld, w_dist = c.weights
    g = NS()
    score, wt, sums = nan(N, A), nan(N, A), nan(nl, 4, dtype=F64)
    fwd = lambda: L.call("erd_gfl_losses_fwd", p(cls), p(bbox), p(anchors), p(labels), p(lw), p(bt), off, strides, nl, N, A, c_old, c_all,
                         p(score), p(wt), p(sums), s())
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
        for name, buf, call in (("l2", l2s, lambda: L.call("erd_l2_distill", p(cls), p(t_cls), p(idx), p(counts), N, A, c_all, c.c_t, c_old, p(l2s), s())),
                                ("kd", kds, lambda: L.call("erd_kd_kl", p(bbox), p(t_bbox), p(cls), p(keep), N, A, c_all, c_old, c.T, p(kds), s()))):
            call()
            first = buf.clone()
            call()
            assert _same_sums(first, buf), (c.name, name)
    losses, coef = nan(3 * nl + 2 * nd), nan(4 * nl + 2 * nd)
    up = dev(c.up)
    fin = lambda upv, lo, co: L.call("erd_loss_finalize", p(sums), p(avg), p(l2s), p(kds), p(counts), nl, nd, c_old, w_dist, lw_cls, lw_bbox, lw_dfl,
                                     lw_ld, p(upv), p(lo), p(co), s())
    fin(None, losses, None)                     # losses only, as the forward of ERDLossFn
    fin(up, None, coef)                         # coefficients only, as its backward
    dcls_buf = shifted(torch.full(c.cls.shape, NAN), c.cls_shift)
    dbbox = nan(N, A, 68)
    bwd = lambda dc, db: L.call("erd_gfl_losses_bwd", p(cls), p(bbox), p(anchors), p(labels), p(lw), p(bt), off, strides, nl, N, A, c_old, c_all,
                                p(score), p(wt), p(coef), p(dc), p(db), s())
    bwd(dcls_buf, dbbox)
    assert bool((dcls_buf[:, :, :c_old] == 0).all()), c.name            # the old channels: zeros, before the distillation adds
    if c.cls_shift:                                                     # the write-back into a buffer of another alignment: the same bits
        d2, b2 = nan(N, A, c_all), nan(N, A, 68)
        bwd(d2, b2)
        assert torch.equal(d2, dcls_buf) and torch.equal(b2, dbbox)
    g.dcls_gfl, g.dbbox_gfl = dcls_buf.cpu().clone(), dbbox.cpu().clone()
    if c.distill:
        L.call("erd_l2_distill_bwd", p(cls), p(t_cls), p(idx), p(counts), p(coef[4 * nl:]), N, A, c_all, c.c_t, c_old, p(dcls_buf), s())
        L.call("erd_kd_kl_bwd", p(bbox), p(t_bbox), p(cls), p(keep), p(coef[4 * nl + N:]), N, A, c_all, c_old, c.T, p(dbbox), s())
        # the same two calls into a known pattern: what they do not own keeps it bit for bit
        pat_c = dev(0.5 + 0.25 * (torch.arange(c.cls.numel()) % 5).float().reshape(c.cls.shape))
        pat_b = dev(-1.0 + 0.5 * (torch.arange(c.bbox.numel()) % 3).float().reshape(c.bbox.shape))
        oc, ob = pat_c.clone(), pat_b.clone()
        L.call("erd_l2_distill_bwd", p(cls), p(t_cls), p(idx), p(counts), p(coef[4 * nl:]), N, A, c_all, c.c_t, c_old, p(oc), s())
        L.call("erd_kd_kl_bwd", p(bbox), p(t_bbox), p(cls), p(keep), p(coef[4 * nl + N:]), N, A, c_all, c_old, c.T, p(ob), s())
        g.pat_c, g.pat_b, g.out_c, g.out_b = pat_c.cpu(), pat_b.cpu(), oc.cpu(), ob.cpu()
    torch.cuda.synchronize()
    for k, v in (("score", score), ("wt", wt), ("sums", sums), ("avg", avg), ("losses", losses), ("coef", coef), ("dcls", dcls_buf), ("dbbox", dbbox),
                 ("l2s", l2s), ("kds", kds)):
        setattr(g, k, None if v is None else v.cpu().clone())
    return g


def _pattern_check(c, i, g, E):
    """rows outside idx, rows outside keep and the new channels of dcls keep the pattern; the touched entries are pattern + addend:
    the addend under the rule, plus the half ulp of the one rounding of the stored sum"""
    r = LR.ref64(i)
    N, A, c_old = c.N, c.A, c.c_old
    sel = torch.zeros(N, A, dtype=torch.bool)
    for n in range(N):
        sel[n, c.idx_cls[n, :int(c.counts[n, 0])]] = True
    kept = c.keep != 0
    assert torch.equal(g.out_c[:, :, c_old:], g.pat_c[:, :, c_old:]), c.name
    assert torch.equal(g.out_c[:, :, :c_old][~sel], g.pat_c[:, :, :c_old][~sel]), c.name
    assert torch.equal(g.out_b[~kept], g.pat_b[~kept]), c.name
    same = kept & (c.t_bbox == c.bbox).all(2)                          # student == teacher: the addend is exactly 0
    assert torch.equal(g.out_b[same], g.pat_b[same]), c.name
    add_c = r.dcls[:, :, :c_old]                                      # (gfl_bwd leaves the old channels 0: the reference's gradient there is the L2 addend)
    want = g.pat_c[:, :, :c_old].double() + add_c
    tol = LR.FACTOR * E["dcls_old"] * r.scale.dcls_old[..., None] + HALF_ULP * want.abs()
    assert bool(((g.out_c[:, :, :c_old].double() - want).abs() <= tol)[sel].all()), c.name
    add_b = (r.dbbox - g.dbbox_gfl.double()).reshape(N, A, 4, 17)     # the KD addend: the reference's total less what gfl_bwd wrote (held to the rule itself)
    want = g.pat_b.double().reshape(N, A, 4, 17) + add_b
    tol = LR.FACTOR * E["dbbox"] * (r.scale.dbbox + r.scale.dbbox_kd)[..., None] + HALF_ULP * want.abs()
    assert bool(((g.out_b.double().reshape(N, A, 4, 17) - want).abs() <= tol)[kept].all()), c.name


ENTRY = {"score": "erd_gfl_losses_fwd", "wt": "erd_gfl_losses_fwd", "qfl": "erd_gfl_losses_fwd", "giou": "erd_gfl_losses_fwd",
         "dfl": "erd_gfl_losses_fwd", "wt_sum": "erd_gfl_losses_fwd", "dcls_new": "erd_gfl_losses_bwd", "dbbox": "erd_gfl_losses_bwd+kd_kl_bwd",
         "l2": "erd_l2_distill", "dcls_old": "erd_l2_distill_bwd", "kd": "erd_kd_kl"}


def test_the_chain_of_a_step_row_by_row(L):
    E = LR.e32()
    worst, bad = {}, []
    for i, c in enumerate(LR.cases()):
        g = run_chain(L, c)
        for k, v in LR.figures(c, i, g).items():
            worst[k] = max(worst.get(k, 0.0), v)
        bad += [(c.name,) + v for v in LR.violations(c, i, g, E)]
        if c.distill:
            _pattern_check(c, i, g, E)
        # one fp32 run against the restatement: the parts that are add / multiply / divide only (also inside violations)
        assert LR.exact_violations(c, g) == [], c.name
    for k in sorted(worst, key=lambda k: ENTRY[k]):
        _report(ENTRY[k], k, E[k], worst[k])
    assert bad == []


def test_loss_avg_and_finalize_alone_bit_equal(L):
    p, s = L.p, L.s
    for f in LR.finalize_cases():
        nl, N = f.nlvl, f.N
        sums, npos = dev(f.sums), dev(f.num_pos)
        avg = nan(2)
        L.call("erd_loss_avg", p(npos), N, p(sums), nl, p(avg), s())
        want_avg = LR.avg_restate(f.num_pos[:N], f.sums)
        assert torch.equal(avg.cpu(), want_avg), f.name
        l2s, kds, cnt = (dev(f.l2s), dev(f.kds), dev(f.counts)) if N else (None, None, None)
        up = dev(f.up)
        for upv, want_l, want_c in ((None, True, False), (up, False, True), (up, True, True), (None, True, True)):
            lo, co = nan(3 * nl + 2 * N), nan(4 * nl + 2 * N)
            L.call("erd_loss_finalize", p(sums), p(avg), p(l2s), p(kds), p(cnt), nl, N, f.c_old, f.weights[4], f.weights[0], f.weights[1],
                   f.weights[2], f.weights[3], p(upv), p(lo if want_l else None), p(co if want_c else None), s())
            rl, rc = LR.finalize_restate(f.sums, want_avg, f.l2s, f.kds, f.counts, nl, N, f.c_old, f.weights, None if upv is None else f.up)
            assert torch.equal(lo.cpu(), rl) if want_l else bool(torch.isnan(lo).all()), f.name
            assert torch.equal(co.cpu(), rc) if want_c else bool(torch.isnan(co).all()), f.name


def test_autograd_path_with_three_levels(L):
    """functional.ERDLossFn with a hand-built `t`: L = 3, N = 2, distillation on, a non-uniform upstream: the coefficient slots of
    the distillation terms start at 4 * L = 12"""
    names = [c.name for c in LR.cases()]
    i = names.index("pyr3")
    c = LR.cases()[i]
    assert c.nlvl == 3 and c.N == 2 and c.distill and len(set(c.up.tolist())) == len(c.up)
    s_cls, s_bbox = dev(c.cls).requires_grad_(True), dev(c.bbox).requires_grad_(True)
    t = NS(sizes=c.sizes, strides=c.strides, anchors=dev(c.anchors), labels=dev(c.labels), label_weights=dev(c.lw), bbox_targets=dev(c.bt),
           c_old=c.c_old, num_pos=dev(c.num_pos), world_size=1, distill=True, t_cls=dev(c.t_cls), t_bbox=dev(c.t_bbox),
           ers=dict(idx_cls=dev(c.idx_cls), counts=dev(c.counts)), keep=dev(c.keep), T=c.T, dist_loss_weight=c.weights[4], lw_cls=c.weights[0],
           lw_bbox=c.weights[1], lw_dfl=c.weights[2], lw_ld=c.weights[3])
    losses = L.functional.ERDLossFn.apply(s_cls, s_bbox, t)
    losses.backward(gradient=dev(c.up))
    g = run_chain(L, c)
    assert torch.equal(losses.detach().cpu(), g.losses)
    got = NS(score=g.score, wt=g.wt, sums=g.sums, avg=g.avg, losses=g.losses, coef=g.coef, l2s=g.l2s, kds=g.kds, dcls=s_cls.grad.cpu(),
             dbbox=s_bbox.grad.cpu())
    E = LR.e32()
    f = LR.figures(c, i, got)
    for k in ("dcls_new", "dcls_old", "dbbox"):
        _report("ERDLossFn", k, E[k], f[k])
    assert LR.violations(c, i, got, E) == []


# ---- refusals: what ERD_REQUIRE rejects before any launch ------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(L):
    p, s, z = L.p, L.s, L.p(None)
    f, d, i64, i32, u8 = nan(4 * 68), nan(8, dtype=F64), nan(8, dtype=torch.int64), nan(8, dtype=torch.int32), nan(8, dtype=torch.uint8)
    b, dd, il, ii, m = p(f), p(d), p(i64), p(i32), p(u8)
    off, strides = _iarr([0, 1], C.c_int64), _iarr([8], C.c_int)
    off6, strides6 = _iarr(range(7), C.c_int64), _iarr([8] * 6, C.c_int)
    calls = [
        lambda: L.call("erd_gfl_losses_fwd", z, b, b, il, b, b, off, strides, 1, 1, 1, 0, 4, b, b, dd, s()),
        lambda: L.call("erd_gfl_losses_bwd", z, b, b, il, b, b, off, strides, 1, 1, 1, 0, 4, b, b, b, b, b, s()),
        lambda: L.call("erd_gfl_losses_fwd", b, b, b, il, b, b, off, strides, 1, 1, 1, 4, 4, b, b, dd, s()),          # c_old >= c_all
        lambda: L.call("erd_gfl_losses_bwd", b, b, b, il, b, b, off, strides, 1, 1, 1, 5, 4, b, b, b, b, b, s()),
        lambda: L.call("erd_gfl_losses_fwd", b, b, b, il, b, b, off6, strides6, 6, 1, 6, 0, 4, b, b, dd, s()),        # nlvl == 6
        lambda: L.call("erd_gfl_losses_bwd", b, b, b, il, b, b, off6, strides6, 6, 1, 6, 0, 4, b, b, b, b, b, s()),
        lambda: L.call("erd_l2_distill", z, b, il, ii, 1, 1, 4, 4, 2, dd, s()),
        lambda: L.call("erd_l2_distill_bwd", z, b, il, ii, b, 1, 1, 4, 4, 2, b, s()),
        lambda: L.call("erd_kd_kl", z, b, b, m, 1, 1, 4, 2, 10.0, dd, s()),
        lambda: L.call("erd_kd_kl_bwd", z, b, b, m, b, 1, 1, 4, 2, 10.0, b, s()),
        lambda: L.call("erd_loss_avg", z, 1, dd, 1, b, s()),
        lambda: L.call("erd_loss_finalize", z, b, dd, dd, ii, 1, 1, 2, 1.0, 1.0, 2.0, 0.25, 0.25, z, b, b, s()),
        lambda: L.call("erd_loss_finalize", dd, b, dd, dd, ii, 1, 1, 2, 1.0, 1.0, 2.0, 0.25, 0.25, z, z, z, s()),      # neither output
        lambda: L.call("erd_ers_select", z, b, 1, 1, 4, 68, m, m, il, il, ii, b, dd, s()),
        lambda: L.call("erd_atss_assign", z, z, off, 1, 1, b, il, ii, 1, 1, 9, 80, il, b, b, ii, dd, s()),
        lambda: L.call("erd_distill_nms", z, b, b, il, ii, 1, 2, 4, 0.005, m, ii, b, C.c_size_t(64), s()),
        lambda: L.call("erd_distill_nms", b, b, b, il, ii, 1, 2, 4, 0.005, m, ii, b, C.c_size_t(2 * 32 - 1), s()),     # one byte short
    ]
    for k, call in enumerate(calls):
        with pytest.raises(L.Err):
            call()
    torch.cuda.synchronize()
    assert bool(torch.isnan(f).all()) and bool(torch.isnan(d).all()) and bool((i64 == -7777).all()) and bool((i32 == -7777).all()) \
        and bool((u8 == 0xFF).all())


# ---- the decision kernels against the oracle ----------------------------------------------------------------------------------
def test_ers_select_against_the_oracle(L):
    p, s = L.p, L.s
    for c in LR.ers_cases():
        N, A, Cc = c.cls.shape
        cls, bbox = dev(c.cls), dev(c.bbox)
        mc, mb = nan(N, A, dtype=torch.uint8), nan(N, A, dtype=torch.uint8)
        ic, ib = nan(N, A, dtype=torch.int64), nan(N, A, dtype=torch.int64)
        cnt, thr = nan(N, 2, dtype=torch.int32), nan(N, 2)
        ws = nan(N * 4 + N * A + 1, dtype=F64)
        L.call("erd_ers_select", p(cls), p(bbox), N, A, Cc, 68, p(mc), p(mb), p(ic), p(ib), p(cnt), p(thr), p(ws), s())
        for n in range(N):
            oc, ob, _, _ = O.ers_select_single(c.cls[n], c.bbox[n])
            for o, idx, mask, col in ((oc, ic, mc, 0), (ob, ib, mb, 1)):
                k = int(cnt[n, col])
                assert k == len(o) and torch.equal(idx[n, :k].cpu(), o) and bool((idx[n, k:] == -7777).all()), (c.name, n, col)
                want = torch.zeros(A, dtype=torch.uint8)
                want[o] = 1
                assert torch.equal(mask[n].cpu(), want), (c.name, n, col)


def test_distill_nms_against_the_oracle(L):
    p, s = L.p, L.s
    for c in LR.nms_cases():
        N, A, ct = c.t_cls.shape
        anchors = dev(torch.cat(O.grid_anchors(c.sizes, c.strides), 0))
        counts = torch.zeros(N, 2, dtype=torch.int32)
        counts[:, 1] = torch.tensor(c.K, dtype=torch.int32)
        keep, kcnt, ws = nan(N, A, dtype=torch.uint8), nan(N, dtype=torch.int32), nan(N * A * 8)
        t_cls, t_bbox, idx, cnt = dev(c.t_cls), dev(c.t_bbox), dev(c.idx), dev(counts)       # (named: a pointer outlives no temporary)
        assert int(idx.max()) < A and max(c.K) <= A
        L.call("erd_distill_nms", p(t_cls), p(t_bbox), p(anchors), p(idx), p(cnt), N, A, ct, 0.005, p(keep), p(kcnt), p(ws),
               C.c_size_t(N * A * 32), s())
        for n in range(N):
            want = LR.nms_oracle(c, n)
            assert keep[n].nonzero().squeeze(1).tolist() == want and int(kcnt[n]) == len(want), (c.name, n)
            assert bool((keep[n] <= 1).all())


def test_atss_assign_against_the_oracle(L):
    p, s = L.p, L.s
    for c in LR.atss_cases():
        anchors = torch.cat(O.grid_anchors(c.sizes, c.strides), 0)
        A, N = anchors.shape[0], len(c.boxes)
        goff = [0]
        for b in c.boxes:
            goff.append(goff[-1] + b.shape[0])
        labels, lw, bt, npos = nan(N, A, dtype=torch.int64), nan(N, A), nan(N, A, 4), nan(N, dtype=torch.int32)
        ws = nan(N * A, dtype=F64)
        an, gb, gl, go = dev(anchors), dev(torch.cat(c.boxes)), dev(torch.cat(c.labels)), dev(torch.tensor(goff, dtype=torch.int32))
        L.call("erd_atss_assign", p(an), p(None), _iarr(LR.lvl_off(c.sizes), C.c_int64), len(c.sizes), A, p(gb), p(gl), p(go), N,
               max(b.shape[0] for b in c.boxes), 9, c.num_classes, p(labels), p(lw), p(bt), p(npos), p(ws), s())
        for n in range(N):
            ol, ow, ob, on = LR.atss_oracle(c, n)
            assert torch.equal(labels[n].cpu(), ol) and torch.equal(lw[n].cpu(), ow) and torch.equal(bt[n].cpu(), ob) and int(npos[n]) == on, (c.name, n)
