"""References, restatement and case tables of the fused training-loss kernels (erd_amd/csrc/losses.hip: erd_gfl_losses_fwd / _bwd,
erd_l2_distill / _bwd, erd_kd_kl / _bwd, erd_loss_avg, erd_loss_finalize).  Imports no erd_amd: tests/test_loss_refs_cpu.py proves
on the CPU that the reference is right and that the rule bites, tests/test_gpu_loss_exact.py holds the kernels to it.

The inputs of the arithmetic kernels are the TARGETS (labels, label_weights, bbox_targets, idx_cls, counts, keep): the case tables
give them, the decision kernels (ERS, ATSS, NMS) do not produce them, so an arithmetic error can neither hide behind nor be blamed
on a flipped decision.

  compose(case, F64)  the fused head loss in float64 under autograd, from the oracle's pieces (oracle/erd_oracle.py, pinned to the
                      reference by tests/test_oracle_vs_reference.py) in the order of O.loss_by_feat_single / O.distill_loss_single /
                      O.erd_head_loss.  The whole functions return reduced losses only; the rows are needed, so the pieces are
                      composed, and tests/test_loss_refs_cpu.py asserts that the composition equals the whole functions.
                      weight_targets, the IoU score and both averaging factors are detached, as in the reference.
  compose(case, F32)  the yardstick: the same on the CPU in float32
  restate(case, mut)  the kernels' expressions in the kernels' operation order in fp32 torch ops (4 lanes per row over channels q,
                      q + 4, ..., then the two xor shuffles; softmax17 with the reciprocal multiply; stride-unit decode; the (float)
                      casts of the f64 sums in finalize_kernel), with one switch per planted mistake (MUTATIONS).  The GIoU gradient
                      and the KD-KL row are leaf_refs.giou_restate / kd_restate: the same formulas, imported, not copied.

Row scales (leaf_refs' magnitudes, imported; an error is divided by its own row's scale, never by a tensor's maximum):
  wt          sigma(max logit): the logit is an exact input, the value has relative precision
  score       iou + sum_q |d iou / d pred_q| (|centre_q| + integral scale_q): the decoded box carries the rounding of the centre and
              of the expectation, and the IoU passes it on with its derivative
  QFL row     leaf qfl row scale, plus for a positive row (|x| d^2 + 2 |BCE| d) score_scale: the score is computed, not given; plus
              2 (1 - t) |min(x, 0)| d^2 per class: the reference's binary_cross_entropy_with_logits adds (1 - t) x and max(-x, 0), two
              terms of magnitude |x| that cancel at x < 0 (at x = -8 its fp32 value of 3.4e-4 carries an error of 1e-6: without the
              term one-channel rows set E32 of the QFL rows and of dcls to 9e-4 and 6e-4 for every row of the table)
  GIoU row    leaf scale 3 plus sum_q |d giou / d pred_q| (|centre_q| + integral scale_q)
  DFL row     leaf dfl row scale per box side, summed over the four sides of an anchor
  dcls row    new channels: |coef_l label_weight| leaf qfl gradient scale (plus the score term of the label's class);
              old channels: |coef_n| 2 max_k (|s_k| + |t_k|)
  dbbox row   (one box side) adds a GIoU-through-Integral term and a DFL term: |coef wt| (giou gradient magnitude) (integral gradient
              magnitude) + leaf dfl gradient scale; a KD-KL addend: leaf kd gradient scale with coef_n wt
  a sum       the sum of its rows' scales (the kernels add fp32 rows in f64: the triangle inequality)

The rule is leaf_refs' own: FACTOR = 4 times E32, the worst row-normalised error of the yardstick against compose(F64) over the
table, per kind of output (for a kind the kernels give out as sums: of the rows behind the sums).  erd_loss_avg and
erd_loss_finalize (add, multiply, IEEE divide), the zeros of dcls' old channels and of non-positive rows are bit-equal to the
restatement."""
import functools
from types import SimpleNamespace as NS

import torch

import leaf_refs as R
from leaf_refs import F32, F64, FACTOR, EPS32, nerr
from leaf_refs import qfl_scales, dfl_scales, kd_scales, _giou_scales, integral_scales
from oracle import erd_oracle as O

I64 = torch.int64
DEFAULT_W = (1.0, 2.0, 0.25, 0.25, 1.0)      # lw_cls, lw_bbox, lw_dfl, lw_ld, dist_loss_weight
GL_ROWS = 64

MUTATIONS = ["level_of_block", "distill_coef_at_20", "qfl_all_channels", "bg_not_remapped", "kd_weight_all_channels",
             "avg_no_clamp", "l2_denominator_no_c_old", "kc_zero_nan", "dfl_clamp_16", "tl_rounds", "ties_1_0",
             "old_channels_left", "T_not_T2", "lw_ignored"]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _leaf(t, dtype):
    return t.detach().to(dtype).clone().requires_grad_(True)


def lvl_off(sizes):
    off = [0]
    for h, w in sizes:
        off.append(off[-1] + h * w)
    return off


def level_of(sizes):
    """[A] level index of every anchor"""
    return torch.cat([torch.full((h * w,), l, dtype=I64) for l, (h, w) in enumerate(sizes)])


# ---------------------------------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------------------------------
DFL_MENU = (-1.5, 16.25, 3.0, 15.5, 0.0, 15.9, 7.3, 2.75)      # raw < 0, raw >= 15.9, integer, last bin, 0, the bound, plain


def make_case(name, sizes, strides, N, c_old, c_all, seed, pos=(), distill=None, T=10.0, weights=DEFAULT_W, up="ones",
              lw_zero=False, K=None, keep="random", cls_shift=0, sat=False):
    """a seeded case: N(-2, 2^2) class logits, N(0, 1.5^2) box logits, grid anchors; `pos` = [(image, anchor, label)], the target of
    the k-th positive is its anchor centre -/+ DFL_MENU distances (stride units, times the stride: exact), so the DFL targets run
    through every clamp; every other row is background (label c_all)"""
    g = _gen(seed)
    A = lvl_off(sizes)[-1]
    nlvl = len(sizes)
    cn = c_all - c_old
    cls = -2.0 + 2.0 * torch.randn(N, A, c_all, generator=g)
    bbox = 1.5 * torch.randn(N, A, 68, generator=g)
    anchors = torch.cat(O.grid_anchors(sizes, strides), 0)
    lv = level_of(sizes)
    labels = torch.full((N, A), c_all, dtype=I64)
    lw = torch.ones(N, A)
    bt = torch.zeros(N, A, 4)
    ctr = O.anchor_centers(anchors)
    for k, (n, a, lb) in enumerate(pos):
        s = float(strides[int(lv[a])])
        d = [DFL_MENU[(k + j * 3) % len(DFL_MENU)] for j in range(4)]
        if d[0] + d[2] <= 0:
            d[2] = 5.0
        if d[1] + d[3] <= 0:
            d[3] = 4.5
        labels[n, a] = lb
        bt[n, a] = torch.tensor([float(ctr[a, 0]) - d[0] * s, float(ctr[a, 1]) - d[1] * s, float(ctr[a, 0]) + d[2] * s, float(ctr[a, 1]) + d[3] * s])
    if lw_zero:
        bgr = (labels == c_all)
        lw[bgr & (torch.arange(A)[None, :] % 3 == 1)] = 0.0
    if sat:                     # leaf_refs._SAT in cls (the label's class of a positive row stays off -90: weight_targets of 8e-40 are below what fp32 holds), one-hot +-90 box rows
        for n in range(N):
            for a in range(A):
                cls[n, a, (a * 7 + n) % c_all] = R._SAT[(a + n) % 5]
                if 0 <= int(labels[n, a]) < cn:
                    cls[n, a, c_old + int(labels[n, a])] = R._SAT[(a + n) % 4]
                if a % 2 == 0:
                    for q in range(4):
                        bbox[n, a, q * 17:(q + 1) * 17] = -90.0
                        bbox[n, a, q * 17 + (0, 16, 5, 11)[(a // 2 + q) % 4]] = 90.0
    num_pos = torch.tensor([sum(1 for p in pos if p[0] == n) for n in range(N)], dtype=torch.int32)
    distill = (c_old > 0) if distill is None else distill
    c = NS(name=name, sizes=list(sizes), strides=list(strides), nlvl=nlvl, N=N, A=A, c_old=c_old, c_all=c_all, cls=cls, bbox=bbox,
           anchors=anchors, labels=labels, lw=lw, bt=bt, num_pos=num_pos, distill=distill, T=float(T), weights=tuple(weights),
           cls_shift=cls_shift)
    if distill:
        c.c_t = c_old
        c.t_cls = cls[:, :, :c.c_t] + 0.7 * torch.randn(N, A, c.c_t, generator=g)
        c.t_bbox = bbox + 1.0 * torch.randn(N, A, 68, generator=g)
        Ks = list(K) if K is not None else [int(torch.randint(1, A + 1, (1,), generator=g)) for _ in range(N)]
        c.idx_cls = torch.zeros(N, A, dtype=I64)
        c.counts = torch.zeros(N, 2, dtype=torch.int32)
        for n in range(N):
            sel = torch.sort(torch.randperm(A, generator=g)[:Ks[n]]).values
            c.idx_cls[n, :Ks[n]] = sel
            c.counts[n, 0] = Ks[n]
        if keep == "random":
            c.keep = (torch.rand(N, A, generator=g) < 0.4).to(torch.uint8)
        elif keep == "none":
            c.keep = torch.zeros(N, A, dtype=torch.uint8)
        elif keep == "all":
            c.keep = torch.ones(N, A, dtype=torch.uint8)
        elif keep == "last":                      # only the last anchor (of a ragged block of 64), and a different mask per image
            c.keep = torch.zeros(N, A, dtype=torch.uint8)
            c.keep[0, A - 1] = 1
            c.keep[1:, ::2] = 1
        c.counts[:, 1] = c.keep.sum(1).to(torch.int32)
    nl = 3 * nlvl + 2 * (N if distill else 0)
    if up == "ones":
        c.up = torch.ones(nl)
    elif up is None:
        c.up = None
    else:                                          # distinct values, one zero, one negative
        c.up = 0.5 + 0.25 * torch.arange(nl, dtype=F32)
        c.up[1 if nlvl > 1 else (3 if distill else 2)] = 0.0     # (a level's loss_cls; with one level loss_dist_cls or loss_dfl)
        c.up[(nl - 1)] = -1.5
    return c


def _corner_pos(sizes, N, cn, every=None):
    """positives on the first and last anchor of every level, the first and last row of every 64-row block, in every image but the
    one `every` leaves empty"""
    off = lvl_off(sizes)
    A = off[-1]
    rows = set()
    for l in range(len(sizes)):
        rows |= {off[l], off[l + 1] - 1}
    for b in range(0, A, GL_ROWS):
        rows |= {b, min(b + GL_ROWS, A) - 1}
    out = []
    for n in range(N):
        if every is not None and n == every:
            continue
        for k, a in enumerate(sorted(rows)):
            out.append((n, a, (k + n) % cn))
    return out


PYR5 = [(5, 7), (3, 4), (2, 2), (1, 1), (1, 1)]
CHANNELS = [(0, 1), (0, 3), (3, 4), (2, 5), (40, 80), (70, 80)]


def family_case():
    """leaf_refs.BOX_FAMILY mapped through the decode: the family's coordinates are multiples of 10; divided by 5 they are even
    integers in stride units, the centre of the prediction is an integer and its four distances are integers in [0, 16], which a
    box row with +90 on the two bins beside the distance and -90 elsewhere decodes exactly in fp32 AND fp64 (two probabilities of 1/2;
    exp(-180) vanishes beside 1 in both), and through which the GIoU gradient still passes (a one-hot row has p_j (j - d) == 0).  The anchor sits on that centre
    (stride 8), the target is the family's target times 8 / 5 in pixels.  So a tie is a tie in the kernel, the yardstick and the
    fp64 reference alike.  The two inverted predictions of the family (x2 < x1) are no decode of non-negative distances and are
    left out; every other member is here."""
    fam = [(p, t, w) for p, t, w in R.BOX_FAMILY if p[2] >= p[0] and p[3] >= p[1]]
    n = len(fam)
    c = make_case("family", [(1, n)], [8], 1, 2, 5, 900, pos=[(0, a, a % 3) for a in range(n)], up="distinct", K=[3], keep="random")
    for a, (p, t, _) in enumerate(fam):
        p5, t5 = [v / 5.0 for v in p], [v / 5.0 for v in t]
        cx, cy = (p5[0] + p5[2]) / 2.0, (p5[1] + p5[3]) / 2.0
        d = [cx - p5[0], cy - p5[1], p5[2] - cx, p5[3] - cy]
        assert all(float(v).is_integer() for v in d + [cx, cy]) and all(0 <= v <= 16 for v in d)
        c.anchors[a] = torch.tensor([cx * 8 - 32, cy * 8 - 32, cx * 8 + 32, cy * 8 + 32])
        c.bt[0, a] = torch.tensor(t5) * 8.0
        for q in range(4):              # two bins of +90 around the distance (probabilities of exactly 1/2 each), one bin for a distance of 0
            c.bbox[0, a, q * 17:(q + 1) * 17] = -90.0
            for b in ((int(d[q]) - 1, int(d[q]) + 1) if d[q] >= 1 else (0,)):
                c.bbox[0, a, q * 17 + b] = 90.0
    c.family = fam
    return c


def kd_edge_case(T):
    """keep = only the last anchor of a ragged block in image 0, every second anchor in image 1; a row with student == teacher; at
    T = 1 a teacher row with a logit gap above 104 (its other probabilities underflow: the `t > 0` branch)"""
    c = make_case(f"kd_edge_T{T}", [(1, 65)], [8], 2, 3, 4, 910 + int(T), pos=[(0, 64, 0), (1, 0, 0)], T=T, K=[1, 65], keep="last",
                  up="distinct")
    c.t_bbox[1, 2] = c.bbox[1, 2]
    c.t_bbox[0, 64, 0:17] = c.bbox[0, 64, 0:17]
    if T == 1:
        c.t_bbox[1, 4, 17:34] = 0.0
        c.t_bbox[1, 4, 20] = 120.0
        c.t_bbox[0, 64, 34:51] = -60.0
        c.t_bbox[0, 64, 50] = 60.0
    return c


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    k = 0
    for A in (1, 63, 64, 65, 130):                                  # geometry of gfl_losses_kernel x the channel pairs
        for N in (1, 3):
            c_old, c_all = CHANNELS[k % len(CHANNELS)]
            sizes = [(1, A)]
            out.append(make_case(f"A{A}N{N}c{c_old}_{c_all}", sizes, [8 << (k % 3)], N, c_old, c_all, 100 + k,
                                 pos=_corner_pos(sizes, N, c_all - c_old, every=1 if N == 3 else None), lw_zero=(k % 2 == 0),
                                 up=("distinct", "ones", None)[k % 3], T=(10.0, 1.0)[k % 2]))
            k += 1
    out.append(make_case("pyr5", PYR5, O.STRIDES, 2, 40, 80, 200, pos=_corner_pos(PYR5, 2, 40), up="distinct",
                         weights=(0.75, 1.5, 0.5, 0.125, 2.0), lw_zero=True))
    out.append(make_case("pyr3", PYR5[1:4], (16, 32, 64), 2, 2, 5, 201, pos=_corner_pos(PYR5[1:4], 2, 3, every=0), up="distinct", K=[0, 17]))
    out.append(make_case("pyr5_c0_1", PYR5, O.STRIDES, 1, 0, 1, 202, pos=_corner_pos(PYR5, 1, 1), up="distinct"))
    out.append(make_case("c1_5", [(1, 9)], [32], 2, 1, 5, 203, pos=[(0, 3, 3), (1, 8, 0)], K=[9, 1], keep="all", up="distinct", T=1.0))
    out.append(make_case("nopos_batch", [(1, 65)], [8], 2, 3, 4, 204, pos=[], lw_zero=True, up="distinct", K=[0, 0], keep="none"))
    out.append(make_case("one_pos", [(2, 3), (1, 2)], (8, 16), 2, 2, 5, 205, pos=[(1, 7, 1)], up="distinct"))     # avg[1] < 1
    out.append(make_case("one_row_per_level", PYR5[1:4], (16, 32, 64), 1, 2, 5, 206, pos=[(0, 0, 0), (0, 12, 1), (0, 16, 2)], up="distinct",
                         K=[1], keep="last"))
    out[-1].lw[out[-1].labels == 5] = 0.0                           # one active row per level: its QFL, GIoU and DFL rows are the sums
    out.append(make_case("sat", [(1, 66)], [16], 2, 0, 3, 207, pos=_corner_pos([(1, 66)], 2, 3), sat=True, up="distinct"))
    out.append(make_case("sat_c70_80", [(1, 21)], [8], 1, 70, 80, 208, pos=[(0, 0, 9), (0, 20, 0), (0, 7, 4)], sat=True, up="distinct"))
    out.append(make_case("shifted", [(1, 65)], [8], 2, 40, 80, 209, pos=_corner_pos([(1, 65)], 2, 40), cls_shift=1, up="distinct"))
    out.append(make_case("l2_two_passes", [(1, 240)], [8], 2, 70, 80, 210, pos=[(0, 0, 0), (1, 239, 9)], K=[240, 1], keep="all", up="distinct"))
    out.append(family_case())
    out.append(kd_edge_case(10))
    out.append(kd_edge_case(1))
    return out


def finalize_cases():
    """erd_loss_avg / erd_loss_finalize alone on given sums: nlvl in {1, 3, 5}, N in {0, 1, 3}, kc == 0 with non-zero upstream,
    avg[1] < 1, num_pos in {0, 1, 2} mixed, losses only / coefficients only / upstream null"""
    out = []
    g = _gen(300)
    for i, (nlvl, N) in enumerate([(1, 0), (3, 1), (5, 3), (3, 3), (1, 3), (5, 0)]):
        sums = torch.rand(nlvl, 4, generator=g, dtype=F64) * 3.0
        if i % 2 == 1:
            sums[:, 3] *= 0.05                                    # avg[1] < 1
        counts = torch.randint(1, 50, (max(N, 1), 2), generator=g).to(torch.int32)
        if N:
            counts[N - 1, 0] = 0                                  # kc == 0 with non-zero upstream
        nl = 3 * nlvl + 2 * N
        up = torch.randn(nl, generator=g)
        out.append(NS(name=f"fin_L{nlvl}N{N}", nlvl=nlvl, N=N, sums=sums, l2s=torch.rand(max(N, 1), generator=g, dtype=F64) * 40.0,
                      kds=torch.rand(max(N, 1), generator=g, dtype=F64), counts=counts, c_old=(1, 3, 40, 70)[i % 4],
                      num_pos=torch.tensor([(0, 1, 2)[(i + j) % 3] for j in range(max(N, 1))], dtype=torch.int32),
                      weights=DEFAULT_W if i % 2 else (0.75, 1.5, 0.5, 0.125, 2.0), up=up))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the composition of the oracle's pieces (ref64 at F64, the yardstick at F32)
# ---------------------------------------------------------------------------------------------------------------------
def _level_rows(anchors, cls_score, bbox_pred, labels, bbox_targets, stride, c_old, c_all, want_scales):
    """O.loss_by_feat_single, gfl_head_increment_erd.py:225-322, up to the rows (before the reductions)"""
    dtype = cls_score.dtype
    cls_new = cls_score[:, c_old:]
    bg = c_all - c_old
    labels = labels.clone()
    labels[labels == c_all] = bg
    n = labels.shape[0]
    pos = ((labels >= 0) & (labels < bg)).nonzero().squeeze(1)
    r = NS(pos=pos, labels=labels, score=torch.zeros(n, dtype=dtype), wt=torch.zeros(n, dtype=dtype), giou=torch.zeros(n, dtype=dtype),
           dfl=torch.zeros(n, dtype=dtype), dfl_sides=None)
    if len(pos) > 0:
        pbp = bbox_pred[pos]
        pc = O.anchor_centers(anchors[pos]) / stride
        r.wt = r.wt.index_put((pos,), cls_new.detach().sigmoid().max(dim=1)[0][pos])
        dec = O.distance2bbox(pc, O.integral(pbp))
        tgt = bbox_targets[pos] / stride
        r.score[pos] = O.bbox_overlaps(dec.detach(), tgt, is_aligned=True)
        r.tc = O.bbox2distance(pc, tgt, O.REG_MAX).reshape(-1)
        r.giou = r.giou.index_put((pos,), 1 - O.bbox_overlaps(dec, tgt, mode="giou", is_aligned=True, eps=1e-6))
        r.dfl_sides = O.distribution_focal_loss(pbp.reshape(-1, O.REG_MAX + 1), r.tc)
        r.dfl = r.dfl.index_put((pos,), r.dfl_sides.reshape(-1, 4).sum(1))
        r.dec, r.tgt, r.pbp = dec.detach(), tgt, pbp.detach()
        if want_scales:      # the decoded box's magnitude and what IoU / GIoU make of its rounding
            d = dec.detach().clone().requires_grad_(True)
            iou = O.bbox_overlaps(d, tgt, is_aligned=True)
            gi = torch.autograd.grad(iou.sum(), d)[0].abs()
            gg = torch.autograd.grad(O.bbox_overlaps(d, tgt, mode="giou", is_aligned=True, eps=1e-6).sum(), d)[0].abs()
            isc = integral_scales(NS(x=r.pbp.reshape(-1, 17), dy=torch.ones(4 * len(pos)), nb=17))
            pmag = pc.abs()[:, [0, 1, 0, 1]] + isc[0].reshape(-1, 4)
            r.score_scale = iou.detach() + (gi * pmag).sum(1)
            r.giou_scale = 3.0 + (gg * pmag).sum(1)
            r.int_gscale = isc[1].reshape(-1, 4)
    r.qfl = O.quality_focal_loss(cls_new, labels, r.score)
    return r


def compose(c, dtype, want_scales=False):
    """every value and gradient of the fused head loss in `dtype` under autograd"""
    N, A, L, c_old, c_all = c.N, c.A, c.nlvl, c.c_old, c.c_all
    lw_cls, lw_bbox, lw_dfl, lw_ld, w_dist = c.weights
    cls, bbox = _leaf(c.cls, dtype), _leaf(c.bbox, dtype)
    anchors = c.anchors.to(dtype)
    off = lvl_off(c.sizes)
    avg1 = float(sum(max(int(p), 1) for p in c.num_pos))
    lv = []
    for l in range(L):
        sl = slice(off[l], off[l + 1])
        a = anchors[sl][None].expand(N, -1, -1).reshape(-1, 4)
        lv.append(_level_rows(a, cls[:, sl].reshape(-1, c_all), bbox[:, sl].reshape(-1, 68), c.labels[:, sl].reshape(-1),
                              c.bt.to(dtype)[:, sl].reshape(-1, 4), c.strides[l], c_old, c_all, want_scales))
    lws = [c.lw.to(dtype)[:, off[l]:off[l + 1]].reshape(-1) for l in range(L)]
    wsum = sum(r.wt.sum() for r in lv)
    avg2 = max(float(wsum), 1.0)
    out = NS(lv=lv, avg=(avg1, float(wsum)))
    out.sums = torch.stack([torch.stack([(r.qfl * w).sum(), (r.giou * r.wt).sum(), (r.dfl * r.wt).sum(), r.wt.sum()]) for r, w in zip(lv, lws)]).detach()
    loss_cls = [lw_cls * O.weight_reduce(r.qfl, w, avg1) for r, w in zip(lv, lws)]
    loss_bbox = [lw_bbox * O.weight_reduce(r.giou, r.wt, 1.0) / avg2 for r in lv]
    loss_dfl = [lw_dfl * O.weight_reduce(r.dfl, r.wt, 4.0) / avg2 for r in lv]
    losses = loss_cls + loss_bbox + loss_dfl

    def full(get):          # per-level [N * n_l] rows back to [N, A]
        return torch.cat([get(r).detach().reshape(N, -1) for r in lv], 1)
    out.score, out.wt, out.qfl, out.giou, out.dfl = (full(lambda r, k=k: getattr(r, k)) for k in ("score", "wt", "qfl", "giou", "dfl"))
    if c.distill:
        t_cls, t_bbox = c.t_cls.to(dtype), c.t_bbox.to(dtype)
        dc, db = [], []
        out.l2_rows = torch.zeros(N, A, dtype=dtype)
        out.kd_rows = torch.zeros(N, A, 4, dtype=dtype)
        out.kd_wt = torch.zeros(N, A, dtype=dtype)
        l2s, kds = [], []
        for n in range(N):
            K = int(c.counts[n, 0])
            idx = c.idx_cls[n, :K]
            d2 = (cls[n, :, :c_old][idx] - t_cls[n, :, :c_old][idx]).pow(2)
            out.l2_rows[n, idx] = d2.sum(1).detach()
            l2s.append(d2.sum().detach())
            dc.append(w_dist * d2.mean() if K > 0 else w_dist * d2.sum())        # D10: an empty selection gives 0 (reference: NaN)
            kept = c.keep[n].nonzero().squeeze(1)
            wt = cls[n, :, :c_old][kept].detach().sigmoid().max(dim=1)[0] if len(kept) else torch.zeros(0, dtype=dtype)
            kd = O.kd_kl_div(bbox[n][kept].reshape(-1, 17), t_bbox[n][kept].reshape(-1, 17), c.T)
            out.kd_rows[n, kept] = kd.detach().reshape(-1, 4)
            out.kd_wt[n, kept] = wt
            wt4 = wt[:, None].expand(-1, 4).reshape(-1)
            kds.append((kd * wt4).sum().detach())
            db.append(w_dist * lw_ld * O.weight_reduce(kd, wt4, 4.0))
        losses = losses + dc + db
        out.l2s, out.kds = torch.stack(l2s), torch.stack(kds)
    out.losses = torch.stack(losses)
    up = torch.ones_like(out.losses) if c.up is None else c.up.to(dtype)
    (out.losses * up).sum().backward()
    out.losses = out.losses.detach()
    out.dcls = cls.grad if cls.grad is not None else torch.zeros_like(cls.detach())
    out.dbbox = bbox.grad if bbox.grad is not None else torch.zeros_like(bbox.detach())
    if want_scales:
        out.scale = _scales(c, out, up.double())
    return out


def _scales(c, r, up):
    """the row scales of the module's docstring, in fp64, from the fp64 composition `r`"""
    N, A, L, c_old, c_all = c.N, c.A, c.nlvl, c.c_old, c.c_all
    cn = c_all - c_old
    lw_cls, lw_bbox, lw_dfl, lw_ld, w_dist = c.weights
    off = lvl_off(c.sizes)
    a1, a2 = r.avg[0], max(r.avg[1], 1.0)
    s = NS(score=torch.zeros(N, A, dtype=F64), giou=torch.zeros(N, A, dtype=F64), dfl=torch.zeros(N, A, dtype=F64),
           qfl=torch.zeros(N, A, dtype=F64), dcls_new=torch.zeros(N, A, dtype=F64), dbbox=torch.zeros(N, A, 4, dtype=F64))
    s.wt = r.wt.clone()
    for l, lv in enumerate(r.lv):
        sl = slice(off[l], off[l + 1])
        n_l = off[l + 1] - off[l]
        cq = lw_cls / (a1 + EPS32) * float(up[l])
        cb = lw_bbox / (1.0 + EPS32) / a2 * float(up[L + l])
        cd = lw_dfl / (4.0 + EPS32) / a2 * float(up[2 * L + l])
        lwl = c.lw.double()[:, sl].reshape(-1)
        x = c.cls.double()[:, sl, c_old:].reshape(-1, cn)
        qr, qg = qfl_scales(NS(pred=x, label=lv.labels, score=lv.score, coef=cq * lwl, C=cn))
        # the reference's BCE adds (1 - t) x and max(-x, 0): at x < 0 two terms of magnitude |x| that cancel, which the leaf scale's
        # max(x, 0) + |x t| + log1p(exp(-|x|)) does not hold
        tq = torch.zeros_like(x)
        pq = ((lv.labels >= 0) & (lv.labels < cn)).nonzero().squeeze(1)
        tq[pq, lv.labels[pq]] = lv.score[pq]
        sq = torch.sigmoid(x)
        dq = (sq - tq).abs()
        extra = 2 * (1 - tq) * (-x).clamp(min=0)
        qr = qr + (extra * dq * dq).sum(1)
        qg = qg + (cq * lwl).abs() * (extra * 2 * dq * sq * (1 + sq)).max(1)[0]
        sc = torch.zeros(N * n_l, dtype=F64)
        gi = torch.zeros(N * n_l, dtype=F64)
        df = torch.zeros(N * n_l, dtype=F64)
        dbb = torch.zeros(N * n_l, 4, dtype=F64)
        if len(lv.pos):
            pos = lv.pos
            sc[pos] = lv.score_scale
            gi[pos] = lv.giou_scale
            wt = lv.wt[pos]
            # the score is computed: its scale enters the label's class of a positive row with the derivative of the QFL term
            xl = x[pos, lv.labels[pos]]
            sg = torch.sigmoid(xl)
            d = (lv.score[pos] - sg).abs()
            bce = xl.clamp(min=0) + (xl * lv.score[pos]).abs() + torch.log1p(torch.exp(-xl.abs()))
            qr[pos] = qr[pos] + (xl.abs() * d * d + 2 * bce * d) * lv.score_scale
            qg[pos] = qg[pos] + (cq * lwl[pos]).abs() * (3 * d * d + 2 * xl.abs() * d * sg * (1 + sg) + 2 * bce * sg * (1 + sg)) * lv.score_scale
            dr, dg = dfl_scales(NS(pred=lv.pbp.reshape(-1, 17), target=lv.tc, coef=cd * wt[:, None].expand(-1, 4).reshape(-1), nb=17))
            df[pos] = dr.reshape(-1, 4).sum(1)
            gmag = _giou_scales(NS(pred=lv.dec, target=lv.tgt, coef=cb * wt, eps=1e-6))[1]
            dbb[pos] = gmag[:, None] * lv.int_gscale + dg.reshape(-1, 4)
        for k, v in (("score", sc), ("giou", gi), ("dfl", df), ("qfl", qr), ("dcls_new", qg)):
            getattr(s, k)[:, sl] = v.reshape(N, n_l)
        s.dbbox[:, sl] = dbb.reshape(N, n_l, 4)
    # the per-level sums {qfl * lw, giou * wt, dfl * wt, wt}
    lvv = level_of(c.sizes)
    s.sums = torch.zeros(L, 4, dtype=F64)
    for l in range(L):
        m = lvv == l
        s.sums[l] = torch.stack([(s.qfl * c.lw.double().abs())[:, m].sum(), (s.giou * r.wt)[:, m].sum(), (s.dfl * r.wt)[:, m].sum(), r.wt[:, m].sum()])
    if c.distill:
        sa, ta = c.cls.double()[:, :, :c_old].abs(), c.t_cls.double()[:, :, :c_old].abs()
        sel = torch.zeros(N, A, dtype=torch.bool)
        for n in range(N):
            sel[n, c.idx_cls[n, :int(c.counts[n, 0])]] = True
        s.l2 = torch.where(sel, ((sa + ta) ** 2).sum(2), torch.zeros((), dtype=F64))
        kc = c.counts[:, 0].double()
        cl = torch.where(kc > 0, w_dist / (kc * c_old).clamp(min=1) * up[3 * L:3 * L + N], torch.zeros((), dtype=F64))
        ck = w_dist * lw_ld / (4.0 + EPS32) * up[3 * L + N:]
        s.dcls_old = torch.where(sel, cl.abs()[:, None] * 2 * (sa + ta).max(2)[0], torch.zeros((), dtype=F64))
        kr, kg = kd_scales(NS(pred=c.bbox.double().reshape(-1, 17), soft=c.t_bbox.double().reshape(-1, 17), T=c.T, nb=17,
                              coef=(ck[:, None] * r.kd_wt).reshape(-1, 1).expand(-1, 4).reshape(-1)))
        kept = (c.keep != 0)[:, :, None]
        s.kd = torch.where(kept, kr.reshape(N, A, 4), torch.zeros((), dtype=F64))
        s.dbbox_kd = torch.where(kept, kg.reshape(N, A, 4), torch.zeros((), dtype=F64))
        s.l2s = s.l2.sum(1)
        s.kds = (s.kd * r.kd_wt[:, :, None]).sum((1, 2))
    return s


@functools.lru_cache(maxsize=None)
def ref64(i):
    """compose(cases()[i], F64) with its row scales: computed once, shared, left unchanged"""
    return compose(cases()[i], F64, want_scales=True)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement of the kernels
# ---------------------------------------------------------------------------------------------------------------------
def _f(v):
    return torch.tensor(v, dtype=F32)


def avg_restate(num_pos, sums):
    """loss_avg_kernel"""
    t = sum(max(int(p), 1) for p in num_pos)
    w = torch.zeros((), dtype=F64)
    for l in range(sums.shape[0]):             # in level order, in f64; rounded to fp32 once
        w = w + sums[l, 3]
    return torch.stack([_f(float(t)), w.to(F32)])


def finalize_restate(sums, avg, l2s, kds, counts, nlvl, N, c_old, weights, up, mut=None):
    """finalize_kernel: (losses, coef) in its operations and their order; every operand is an fp32 scalar"""
    lw_cls, lw_bbox, lw_dfl, lw_ld, w_dist = (_f(v) for v in weights)
    eps, one, four = _f(EPS32), _f(1.0), _f(4.0)
    a1 = avg[0]
    a2 = avg[1] if mut == "avg_no_clamp" else torch.maximum(avg[1], one)
    u = (lambda i: one) if up is None else (lambda i: up[i].to(F32))
    losses, coef = torch.zeros(3 * nlvl + 2 * N), torch.zeros(4 * nlvl + 2 * N)
    for l in range(nlvl):
        q, b, d = (sums[l, j].to(F32) for j in range(3))
        losses[l] = lw_cls * (q / (a1 + eps))
        losses[nlvl + l] = lw_bbox * (b / (one + eps)) / a2
        losses[2 * nlvl + l] = lw_dfl * (d / (four + eps)) / a2
        coef[4 * l + 0] = lw_cls / (a1 + eps) * u(l)
        coef[4 * l + 1] = lw_bbox / (one + eps) / a2 * u(nlvl + l)
        coef[4 * l + 2] = lw_dfl / (four + eps) / a2 * u(2 * nlvl + l)
    for n in range(N):
        kc = int(counts[n, 0])
        denom = _f(float(kc)) if mut == "l2_denominator_no_c_old" else _f(float(kc)) * _f(float(c_old))
        live = kc > 0 or mut == "kc_zero_nan"
        losses[3 * nlvl + n] = w_dist * (l2s[n].to(F32) / denom if live else _f(0.0))
        losses[3 * nlvl + N + n] = w_dist * (lw_ld * (kds[n].to(F32) / (four + eps)))
        coef[4 * nlvl + n] = w_dist / denom * u(3 * nlvl + n) if live else _f(0.0)
        coef[4 * nlvl + N + n] = w_dist * lw_ld / (four + eps) * u(3 * nlvl + N + n)
    return losses, coef


def _lanes4(terms):
    """[rows, C] -> [rows]: lane q adds channels q, q + 4, ... in turn, then the xor-1 and xor-2 shuffles (lane 0)"""
    rows, C = terms.shape
    t = torch.nn.functional.pad(terms, (0, (-C) % 4)).reshape(rows, -1, 4)
    lanes = torch.zeros(rows, 4, dtype=terms.dtype)
    for i in range(t.shape[1]):
        lanes = lanes + t[:, i]
    lanes = lanes + lanes[:, [1, 0, 3, 2]]
    lanes = lanes + lanes[:, [2, 3, 0, 1]]
    return lanes[:, 0]


def restate(c, mut=None):
    """the whole chain the training step runs: gfl_losses_kernel<false>, loss_avg, l2 / kd forward, finalize (losses), finalize
    (coefficients under `up`), gfl_losses_kernel<true>, l2 / kd backward.  Returns what the kernels write."""
    N, A, L, c_old, c_all = c.N, c.A, c.nlvl, c.c_old, c.c_all
    cn = c_all - c_old
    zero, one = _f(0.0), _f(1.0)
    lvl = level_of(c.sizes)
    if mut == "level_of_block":
        lvl = lvl[(torch.arange(A) // GL_ROWS) * GL_ROWS]
    stride = torch.tensor(c.strides, dtype=F32)[lvl][None, :]                     # [1, A]
    lab = c.labels.clone()
    if mut == "bg_not_remapped":
        # planted in the form in which it bites: background taken as `label == cn` with the remap left out.  In the kernel's form
        # (`label < cn`) the remap is redundant: test_loss_refs_cpu.py asserts that too.
        is_pos = (lab >= 0) & (lab != cn)
    else:
        lab = torch.where(lab == c_all, torch.full_like(lab, cn), lab)
        is_pos = (lab >= 0) & (lab < cn)
    lw = torch.ones_like(c.lw) if mut == "lw_ignored" else c.lw
    q0 = 0 if mut == "qfl_all_channels" else c_old
    x = c.cls[:, :, q0:]
    nq = c_all - q0
    wt = torch.where(is_pos, 1.0 / (1.0 + torch.exp(-c.cls[:, :, c_old:].max(2)[0])), zero)
    # ---- decode (stride units), softmax17, IoU, GIoU, DFL
    an = c.anchors
    cx, cy = ((an[:, 2] + an[:, 0]) / 2.0)[None] / stride, ((an[:, 3] + an[:, 1]) / 2.0)[None] / stride
    z = c.bbox.reshape(N, A, 4, 17)
    mx = z.max(3, keepdim=True)[0]
    e = torch.exp(z - mx)
    ssum = R._seq_sum(e.reshape(-1, 17)).reshape(N, A, 4, 1)
    p = e * (1.0 / ssum)
    jb = torch.arange(17, dtype=F32)
    d = R._seq_sum((p * jb).reshape(-1, 17)).reshape(N, A, 4)
    lse = (mx + torch.log(ssum))[..., 0]
    pred = torch.stack([cx - d[..., 0], cy - d[..., 1], cx + d[..., 2], cy + d[..., 3]], -1)
    tg = c.bt / stride[..., None]
    g = NS(pred=pred.reshape(-1, 4), target=tg.reshape(-1, 4), coef=torch.ones(N * A), eps=1e-6)
    giou_rows, ggrad, _ = R.giou_restate(g, mut="ties_1_0" if mut == "ties_1_0" else None)
    giou_rows, ggrad = giou_rows.reshape(N, A), ggrad.reshape(N, A, 4)
    score = torch.where(is_pos, R.overlaps_restate(g.pred, g.target, "iou", True).reshape(N, A), zero)
    raw = torch.stack([cx - tg[..., 0], cy - tg[..., 1], tg[..., 2] - cx, tg[..., 3] - cy], -1)
    hi = _f(16.0) if mut == "dfl_clamp_16" else _f(16.0) - _f(0.1)
    y = torch.minimum(torch.maximum(raw, zero), hi)
    y = torch.where(is_pos[..., None], y, zero)
    tl = (y + 0.5).to(I64) if mut == "tl_rounds" else y.to(I64)
    wl, wr = (tl + 1).to(F32) - y, y - tl.to(F32)
    zp = torch.cat([z, torch.full((N, A, 4, 2), float("nan"))], 3)                 # (reading past z[16] is no number)
    zl, zr = zp.gather(3, tl[..., None])[..., 0], zp.gather(3, (tl + 1)[..., None])[..., 0]
    dfl_side = (lse - zl) * wl + (lse - zr) * wr
    dfl = (dfl_side[..., 0] + dfl_side[..., 1]) + (dfl_side[..., 2] + dfl_side[..., 3])
    probe = NS(is_pos=is_pos, pred=pred, tg=tg, raw=raw, y=y, tl=tl, wr=wr, d=d, lvl=lvl)         # what the edge assertions read
    # ---- QFL
    sg = 1.0 / (1.0 + torch.exp(-x))
    l1p = torch.log1p(torch.exp(-x.abs()))
    sp = x.clamp(min=0) + l1p
    M = is_pos[..., None] & (torch.arange(nq)[None, None, :] == lab[..., None])
    sc3 = score[..., None]
    bce = x.clamp(min=0) - x * sc3 + l1p
    u = sc3 - sg
    qsum = _lanes4(torch.where(M, bce * (u * u), sp * (sg * sg)).reshape(N * A, nq)).reshape(N, A)
    # ---- the f64 level sums
    out = NS(score=score, wt=wt, probe=probe)
    out.sums = torch.zeros(L, 4, dtype=F64)
    for l in range(L):
        m = (lvl == l)[None, :]
        pm = m & is_pos
        out.sums[l] = torch.stack([torch.where(m, (qsum * lw).double(), torch.zeros((), dtype=F64)).sum()] +
                                  [torch.where(pm, v.double(), torch.zeros((), dtype=F64)).sum() for v in (giou_rows * wt, dfl * wt, wt)])
    out.avg = avg_restate(c.num_pos, out.sums)
    nd = N if c.distill else 0
    if c.distill:
        t_old, s_old = c.t_cls[:, :, :c_old], c.cls[:, :, :c_old]
        sel = torch.zeros(N, A, dtype=torch.bool)
        for n in range(N):
            sel[n, c.idx_cls[n, :int(c.counts[n, 0])]] = True
        dl2 = torch.where(sel[..., None], s_old - t_old, zero)
        out.l2s = (dl2 * dl2).double().sum((1, 2))
        kall = c.cls if mut == "kd_weight_all_channels" else s_old
        kwt = 1.0 / (1.0 + torch.exp(-kall.max(2)[0]))
        kept = c.keep != 0
        kc = NS(pred=c.bbox.reshape(-1, 17), soft=c.t_bbox.reshape(-1, 17), T=c.T, nb=17, m=N * A * 4, coef=torch.ones(N * A * 4))
        kd_rows = R.kd_restate(kc, mut="T_not_T2" if mut == "T_not_T2" else None)[0].reshape(N, A, 4)
        out.kds = torch.where(kept[..., None], (kd_rows * kwt[..., None]).double(), torch.zeros((), dtype=F64)).sum((1, 2))
    else:
        out.l2s = out.kds = None
    fin = lambda upv: finalize_restate(out.sums, out.avg, out.l2s, out.kds, c.counts if c.distill else None, L, nd, c_old, c.weights, upv, mut)
    out.losses = fin(None)[0]
    coef = out.coef = fin(c.up)[1]
    # ---- backward
    cq = coef[4 * lvl + 0][None] * lw
    cb, cd = coef[4 * lvl + 1][None] * wt, coef[4 * lvl + 2][None] * wt
    sign = torch.tensor([-1.0, -1.0, 1.0, 1.0])
    gq = (sign * ggrad) * cb[..., None]
    tgtm = torch.where(jb.to(I64) == tl[..., None], wl[..., None], zero) + torch.where(jb.to(I64) == (tl + 1)[..., None], wr[..., None], zero)
    gz = gq[..., None] * p * (jb - d[..., None])
    gz = gz + cd[..., None, None] * ((p - torch.where(jb.to(I64) == tl[..., None], wl[..., None], zero))
                                     - torch.where(jb.to(I64) == (tl + 1)[..., None], wr[..., None], zero))
    out.dbbox = torch.where(is_pos[..., None, None], gz, zero).reshape(N, A, 68)
    gl = cq[..., None] * (-(u * u * u) - 2.0 * bce * u * sg * (1.0 - sg))
    gb = cq[..., None] * (sg * sg * sg + 2.0 * sp * sg * sg * (1.0 - sg))
    dnew = torch.where(M, gl, gb)
    old = c.cls[:, :, :q0] if mut == "old_channels_left" else torch.zeros(N, A, q0)
    out.dcls = torch.cat([old, dnew], 2).contiguous()
    if c.distill:
        base = 20 if mut == "distill_coef_at_20" else 4 * L
        cpad = torch.cat([coef, torch.full((24 + 2 * N,), float("nan"))])          # (reading past the vector is no number)
        cl, ck = cpad[base:base + N], cpad[base + N:base + 2 * N]
        out.dcls[:, :, :c_old] = out.dcls[:, :, :c_old] + torch.where(sel[..., None], cl[:, None, None] * 2.0 * dl2, zero)
        kc.coef = (ck[:, None] * kwt).reshape(-1, 1).expand(-1, 4).reshape(-1)
        kg = R.kd_restate(kc, mut="T_not_T2" if mut == "T_not_T2" else None)[1].reshape(N, A, 68)
        out.dbbox = out.dbbox + torch.where(kept[..., None], kg, zero)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------------------------
def _row_figures(c, r, got):
    """{kind: worst row-normalised error of `got` against the fp64 composition r}; sums are divided by the sum of their rows' scales"""
    s = r.scale
    N, A, c_old = c.N, c.A, c.c_old
    f = {"score": nerr(got.score, r.score, s.score), "wt": nerr(got.wt, r.wt, s.wt),
         "dcls_new": nerr(got.dcls[:, :, c_old:], r.dcls[:, :, c_old:], s.dcls_new)}
    for j, k in enumerate(("qfl", "giou", "dfl", "wt_sum")):
        f[k] = nerr(got.sums[:, j], r.sums[:, j], s.sums[:, j])
    db = s.dbbox
    if c.distill:
        db = db + s.dbbox_kd
        f["l2"] = nerr(got.l2s, r.l2s, s.l2s)
        f["kd"] = nerr(got.kds, r.kds, s.kds)
        f["dcls_old"] = nerr(got.dcls[:, :, :c_old], r.dcls[:, :, :c_old], s.dcls_old)
    f["dbbox"] = nerr(got.dbbox.reshape(N, A, 4, 17), r.dbbox.reshape(N, A, 4, 17), db)
    return f


def _yard_figures(c, r, y):
    """{kind: worst row-normalised error of the composition y against the fp64 composition r}: the outputs that are rows as they
    stand, and the ROWS (QFL, GIoU, DFL per anchor, KD-KL per box side, L2 per anchor) behind the sums"""
    s = r.scale
    N, A, c_old = c.N, c.A, c.c_old
    f = {"score": nerr(y.score, r.score, s.score), "wt": nerr(y.wt, r.wt, s.wt), "dcls_new": nerr(y.dcls[:, :, c_old:], r.dcls[:, :, c_old:], s.dcls_new),
         "qfl": nerr(y.qfl, r.qfl, s.qfl), "giou": nerr(y.giou, r.giou, s.giou), "dfl": nerr(y.dfl, r.dfl, s.dfl)}
    f["wt_sum"] = f["wt"]
    db = s.dbbox
    if c.distill:
        db = db + s.dbbox_kd
        f["l2"] = nerr(y.l2_rows, r.l2_rows, s.l2)
        f["kd"] = nerr(y.kd_rows, r.kd_rows, s.kd)
        f["dcls_old"] = nerr(y.dcls[:, :, :c_old], r.dcls[:, :, :c_old], s.dcls_old)
    f["dbbox"] = nerr(y.dbbox.reshape(N, A, 4, 17), r.dbbox.reshape(N, A, 4, 17), db)
    return f


@functools.lru_cache(maxsize=None)
def e32():
    """{kind: E32}: the fp32 yardstick against ref64 over the whole table, from the reference alone.  For a kind that the kernels
    give out as sums, E32 is that of its ROWS: a sum may deviate by 4 x E32_rows x the sum of its rows' scales (the triangle
    inequality; the kernels add fp32 rows in f64)."""
    fig = {}
    for i, c in enumerate(cases()):
        for k, v in _yard_figures(c, ref64(i), compose(c, F32)).items():
            fig[k] = max(fig.get(k, 0.0), v)
    return fig


def figures(c, i, got):
    return _row_figures(c, ref64(i), got)


def exact_violations(c, got):
    """the parts held to bit-equality, each against the restatement applied to what `got` itself holds"""
    bad = []
    N, L, c_old = c.N, c.nlvl, c.c_old
    nd = N if c.distill else 0
    avg = avg_restate(c.num_pos, got.sums)
    if not torch.equal(got.avg, avg):
        bad.append("avg")
    cnt = c.counts if c.distill else None
    losses = finalize_restate(got.sums, got.avg, got.l2s, got.kds, cnt, L, nd, c_old, c.weights, None)[0]
    coef = finalize_restate(got.sums, got.avg, got.l2s, got.kds, cnt, L, nd, c_old, c.weights, c.up)[1]
    if not torch.equal(got.losses, losses):
        bad.append("losses")
    if not torch.equal(got.coef, coef):
        bad.append("coef")
    lab = torch.where(c.labels == c.c_all, torch.full_like(c.labels, c.c_all - c_old), c.labels)
    neg = ~((lab >= 0) & (lab < c.c_all - c_old))
    if bool((got.score[neg] != 0).any()) or bool((got.wt[neg] != 0).any()):
        bad.append("score/wt of non-positives")
    untouched = neg if not c.distill else neg & (c.keep == 0)
    if bool((got.dbbox[untouched] != 0).any()):
        bad.append("dbbox of non-positives")
    sel = torch.zeros(N, c.A, dtype=torch.bool)
    if c.distill:
        for n in range(N):
            sel[n, c.idx_cls[n, :int(c.counts[n, 0])]] = True
    if bool((got.dcls[:, :, :c_old][~sel] != 0).any()):
        bad.append("old channels of dcls")
    return bad


def violations(c, i, got, E=None):
    """every breach of the rule by `got` on case i: [(what, figure, bound)]"""
    E = e32() if E is None else E
    bad = [(k, v, FACTOR * E[k]) for k, v in figures(c, i, got).items() if not v <= FACTOR * E[k]]
    return bad + [(w, float("inf"), 0.0) for w in exact_violations(c, got)]


# ---------------------------------------------------------------------------------------------------------------------
# the decision kernels: cases whose oracle answer does not depend on an order among equals
# ---------------------------------------------------------------------------------------------------------------------
def ers_cases():
    """(name, cls [N, A, C], bbox [N, A, 68]): A in {1, 2, 257, 1025}; A = 100 with N = 5 (a 256-row block spans three images); a
    constant map (the strict `>` selects nothing); C % 4 == 0 and the generic path.  A few anchors are raised so that the selection
    is not empty and no maximum lies near the threshold."""
    out = []
    for k, (N, A, C) in enumerate([(1, 1, 40), (1, 2, 40), (1, 257, 40), (2, 1025, 40), (5, 100, 40), (5, 100, 70), (2, 257, 37)]):
        g = _gen(400 + k)
        cls = -3.0 + torch.randn(N, A, C, generator=g)
        bbox = torch.randn(N, A, 68, generator=g)
        for n in range(N):
            cls[n, n::17, (3 + n) % C] += 9.0
            bbox[n, (n + 5)::23, 11 + n] += 9.0
        out.append(NS(name=f"ers_N{N}A{A}C{C}", cls=cls, bbox=bbox))
    out.append(NS(name="ers_constant", cls=torch.full((2, 130, 40), -1.25), bbox=torch.full((2, 130, 68), 0.5)))
    return out


def _onehot_rows(d4):
    z = torch.full((68,), -90.0)
    for q, d in enumerate(d4):
        z[q * 17 + int(d)] = 90.0
    return z


def nms_cases():
    """A = 3 anchors of stride 8 on one row (centres x = 0, 8, 16), 4 teacher classes, one-hot +-90 box rows: integer distances, so
    the boxes (pixel centre -/+ stride-unit distance) are exact.  (name, t_cls, t_bbox, idx [N, A], K per image):
    K in {0, 1, 2}, N = 2 with different K; all-equal scores on disjoint boxes; two identical boxes of one class with different
    scores (the lower one goes) and of two classes (both stay)."""
    def img(dists, logits):
        return torch.stack([_onehot_rows(d) for d in dists]), torch.tensor(logits, dtype=F32)
    same = [(2, 3, 10, 3), (10, 3, 2, 3), (1, 1, 1, 1)]            # anchors 0 and 1 decode to (-2, -3, 10, 3) alike
    apart = [(1, 1, 1, 1)] * 3
    one = [[-1., -5, -5, -5], [2., -5, -5, -5], [0., -5, -5, -5]]   # class 0 everywhere, anchor 1 scores highest
    two = [[-1., -5, -5, -5], [-5., -5, 2., -5], [0., -5, -5, -5]]  # anchor 1 is of class 2
    flat = [[-5., 1., -5, -5], [-5., 1., -5, -5], [-5., 1., -5, -5]]
    spec = [("nms_K0_K1", (same, one, []), (apart, flat, [2])),
            ("nms_identical_one_class", (same, one, [0, 1]), (apart, flat, [0, 1, 2])),
            ("nms_identical_two_classes", (same, two, [0, 1]), (apart, one, [0, 2]))]
    out = []
    for name, *imgs in spec:
        tb, tc = zip(*[img(d, lg) for d, lg, _ in imgs])
        idx = torch.zeros(2, 3, dtype=I64)
        for n, (_, _, sel) in enumerate(imgs):
            idx[n, :len(sel)] = torch.tensor(sel, dtype=I64)
        out.append(NS(name=name, t_cls=torch.stack(tc), t_bbox=torch.stack(tb), idx=idx, K=[len(s[2]) for s in imgs], sizes=[(1, 3)], strides=[8]))
    return out


def nms_oracle(c, n, order=None):
    """the kept anchors (a sorted list) of image n by O.nms_class_offset, the candidates taken in `order`"""
    anchors = torch.cat(O.grid_anchors(c.sizes, c.strides), 0)
    idx = c.idx[n, :c.K[n]]
    if order is not None:
        idx = idx[order]
    dec = O.distance2bbox(O.anchor_centers(anchors), O.integral(c.t_bbox[n]))
    conf, ids = c.t_cls[n].sigmoid().max(-1)
    keep = O.nms_class_offset(dec[idx], conf[idx], ids[idx], 0.005)
    return sorted(int(v) for v in idx[keep])


def atss_cases():
    """one level of 4 x 4 anchors of stride 8 (centres at multiples of 8), top-k 9.  Image 0: a box centred on (4, 4), equidistant
    from the four centres around it; the nine nearest centres end with (16, 16) alone at its distance, so no tie is cut by top-k.
    Image 1: a box around (4, 4) that holds no anchor centre: zero positives."""
    return [NS(name="atss_equidistant_and_empty", sizes=[(4, 4)], strides=[8],
               boxes=[torch.tensor([[-3., -3., 11., 11.]]), torch.tensor([[1., 1., 7., 7.]])],
               labels=[torch.tensor([2]), torch.tensor([5])], num_classes=80)]


def atss_oracle(c, n, perm=None):
    """O.get_targets_single of image n; `perm` reorders the anchors before the assignment and the answer is put back"""
    anchors = torch.cat(O.grid_anchors(c.sizes, c.strides), 0)
    A = anchors.shape[0]
    p = torch.arange(A) if perm is None else perm
    lab, lw, bt, npos = O.get_targets_single(anchors[p], torch.ones(A, dtype=torch.bool), [A], c.boxes[n], c.labels[n], c.num_classes)
    inv = torch.empty(A, dtype=I64)
    inv[p] = torch.arange(A)
    return lab[inv], lw[inv], bt[inv], npos
