"""References, restatement and case tables of IoULoss / DIoULoss / CIoULoss (erd_amd/csrc/erd_box_loss.h: erd_iou_loss of
leaf_ops.hip and the box term of gfl_losses_kernel).  Imports no erd_amd: tests/test_iou_refs_cpu.py proves on the CPU that the
restatement is the reference (fixture tests/golden/f14_iou_losses.npz, written by tools/gen_iou_loss_golden.py from the real
mmdet/models/losses/iou_loss.py, and the live reference where its tree is present) and that the rule bites;
tests/test_gpu_iou_loss.py holds the kernels to it.

  restate(kind, pred, target, eps, dtype)   the reference's expressions in the reference's order in torch ops under autograd
                                            (iou_loss.py:16-54, 130-181, 185-246), with one switch per planted mistake
  ref64 / e32                               the restatement in float64, and the worst row-normalised error of the float32 one
                                            against it: the rule is leaf_refs' own, FACTOR = 4 times E32 per kind

Row scales (leaf_refs' style: an error is divided by its own row's magnitude, the sum of the magnitudes of the terms it adds):
  IoU rows    'linear' 1 + iou, 'square' 1 + iou^2, 'log' 1 + |log iou| (a relative error of the IoU is an absolute one of its log)
  DIoU rows   1 + iou + (rho2 + |sx| Sx / 2 + |sy| Sy / 2) / c2: sx = (b2_x1 + b2_x2) - (b1_x1 + b1_x2) is a difference of two sums of
              magnitude Sx = |b2_x1 + b2_x2| + |b1_x1 + b1_x2|, and its square passes that rounding on with 2 |sx|
  CIoU rows   the DIoU scale plus alpha (3 V + v (1 + iou) / (1 - iou + v)), V = 4 / pi^2 (|atan(w2 / h2)| + |atan(w1 / h1)|)^2: the
              CANCELLATION in atan(a) - atan(b) (each arctangent carries the rounding of its own magnitude; v and alpha both inherit
              it) and the one in 1 - iou of alpha's denominator
  gradients   |coef| times the largest per-coordinate sum of the magnitudes of the terms autograd adds: |d overlap| / union +
              overlap / union^2 (|d area| + |d overlap|), Sx / 2 / c2 + rho2 / c2^2 |d c2|, and alpha |d v| with the same two
              cancellations
  no scale is smaller than the least normal fp32 number (leaf_refs.nerr)

Exclusion.  A row is left out of E32 and of every GPU comparison only where the CPU fp32 evaluation itself is not finite:
ciou_loss on two identical boxes (union + eps == union in fp32, ious == 1, alpha = 0 / 0).  tests/test_iou_refs_cpu.py asserts
that this is exactly every copy of leaf_refs.BOX_FAMILY[0] under CIoU and nothing else."""
import contextlib
import functools
import math
from types import SimpleNamespace as NS

import torch

import leaf_refs as R
from leaf_refs import F32, F64, FACTOR, EPS32, nerr, worst
from oracle import erd_oracle as O

KINDS = ("iou_log", "iou_linear", "iou_square", "diou", "ciou")
# enum erd_box_loss (include/erd_hip.h)
KIND_ID = {"giou": 0, "iou_log": 1, "iou_linear": 2, "iou_square": 3, "diou": 4, "ciou": 5}
EPS = 1e-6
CIOU_FACTOR = 4 / math.pi ** 2

MUTATIONS = {
    "ties_1_0": ("diou", "ciou", "iou_linear"),
    "alpha_not_detached": ("ciou",),
    "eps_clamped": ("diou", "ciou"),
    "h_without_eps": ("ciou",),
    "rho2_without_quarter": ("diou", "ciou"),
    "square_as_linear": ("iou_square",),
    "clamp_passes_below_eps": ("iou_log", "iou_linear", "iou_square"),
}


# ---------------------------------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------------------------------
EXTRA_ROWS = [          # (pred, target, what): what leaf_refs.BOX_FAMILY lacks
    ((0., 0., 10., 10.), (0., 0., 10., 20.004), "IoU just below 0.5: CIoU's indicator is 0"),
    ((0., 0., 10., 10.), (0., 0., 10., 19.996), "IoU just above 0.5: CIoU's indicator is 1"),
    ((10., 20., 50., 80.), (12., 23., 44., 71.), "equal aspect ratios (2 : 3), different sizes: v == 0 up to eps"),
    ((0., 0., 20., 30.), (5., 5., 45., 65.), "equal aspect ratios, IoU below 0.5"),
    ((0., 0., 400., 4.), (1., 0., 5., 4.5), "w / h = 100 against 0.9: a large atan difference"),
    ((0., 0., 4., 400.), (0., 1., 4.5, 380.), "w / h = 0.01 on both sides, IoU above 0.5"),
    ((0., 0., 300., 3.), (2., 0.5, 290., 3.5), "w / h = 100 on both sides, IoU above 0.5: atan(a) - atan(b) cancels"),
    ((10., 20., 50., 80.), (100., 200., 150., 260.), "disjoint: IoU 'log' clamps to eps, zero gradient"),
    ((10., 20., 50., 80.), (11., 21., 51., 81.), "IoU near 1, nothing tied"),
    ((0., 0., 0.001, 0.001), (0., 0., 0.001, 0.002), "areas of the order of eps: DIoU / CIoU add eps to the union, they do not clamp"),
]


def _case(name, a, b, seed):
    n = a.shape[0]
    coef = torch.randn(n, generator=R._gen(seed))
    coef[6::9] = 0.0
    return NS(name=name, n=n, pred=a, target=b, coef=coef)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for n in (1, 255, 257):
        a, b = R.family_boxes(n, affine=True)
        out.append(_case(f"family{n}", a, b, 8100 + n))
    a, b = R.random_boxes(300, 8300)
    out.append(_case("random300", a, b, 8400))
    a = torch.tensor([r[0] for r in EXTRA_ROWS], dtype=F32)
    b = torch.tensor([r[1] for r in EXTRA_ROWS], dtype=F32)
    out.append(_case("extra", a, b, 8500))
    return out


def family_row0(c):
    """the rows of a case that are a copy of leaf_refs.BOX_FAMILY[0] (two identical boxes)"""
    m = torch.zeros(c.n, dtype=torch.bool)
    if c.name.startswith("family"):
        m[0::len(R.BOX_FAMILY)] = True
    return m


# ---------------------------------------------------------------------------------------------------------------------
# the restatement (the reference's order, torch ops, autograd)
# ---------------------------------------------------------------------------------------------------------------------
def _max(a, b, mut):
    return torch.where(a >= b, a, b) if mut == "ties_1_0" else torch.max(a, b)      # (where: the whole gradient to the first)


def _min(a, b, mut):
    return torch.where(a <= b, a, b) if mut == "ties_1_0" else torch.min(a, b)


def rows_fn(kind, pred, target, eps=EPS, mut=None):
    """the loss rows [n] of `kind` at the dtype of pred, differentiable w.r.t. pred"""
    lt = _max(pred[:, :2], target[:, :2], mut)
    rb = _min(pred[:, 2:], target[:, 2:], mut)
    wh = (rb - lt).clamp(min=0)
    overlap = wh[:, 0] * wh[:, 1]
    ap = (pred[:, 2] - pred[:, 0]) * (pred[:, 3] - pred[:, 1])
    ag = (target[:, 2] - target[:, 0]) * (target[:, 3] - target[:, 1])
    if kind.startswith("iou_"):
        # bbox_overlaps(pred, target, is_aligned=True): the union clamp is the function's own 1e-6 (bbox_overlaps.py:151-199)
        union = torch.max(ap + ag - overlap, pred.new_tensor([1e-6]))
        raw = overlap / union
        ious = raw.clamp(min=eps)
        if mut == "clamp_passes_below_eps":
            ious = raw + (ious - raw).detach()
        mode = kind[4:]
        if mode == "linear" or (mode == "square" and mut == "square_as_linear"):
            return 1 - ious
        if mode == "square":
            return 1 - ious ** 2
        return -ious.log()
    if mut == "eps_clamped":
        union = (ap + ag - overlap).clamp(min=eps)
    else:
        union = ap + ag - overlap + eps
    ious = overlap / union
    enclose_x1y1 = _min(pred[:, :2], target[:, :2], mut)
    enclose_x2y2 = _max(pred[:, 2:], target[:, 2:], mut)
    enclose_wh = (enclose_x2y2 - enclose_x1y1).clamp(min=0)
    cw, ch = enclose_wh[:, 0], enclose_wh[:, 1]
    c2 = (cw ** 2 + ch ** 2).clamp(min=eps) if mut == "eps_clamped" else cw ** 2 + ch ** 2 + eps
    b1_x1, b1_y1, b1_x2, b1_y2 = pred[:, 0], pred[:, 1], pred[:, 2], pred[:, 3]
    b2_x1, b2_y1, b2_x2, b2_y2 = target[:, 0], target[:, 1], target[:, 2], target[:, 3]
    left = ((b2_x1 + b2_x2) - (b1_x1 + b1_x2)) ** 2
    right = ((b2_y1 + b2_y2) - (b1_y1 + b1_y2)) ** 2
    if mut != "rho2_without_quarter":
        left, right = left / 4, right / 4
    rho2 = left + right
    if kind == "diou":
        return 1 - (ious - rho2 / c2)
    he = 0.0 if mut == "h_without_eps" else eps
    w1, h1 = b1_x2 - b1_x1, b1_y2 - b1_y1 + he
    w2, h2 = b2_x2 - b2_x1, b2_y2 - b2_y1 + he
    v = CIOU_FACTOR * torch.pow(torch.atan(w2 / h2) - torch.atan(w1 / h1), 2)
    with torch.set_grad_enabled(mut == "alpha_not_detached"):
        alpha = (ious > 0.5).to(pred.dtype) * v / (1 - ious + v)
    cious = ious - (rho2 / c2 + alpha * v)
    return 1 - cious.clamp(min=-1.0, max=1.0)


def restate(kind, c, dtype=F32, mut=None, eps=EPS):
    """(rows, dpred) with dpred = d sum_i coef_i rows_i / d pred"""
    p = R._leaf(c.pred, dtype)
    rows = rows_fn(kind, p, c.target.to(dtype), eps, mut)
    (rows * c.coef.to(dtype)).sum().backward()
    return rows.detach(), p.grad


def scales(kind, c, eps=EPS):
    """(row scale [n], gradient scale [n]) in fp64: the module docstring"""
    a, b = c.pred.double(), c.target.double()
    ax, ay, az, aw = a.unbind(1)
    bx, by, bz, bw = b.unbind(1)
    zero, one, half = (torch.tensor(v, dtype=F64) for v in (0.0, 1.0, 0.5))

    def gmax(x, y):
        return torch.where(x > y, one, torch.where(x == y, half, zero))

    def gmin(x, y):
        return torch.where(x < y, one, torch.where(x == y, half, zero))

    w0, h0 = torch.minimum(az, bz) - torch.maximum(ax, bx), torch.minimum(aw, bw) - torch.maximum(ay, by)
    w, h = w0.clamp(min=0), h0.clamp(min=0)
    pw, ph = (w0 >= 0).double(), (h0 >= 0).double()
    ov = w * h
    d_ov = torch.stack([gmax(ax, bx) * pw * h, gmax(ay, by) * ph * w, gmin(az, bz) * pw * h, gmin(aw, bw) * ph * w], 1)
    d_a1 = torch.stack([(aw - ay).abs(), (az - ax).abs(), (aw - ay).abs(), (az - ax).abs()], 1)
    uni0 = (az - ax) * (aw - ay) + (bz - bx) * (bw - by) - ov
    cf = c.coef.double().abs()
    if kind.startswith("iou_"):
        uni = uni0.clamp(min=1e-6)
        iou = ov / uni
        ic = iou.clamp(min=eps)
        gate = (uni0 > 1e-6).double()[:, None]
        diou = d_ov / uni[:, None] + (ov / (uni * uni))[:, None] * (d_a1 + d_ov) * gate
        passes = (iou >= eps).double()
        mode = kind[4:]
        if mode == "log":
            return 1 + ic.log().abs(), cf * passes / ic * diou.max(1)[0]
        if mode == "linear":
            return 1 + ic, cf * passes * diou.max(1)[0]
        return 1 + ic * ic, cf * passes * 2 * ic * diou.max(1)[0]
    uni = uni0 + eps
    iou = ov / uni
    diou = d_ov / uni[:, None] + (ov / (uni * uni))[:, None] * (d_a1 + d_ov)
    ew0, eh0 = torch.maximum(az, bz) - torch.minimum(ax, bx), torch.maximum(aw, bw) - torch.minimum(ay, by)
    cw, ch = ew0.clamp(min=0), eh0.clamp(min=0)
    qw, qh = (ew0 >= 0).double(), (eh0 >= 0).double()
    c2 = cw * cw + ch * ch + eps
    d_c2 = torch.stack([2 * cw * gmin(ax, bx) * qw, 2 * ch * gmin(ay, by) * qh, 2 * cw * gmax(az, bz) * qw, 2 * ch * gmax(aw, bw) * qh], 1)
    sx, sy = (bx + bz) - (ax + az), (by + bw) - (ay + aw)
    Sx, Sy = (bx + bz).abs() + (ax + az).abs(), (by + bw).abs() + (ay + aw).abs()
    rho2 = sx * sx / 4 + sy * sy / 4
    rows = 1 + iou.abs() + (rho2 + sx.abs() * Sx / 2 + sy.abs() * Sy / 2) / c2
    d_rho = torch.stack([Sx, Sy, Sx, Sy], 1) / 2
    grad = diou + d_rho / c2[:, None] + (rho2 / (c2 * c2))[:, None] * d_c2
    if kind == "diou":
        return rows, cf * grad.max(1)[0]
    w1, h1 = az - ax, aw - ay + eps
    w2, h2 = bz - bx, bw - by + eps
    r1 = w1 / h1
    A, B = torch.atan(w2 / h2), torch.atan(r1)
    d = A - B
    v = CIOU_FACTOR * d * d
    V = CIOU_FACTOR * (A.abs() + B.abs()) ** 2
    den = 1 - iou + v
    ind = (iou > 0.5).double()
    den = torch.where(ind > 0, den, torch.ones_like(den))
    alpha = ind * v / den
    rows = rows + alpha * (3 * V + v * (1 + iou) / den)
    d_r1 = torch.stack([1 / h1.abs(), (w1 / (h1 * h1)).abs(), 1 / h1.abs(), (w1 / (h1 * h1)).abs()], 1)
    dv_mag = (CIOU_FACTOR * 2 * (A.abs() + B.abs()) / (1 + r1 * r1))[:, None] * d_r1
    dv_true = (CIOU_FACTOR * 2 * d.abs() / (1 + r1 * r1))[:, None] * d_r1
    grad = grad + (alpha * (1 + (1 + iou) / den))[:, None] * dv_mag + (ind / den * 2 * V)[:, None] * dv_true
    cious = iou - (rho2 / c2 + alpha * v)
    passes = ((cious >= -1) & (cious <= 1)).double()
    return rows, cf * passes * grad.max(1)[0]


@functools.lru_cache(maxsize=None)
def ref64(kind):
    """[(case, rows64, grad64, row scale, gradient scale, excluded [n] bool)]: computed once, shared, left unchanged.  `excluded`:
    where the CPU fp32 evaluation is not finite (the module docstring)"""
    out = []
    for c in cases():
        rows, grad = restate(kind, c, F64)
        r32, g32 = restate(kind, c, F32)
        rs, gs = scales(kind, c)
        excl = ~(torch.isfinite(r32) & torch.isfinite(g32).all(1))
        out.append((c, rows, grad, rs, gs, excl))
    return out


def figures(kind, fn):
    """worst row-normalised errors (rows, gradient) of fn(case) -> (rows or None, grad or None) against ref64, excluded rows left out"""
    er, eg = [], []
    for c, rows, grad, rs, gs, excl in ref64(kind):
        got = fn(c)
        keep = ~excl
        if got[0] is not None:
            er.append(nerr(got[0][keep], rows[keep], rs[keep]))
        if got[1] is not None:
            eg.append(nerr(got[1][keep], grad[keep], gs[keep]))
    return worst(er), worst(eg)


@functools.lru_cache(maxsize=None)
def e32(kind):
    """(E32 of the rows, E32 of the gradient): the fp32 restatement on the CPU against the fp64 one"""
    return figures(kind, lambda c: restate(kind, c, F32))


# ---------------------------------------------------------------------------------------------------------------------
# the modules' forward (iou_loss.py:341-389, 553-599, 625-671)
# ---------------------------------------------------------------------------------------------------------------------
def module_forward(kind, pred, target, weight=None, avg_factor=None, reduction="mean", loss_weight=1.0, eps=EPS):
    """IoULoss / DIoULoss / CIoULoss.forward restated, any dtype"""
    early = weight is not None and not bool(torch.any(weight > 0))
    if early and (not kind.startswith("iou_") or reduction != "none"):
        if pred.dim() == weight.dim() + 1:
            weight = weight.unsqueeze(1)
        return (pred * weight).sum()
    if weight is not None and weight.dim() > 1:
        assert weight.shape == pred.shape
        weight = weight.mean(-1)
    return R.reduce_ref(rows_fn(kind, pred, target, eps), weight, reduction, avg_factor, loss_weight)


MODULE_RUNS = [          # (reduction, avg_factor, weight form)
    ("none", None, None), ("mean", None, None), ("sum", None, None), ("mean", 37.0, None), ("none", 37.0, "n"),
    ("mean", None, "n"), ("sum", None, "n4"), ("mean", 11.5, "n4"), ("mean", None, "zero"), ("sum", None, "zero4"), ("none", None, "zero"),
]


def module_weight(c, form):
    if form is None:
        return None
    g = R._gen(8600 + c.n)
    if form == "n":
        w = torch.rand(c.n, generator=g)
        w[2::5] = 0.0
        return w
    if form == "n4":
        return torch.rand(c.n, 4, generator=g)
    return torch.zeros(c.n) if form == "zero" else torch.zeros(c.n, 4)


# ---------------------------------------------------------------------------------------------------------------------
# the step with another loss_bbox
# ---------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def swap_box_loss(kind, eps=EPS, mode=None):
    """For its duration O.giou_loss_module is a function of the same signature that evaluates `kind` ('iou' with `mode`, 'diou',
    'ciou', or the 'iou_<mode>' spelling): O.loss_by_feat_single, O.erd_head_loss, O.gfl_head_loss and O.erd_step_loss then evaluate
    the step with that loss_bbox.  oracle/ is not edited."""
    if kind == "iou":
        kind = "iou_" + (mode or "log")
    assert kind in KINDS, kind

    def box_loss_module(pred, target, weight, avg_factor, loss_weight=2.0, eps=eps):
        if not bool(torch.any(weight > 0)):
            return (pred * weight.unsqueeze(1)).sum()
        return loss_weight * O.weight_reduce(rows_fn(kind, pred, target, eps), weight, avg_factor)

    saved = O.giou_loss_module
    O.giou_loss_module = box_loss_module
    try:
        yield
    finally:
        O.giou_loss_module = saved


CHAIN_SIZES, CHAIN_STRIDES = [(8, 9), (3, 4)], (8, 16)        # A = 72 + 12 = 84: one 64-row block boundary is crossed


@functools.lru_cache(maxsize=None)
def chain_cases():
    """the fused chain on given targets (loss_refs.make_case): positives on the first anchor, on both sides of the block boundary
    and on the last anchor of image 0, one on level 1 of image 1; a batch without any positive; plain GFL (no distillation)"""
    import loss_refs as LR
    pos = [(0, 0, 0), (0, 63, 1), (0, 64, 2), (0, 83, 3), (1, 75, 1)]
    out = [LR.make_case("box_erd", CHAIN_SIZES, CHAIN_STRIDES, 2, 3, 7, 8700, pos=pos, up="distinct", cls_shift=1),
           LR.make_case("box_nopos", CHAIN_SIZES, CHAIN_STRIDES, 2, 3, 7, 8701, pos=[], up="distinct", cls_shift=1),
           LR.make_case("box_gfl", CHAIN_SIZES, CHAIN_STRIDES, 2, 0, 4, 8702, pos=pos, up="distinct", cls_shift=1)]
    # make_case's targets sit far from the decoded boxes (IoU < 0.5: CIoU's alpha is 0 there).  Two positives get a target near
    # their own decoded box with another aspect ratio, so that IoU > 0.5 and v > 0: the alpha term and its gradient are live
    lv = LR.level_of(CHAIN_SIZES)
    for c in (out[0], out[2]):
        ctr = O.anchor_centers(c.anchors)
        for n, a in ((0, 63), (1, 75)):
            s = float(CHAIN_STRIDES[int(lv[a])])
            d = O.integral(c.bbox[n, a].reshape(1, 68)).reshape(4) * torch.tensor([1.25, 0.85, 1.2, 0.9])
            c.bt[n, a] = torch.stack([ctr[a, 0] - d[0] * s, ctr[a, 1] - d[1] * s, ctr[a, 0] + d[2] * s, ctr[a, 1] + d[3] * s])
    return out


@functools.lru_cache(maxsize=None)
def chain_ref64(kind, i):
    return compose(chain_cases()[i], F64, kind, want_scales=True)


@functools.lru_cache(maxsize=None)
def chain_e32(kind):
    """{'giou': E32 of the box-loss rows, 'dbbox': E32 of the dbbox rows} of the composition under `kind` over chain_cases()"""
    import loss_refs as LR
    fig = {}
    for i, c in enumerate(chain_cases()):
        for k, v in LR._yard_figures(c, chain_ref64(kind, i), compose(c, F32, kind)).items():
            fig[k] = max(fig.get(k, 0.0), v)
    return fig


class _OneMinus:
    """stands for 1 - rows where loss_refs writes `1 - O.bbox_overlaps(..., mode='giou')`: `1 - this` gives the rows back exactly"""

    def __init__(self, rows):
        self.rows = rows

    def __rsub__(self, one):
        assert one == 1
        return self.rows

    def sum(self):
        return -self.rows.sum()


def compose(c, dtype, kind, eps=EPS, want_scales=False):
    """loss_refs.compose(c, dtype) with `kind` as the head's loss_bbox: under swap_box_loss, and with the two places where loss_refs
    names the GIoU itself (the rows of _level_rows, the gradient magnitude of _scales) given the kind's rows and magnitudes.  The
    row scale of the box term is the kind's own (scales) in place of GIoU's constant 3."""
    import loss_refs as LR
    saved_ov, saved_gs = O.bbox_overlaps, LR._giou_scales

    def overlaps(b1, b2, mode="iou", is_aligned=False, **kw):
        if mode == "giou":
            assert is_aligned
            return _OneMinus(rows_fn(kind, b1, b2, eps))
        return saved_ov(b1, b2, mode=mode, is_aligned=is_aligned, **kw)

    def kind_scales(ns):
        rs, gs = scales(kind, NS(pred=ns.pred, target=ns.target, coef=ns.coef, n=ns.pred.shape[0]), eps)
        return rs, gs

    O.bbox_overlaps, LR._giou_scales = overlaps, kind_scales
    try:
        with swap_box_loss(kind, eps):
            out = LR.compose(c, dtype, want_scales=want_scales)
    finally:
        O.bbox_overlaps, LR._giou_scales = saved_ov, saved_gs
    if want_scales:
        off = LR.lvl_off(c.sizes)
        for l, lv in enumerate(out.lv):
            if len(lv.pos):
                rs = scales(kind, NS(pred=lv.dec, target=lv.tgt, coef=torch.ones(len(lv.pos)), n=len(lv.pos)), eps)[0]
                flat = out.scale.giou[:, off[l]:off[l + 1]].reshape(-1).clone()
                flat[lv.pos] = flat[lv.pos] - 3.0 + rs
                out.scale.giou[:, off[l]:off[l + 1]] = flat.reshape(c.N, -1)
            out.scale.sums[l, 1] = (out.scale.giou * out.wt)[:, off[l]:off[l + 1]].sum()
    return out
