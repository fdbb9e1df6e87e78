"""References, restatements and case tables of the stand-alone leaf operators (erd_amd/csrc/leaf_ops.hip, erd_amd/leaf.py).
Imports no erd_amd: tests/test_leaf_refs_cpu.py proves on the CPU that the references are right and that the rule bites,
tests/test_gpu_leaf_exact.py holds the kernels to it.

Three things per operator:

  ref64     the oracle's function (oracle/erd_oracle.py, pinned to the reference by tests/test_oracle_vs_reference.py) in float64
            under autograd: every value and every gradient, plus one SCALE per row (one anchor, one box, one box side)
  yardstick the same oracle function in float32 on the CPU
  restate   the kernel's expression in the kernel's operation order, in fp32 torch ops on the CPU, with switches that plant one
            mistake each (MUTATIONS): the negative controls of the rule, and the expected value of the operators that are
            held to bit-equality

Row scales.  An error is always divided by its own row's scale, never by the tensor's maximum.  The scale is the sum of the
MAGNITUDES of the terms a row adds, so a row whose terms cancel (pred == soft: 1e-18 in fp64) is not held to a relative
error fp32 cannot reach:
  * a sum of products is scaled by the sum of |product|; a binary cross entropy max(x, 0) - x t + log1p(exp(-|x|)) by the sum
    of its three magnitudes
  * a softmax probability p_b = exp(z_b - lse) carries the rounding of its exponent's operands, eps (|z_b| + |lse|), into
    p_b: its magnitude is u_b = p_b (1 + |z_b| + |max| + log s).  Without that factor one row with a logit at +-40 .. 80 sets
    E32 for the whole operator and loosens the bound for every ordinary row
  * a gradient row c (softmax - target) is scaled by |c| max_b (u_b + target_b); a QFL gradient row by |c| times the largest
    per-class magnitude, with 1 - sigma counted as the difference of 1 and sigma that it is; a GIoU gradient row by |c| times the
    magnitudes of the four terms it adds, the enclosing-area term in the two-term form the reference's autograd adds
  * no scale is smaller than the least normal fp32 number: below it fp32 has no relative precision to be held to

The rule (operators with expf / logf / log1pf): E32(op) is the worst row-normalised error of the fp32 yardstick against
ref64 over the operator's cases, measured when the test runs; the kernel's worst figure may be at most FACTOR = 4 times it.
The operators made of add / sub / mul / IEEE divide / min / max must equal the restatement bit for bit."""
import functools
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

from oracle import erd_oracle as O

F32, F64 = torch.float32, torch.float64
TINY = float(torch.finfo(F32).tiny)
EPS32 = float(torch.finfo(F32).eps)
FACTOR = 4.0
INF = float("inf")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _leaf(t, dtype):
    """a fresh autograd leaf: the case tables are shared and stay unchanged"""
    return t.detach().to(dtype).clone().requires_grad_(True)


def nerr(x, ref, scale):
    """worst |x - ref| / max(scale, TINY) over a tensor whose leading dimension are the rows of `scale`; NaN counts as inf"""
    if ref.numel() == 0:
        assert x.numel() == 0
        return 0.0
    assert x.shape == ref.shape, (x.shape, ref.shape)
    s = scale.double().clamp(min=TINY)
    while s.dim() < ref.dim():
        s = s.unsqueeze(-1)
    e = (x.double() - ref.double()).abs() / s
    e = torch.where(torch.isnan(e), torch.full_like(e, INF), e)
    return float(e.max())


def worst(pairs):
    return max([0.0] + list(pairs))


# ---------------------------------------------------------------------------------------------------------------------
# QFL
# ---------------------------------------------------------------------------------------------------------------------
QFL_SHAPES = [(1, 1), (5, 40), (7, 64), (6, 65), (9, 80), (3, 129), (1030, 80)]
_SAT = (0.0, 30.0, -30.0, 90.0, -90.0)


def _qfl_case(n, C, all_bg=False):
    g = _gen(1000 + 31 * n + C)
    pred = -2.0 + 3.0 * torch.randn(n, C, generator=g)
    rnd = torch.randint(0, C, (n,), generator=g)
    pat = [0, C - 1, C, C + 5, -1]
    label = torch.tensor([pat[i % 7] if i % 7 < 5 else int(rnd[i]) for i in range(n)], dtype=torch.int64)
    if all_bg:
        label = torch.full((n,), C, dtype=torch.int64)
    if n == 1:
        label[0] = 0
    score = torch.rand(n, generator=g)
    score[1::6] = 0.0
    score[2::6] = 1.0
    if C > 1:             # saturated logits beside the N(-2, 3^2) ones: on the label's class and on another one
        for i in range(n):
            v = _SAT[i % 5]
            lb = int(label[i])
            if i % 3 != 2:
                pred[i, lb if 0 <= lb < C else (i * 7) % C] = v
            pred[i, (i * 11 + 3) % C] = _SAT[(i + 2) % 5]
    coef = torch.randn(n, generator=g)
    coef[3::4] = 0.0
    return NS(name=f"qfl{n}x{C}" + ("bg" if all_bg else ""), n=n, C=C, pred=pred, label=label, score=score, coef=coef)


@functools.lru_cache(maxsize=None)
def qfl_cases():
    return [_qfl_case(n, C) for n, C in QFL_SHAPES] + [_qfl_case(5, 40, all_bg=True)]


def qfl_oracle(c, dtype):
    """(rows, dpred) of the oracle in `dtype` under autograd: dpred = d sum_i coef_i rows_i / d pred"""
    p = _leaf(c.pred, dtype)
    rows = O.quality_focal_loss(p, c.label, c.score.to(dtype))
    (rows * c.coef.to(dtype)).sum().backward()
    return rows.detach(), p.grad


def _bce(x, t):
    return x.clamp(min=0) - x * t + torch.log1p(torch.exp(-x.abs()))


def qfl_scales(c):
    """row scales in fp64.  Every element is BCE(x, t) (t - sigma)^2 with t = score on the label's class and 0 elsewhere."""
    x = c.pred.double()
    valid = (c.label >= 0) & (c.label < c.C)
    t = torch.zeros_like(x)
    idx = valid.nonzero().squeeze(1)
    t[idx, c.label[idx]] = c.score.double()[idx]
    sg = torch.sigmoid(x)
    bce_abs = x.clamp(min=0) + (x * t).abs() + torch.log1p(torch.exp(-x.abs()))
    d = (sg - t).abs()
    rows = (bce_abs * d * d).sum(1)
    # d^3 + BCE 2 d sigma (1 - sigma): `1 - sigma` is itself a difference, of magnitudes 1 and sigma (at x = 10 its fp32 value
    # has three digits left; with 1 - sigma as the magnitude that one class set E32 of the gradient to 1e-6 for every row)
    grad = c.coef.double().abs() * (d ** 3 + bce_abs * 2 * d * sg * (1 + sg)).max(1)[0]
    return rows, grad


def wave_sum(lanes):
    """erd::wave_sum: the xor butterfly over 64 lanes, [n, 64] -> [n] (lane 0)"""
    idx = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[:, idx ^ o]
    return lanes[:, 0]


def qfl_restate(c, mut=None, dtype=F32):
    """qfl_rows_kernel / qfl_bwd_kernel: lane l adds classes l, l + 64, ... in turn, then the wave's butterfly"""
    x, q, C = c.pred.to(dtype), c.score.to(dtype)[:, None], c.C
    lb = c.label.clone()
    if mut == "bg_as_last_class":
        lb[lb == C] = C - 1
    valid = (lb < C) if mut == "no_label_ge0" else ((lb >= 0) & (lb < C))
    lb = torch.where(lb < 0, lb + C, lb)                  # (what an index of -1 selects once `label >= 0` is not asked)
    M = valid[:, None] & (torch.arange(C)[None, :] == lb[:, None])
    sg = 1.0 / (1.0 + torch.exp(-x))
    d = q - sg
    bq, b0 = _bce(x, q), _bce(x, torch.zeros_like(x))
    bg = b0 * sg if mut == "bg_sigma" else b0 * sg * sg
    terms = torch.where(M, bq * d * d, bg)
    pad = (-C) % 64
    tp = F.pad(terms, (0, pad)).reshape(c.n, -1, 64)
    lanes = torch.zeros(c.n, 64, dtype=dtype)
    for trip in range(tp.shape[1]):
        lanes = lanes + tp[:, trip]
    rows = wave_sum(lanes)
    e = sg - q
    gbg = sg * sg + b0 * sg * (1 - sg) if mut == "bg_sigma" else sg * sg * sg + b0 * 2 * sg * sg * (1 - sg)
    gr = torch.where(M, e * e * e + bq * 2 * e * sg * (1 - sg), gbg)
    return rows, c.coef.to(dtype)[:, None] * gr


# ---------------------------------------------------------------------------------------------------------------------
# rows over nb bins: DFL, KD-KL, Integral
# ---------------------------------------------------------------------------------------------------------------------
BIN_SHAPES = [(1, 17), (255, 17), (257, 8), (515, 32), (3, 2)]


def _special_rows(z, nb, period, first):
    """rows that are flat, have one bin at +40, are all -80 (in turn, every `period` rows from `first`)"""
    for k, r in enumerate(range(first, z.shape[0], period)):
        if k % 3 == 0:
            z[r] = 0.75
        elif k % 3 == 1:
            z[r, (r // period) % nb] += 40.0
        else:
            z[r] = -80.0
    return z


def dfl_targets(nb):
    ts = [0.0, 1.0, float(nb - 2), nb - 1.1] + ([15.9] if nb == 17 else [])
    return sorted({t for t in ts if 0.0 <= t <= nb - 1.1 + 1e-9} | {nb - 1.1})


def _dfl_case(m, nb):
    g = _gen(2000 + 13 * m + nb)
    pred = _special_rows(1.5 * torch.randn(m, nb, generator=g), nb, 2, 1)
    ts = dfl_targets(nb)
    rnd = torch.rand(m, generator=g) * (nb - 1.1)
    k = len(ts) + 2
    target = torch.tensor([ts[i % k] if i % k < len(ts) else float(rnd[i]) for i in range(m)], dtype=F32)
    coef = torch.randn(m, generator=g)
    coef[4::5] = 0.0
    return NS(name=f"dfl{m}x{nb}", m=m, nb=nb, pred=pred, target=target, coef=coef)


@functools.lru_cache(maxsize=None)
def dfl_cases():
    return [_dfl_case(m, nb) for m, nb in BIN_SHAPES]


def dfl_oracle(c, dtype):
    p = _leaf(c.pred, dtype)
    rows = O.distribution_focal_loss(p, c.target.to(dtype))
    (rows * c.coef.to(dtype)).sum().backward()
    return rows.detach(), p.grad


def _softmax_mag(z):
    """fp64: (p, u, lse magnitude) with u_b = p_b (1 + |z_b| + |max| + log s), the magnitude a computed probability carries"""
    mx = z.max(1, keepdim=True)[0]
    s = torch.exp(z - mx).sum(1, keepdim=True)
    lmag = mx.abs() + torch.log(s)
    p = torch.exp(z - mx) / s
    return p, p * (1 + z.abs() + lmag), lmag


def dfl_scales(c):
    z, y = c.pred.double(), c.target.double()
    p, u, lmag = _softmax_mag(z)
    dl = y.long()
    dr = (dl + 1).clamp(max=c.nb - 1)
    wl, wr = (dl + 1).double() - y, y - dl.double()
    zl, zr = z.gather(1, dl[:, None])[:, 0].abs(), z.gather(1, dr[:, None])[:, 0].abs()
    rows = (lmag[:, 0] + zl) * wl + (lmag[:, 0] + zr) * wr
    tgt = torch.zeros_like(z)
    tgt.scatter_add_(1, dl[:, None], wl[:, None])
    tgt.scatter_add_(1, dr[:, None], wr[:, None])
    return rows, c.coef.double().abs() * (u + tgt).max(1)[0]


def _seq_sum(cols):
    s = torch.zeros_like(cols[:, 0])
    for b in range(cols.shape[1]):
        s = s + cols[:, b]
    return s


def dfl_restate(c, mut=None, dtype=F32):
    """dfl_kernel: max, sum of exp in bin order, lse = max + log s, p = exp(z - lse)"""
    z, y, nb = c.pred.to(dtype), c.target.to(dtype), c.nb
    mx = z.max(1)[0]
    lse = mx + torch.log(_seq_sum(torch.exp(z - mx[:, None])))
    dl = y.to(torch.int64)
    dr = dl + 1
    wl, wr = dr.to(dtype) - y, y - dl.to(dtype)
    if mut == "swap_wl_wr":
        wl, wr = wr, wl
    zl = z.gather(1, dl[:, None])[:, 0]
    zr = z.gather(1, dr.clamp(max=nb - 1)[:, None])[:, 0]
    rows = (lse - zl) * wl + (lse - zr) * wr
    b = torch.arange(nb)[None, :]
    right = dl if mut == "right_bin_dl" else dr
    p = torch.exp(z - lse[:, None])
    zero = torch.zeros((), dtype=dtype)
    gr = p * (wl + wr)[:, None] - torch.where(b == dl[:, None], wl[:, None], zero) - torch.where(b == right[:, None], wr[:, None], zero)
    return rows, c.coef.to(dtype)[:, None] * gr


def _kd_case(m, nb, T):
    g = _gen(3000 + 13 * m + nb + int(T))
    pred = 2.0 * torch.randn(m, nb, generator=g)
    soft = 2.0 * torch.randn(m, nb, generator=g)
    soft[1::6] = pred[1::6]                               # soft == pred: the row is 0 and so is its gradient
    if T == 1:
        for r in range(3, m, 6):                          # one teacher logit at +200: every other probability underflows
            soft[r, r % nb] = 200.0
    coef = torch.randn(m, generator=g)
    coef[2::5] = 0.0                                      # weight-0 rows
    return NS(name=f"kd{m}x{nb}T{T}", m=m, nb=nb, T=float(T), pred=pred, soft=soft, coef=coef)


@functools.lru_cache(maxsize=None)
def kd_cases():
    return [_kd_case(m, nb, T) for m, nb in BIN_SHAPES for T in (1, 10)]


def kd_oracle(c, dtype):
    p = _leaf(c.pred, dtype)
    rows = O.kd_kl_div(p, c.soft.to(dtype), c.T)
    (rows * c.coef.to(dtype)).sum().backward()
    return rows.detach(), p.grad


def kd_scales(c):
    """rows: T^2 / nb sum_b t_b (1 + |zt_b| + |lse_t|) (|zt_b| + |lse_t| + |zs_b| + |lse_s|): the four operands of
    log t - log p and the magnitude t_b carries; gradient: |c| T / nb max_b (u_s + u_t)"""
    zs, zt = c.pred.double() / c.T, c.soft.double() / c.T
    ps, us, ls = _softmax_mag(zs)
    pt, ut, lt = _softmax_mag(zt)
    rows = (ut * (zt.abs() + lt + zs.abs() + ls)).sum(1) / c.nb * (c.T * c.T)
    return rows, c.coef.double().abs() * c.T / c.nb * (us + ut).max(1)[0]


def kd_restate(c, mut=None, dtype=F32):
    """kdkl_kernel"""
    T, nb = torch.tensor(c.T, dtype=dtype), c.nb
    zs, zt = c.pred.to(dtype) / T, c.soft.to(dtype) / T
    ms, mt = zs.max(1)[0], zt.max(1)[0]
    lses = ms + torch.log(_seq_sum(torch.exp(zs - ms[:, None])))
    lset = mt + torch.log(_seq_sum(torch.exp(zt - mt[:, None])))
    lt = zt - lset[:, None]
    t = torch.exp(lt)
    ls = zs - lses[:, None]
    if mut == "t_log_t":
        terms = t * (torch.log(t) - ls)
    else:
        terms = torch.where(t > 0, t * (lt - ls), torch.zeros((), dtype=dtype))
    acc = _seq_sum(terms)
    coef = c.coef.to(dtype)
    if mut == "T_not_T2":
        rows, cc = acc / nb * T, coef / nb
    elif mut == "sum_not_mean":
        rows, cc = acc * (T * T), coef * T
    else:
        rows, cc = acc / nb * (T * T), coef * T / nb
    return rows, cc[:, None] * (torch.exp(ls) - torch.exp(lt))


INTEGRAL_SHAPES = [(4, 17), (1028, 17), (257, 8), (5, 32)]


def _integral_case(m, nb):
    g = _gen(4000 + 13 * m + nb)
    x = 1.5 * torch.randn(m, nb, generator=g)
    x[1::4] = 0.75                  # flat
    x[2::4, 0] += 40.0              # peaked at bin 0
    x[3::4, nb - 1] += 40.0         # peaked at the last bin
    dy = torch.randn(m, generator=g)
    dy[5::7] = 0.0
    return NS(name=f"integral{m}x{nb}", m=m, nb=nb, x=x, dy=dy)


@functools.lru_cache(maxsize=None)
def integral_cases():
    return [_integral_case(m, nb) for m, nb in INTEGRAL_SHAPES]


def integral_oracle(c, dtype):
    """O.integral returns [n, 4] of 4 n rows: four copies of the rows, read back as the first m values"""
    x = _leaf(c.x, dtype)
    y = O.integral(torch.cat([x] * 4, 0), c.nb - 1).reshape(-1)[:c.m]
    (y * c.dy.to(dtype)).sum().backward()
    return y.detach(), x.grad


def integral_scales(c):
    z = c.x.double()
    p, u, _ = _softmax_mag(z)
    b = torch.arange(c.nb, dtype=F64)[None, :]
    e = (p * b).sum(1, keepdim=True)
    return (u * b).sum(1), c.dy.double().abs() * (u * (b + e)).max(1)[0]


def integral_restate(c, mut=None, dtype=F32):
    """integral_kernel: exp(z - max), sum in bin order, times 1 / s, expectation in bin order"""
    x, nb = c.x.to(dtype), c.nb
    z = torch.exp(x - x.max(1, keepdim=True)[0])
    z = z * (1.0 / _seq_sum(z))[:, None]
    b = torch.arange(nb, dtype=dtype)[None, :]
    e = _seq_sum(z * b)
    k = b if mut == "b_not_b_minus_e" else b - e[:, None]
    return e, z * k * c.dy.to(dtype)[:, None]


# ---------------------------------------------------------------------------------------------------------------------
# boxes
# ---------------------------------------------------------------------------------------------------------------------
BOX_EPS = 1e-6
_A = (10., 20., 50., 80.)
BOX_FAMILY = [          # (pred, target, what)
    (_A, _A, "identical: a tie on every coordinate"),
    (_A, (10., 30., 60., 90.), "shared edge: tie on x1"),
    (_A, (5., 20., 40., 70.), "shared edge: tie on y1"),
    (_A, (20., 30., 50., 90.), "shared edge: tie on x2"),
    (_A, (0., 10., 40., 80.), "shared edge: tie on y2"),
    (_A, (50., 30., 90., 70.), "touching in x: w == 0, h > 0"),
    (_A, (20., 80., 60., 120.), "touching in y: h == 0, w > 0"),
    (_A, (100., 200., 150., 260.), "disjoint"),
    ((100., 200., 150., 260.), _A, "disjoint, the other way"),
    ((20., 30., 40., 50.), _A, "contained in the target"),
    (_A, (20., 30., 40., 50.), "contains the target"),
    ((30., 40., 30., 40.), (30., 40., 30., 40.), "zero-area point equal to the target: union < eps"),
    ((30., 40., 30., 40.), _A, "zero-area point inside the target"),
    ((30., 40., 30., 60.), _A, "zero-width line inside the target"),
    ((50., 20., 10., 80.), _A, "inverted: x2 < x1, union <= eps"),
    ((50., 20., 30., 80.), (10., 20., 60., 80.), "inverted: x2 < x1, union > eps"),
    (_A, (30., 40., 70., 100.), "plain overlap"),
]


def family_boxes(n, affine=False):
    """the family tiled to length n; `affine`: every second pass through the family mapped by x -> 1.5 x + 0.25 (both boxes
    alike, so ties stay ties; exact in fp32, so the inverted box whose union is 0 keeps it: a union that is the rounding residue
    of two areas of +-2400 has no digits to compare in any precision; the coordinates are no integers)"""
    L = len(BOX_FAMILY)
    a = torch.tensor([BOX_FAMILY[i % L][0] for i in range(n)], dtype=F32).reshape(n, 4)
    b = torch.tensor([BOX_FAMILY[i % L][1] for i in range(n)], dtype=F32).reshape(n, 4)
    if affine and n:
        odd = ((torch.arange(n) // L) % 2 == 1)[:, None]
        a = torch.where(odd, a * 1.5 + 0.25, a)
        b = torch.where(odd, b * 1.5 + 0.25, b)
    return a, b


def random_boxes(n, seed, w=1333.0, h=800.0):
    """random xyxy boxes at image scale; half of the targets are the prediction moved by a few pixels"""
    g = _gen(seed)
    def boxes():
        c = torch.rand(n, 2, generator=g) * torch.tensor([w, h])
        s = 8.0 + torch.rand(n, 2, generator=g) * torch.tensor([w / 3, h / 3])
        return torch.cat([c - s / 2, c + s / 2], 1)
    a, b = boxes(), boxes()
    near = a + 6.0 * torch.randn(n, 4, generator=g)
    b[0::2] = near[0::2]
    return a, b


def _giou_case(n, kind):
    a, b = family_boxes(n, affine=True) if kind == "family" else random_boxes(n, 5000 + n)
    coef = torch.randn(n, generator=_gen(5100 + n))
    coef[6::9] = 0.0
    return NS(name=f"giou_{kind}{n}", n=n, pred=a, target=b, coef=coef, eps=BOX_EPS)


@functools.lru_cache(maxsize=None)
def giou_cases():
    return [_giou_case(n, "family") for n in (1, 255, 257)] + [_giou_case(300, "random")]


def giou_oracle(c, dtype):
    p = _leaf(c.pred, dtype)
    rows = 1 - O.bbox_overlaps(p, c.target.to(dtype), mode="giou", is_aligned=True, eps=c.eps)
    (rows * c.coef.to(dtype)).sum().backward()
    return rows.detach(), p.grad


def overlaps_restate(b1, b2, mode="iou", aligned=False, eps=BOX_EPS):
    """overlaps_kernel's arithmetic in its order (fp32 in, fp32 out): bit-equal to the kernel"""
    m, n = b1.shape[0], b2.shape[0]
    if not aligned:
        b1, b2 = b1[:, None, :], b2[None, :, :]
    e = torch.tensor(eps, dtype=b1.dtype)
    zero = torch.zeros((), dtype=b1.dtype)
    a1 = (b1[..., 2] - b1[..., 0]) * (b1[..., 3] - b1[..., 1])
    a2 = (b2[..., 2] - b2[..., 0]) * (b2[..., 3] - b2[..., 1])
    w = torch.maximum(torch.minimum(b1[..., 2], b2[..., 2]) - torch.maximum(b1[..., 0], b2[..., 0]), zero)
    h = torch.maximum(torch.minimum(b1[..., 3], b2[..., 3]) - torch.maximum(b1[..., 1], b2[..., 1]), zero)
    ov = w * h
    uni = torch.maximum(a1 + a2 - ov, e)
    iou = ov / uni
    if mode == "iou":
        return iou.reshape((m,) if aligned else (m, n))
    ew = torch.maximum(torch.maximum(b1[..., 2], b2[..., 2]) - torch.minimum(b1[..., 0], b2[..., 0]), zero)
    eh = torch.maximum(torch.maximum(b1[..., 3], b2[..., 3]) - torch.minimum(b1[..., 1], b2[..., 1]), zero)
    enc = torch.maximum(ew * eh, e)
    return (iou - (enc - uni) / enc).reshape((m,) if aligned else (m, n))


def giou_restate(c, mut=None, dtype=F32):
    """giou_kernel: rows, gradient by its hand-written rules, and the gradient's row scale (the magnitudes of the four terms
    it adds, with d(union) = d(area) - d(overlap) counted as |d(area)| + |d(overlap)|; meaningful at dtype float64)"""
    a, b = c.pred.to(dtype), c.target.to(dtype)
    eps = torch.tensor(c.eps, dtype=dtype)
    zero, one, half = (torch.tensor(v, dtype=dtype) for v in (0.0, 1.0, 0.5))
    ax, ay, az, aw = a.unbind(1)
    bx, by, bz, bw = b.unbind(1)
    area1, area2 = (az - ax) * (aw - ay), (bz - bx) * (bw - by)
    ltx, lty, rbx, rby = torch.maximum(ax, bx), torch.maximum(ay, by), torch.minimum(az, bz), torch.minimum(aw, bw)
    w, h = torch.maximum(rbx - ltx, zero), torch.maximum(rby - lty, zero)
    ov = w * h
    uni_raw = area1 + area2 - ov
    uni = torch.maximum(uni_raw, eps)
    iou = ov / uni
    ex1, ey1, ex2, ey2 = torch.minimum(ax, bx), torch.minimum(ay, by), torch.maximum(az, bz), torch.maximum(aw, bw)
    ew, eh = torch.maximum(ex2 - ex1, zero), torch.maximum(ey2 - ey1, zero)
    enc_raw = ew * eh
    enc = torch.maximum(enc_raw, eps)
    rows = 1 - (iou - (enc - uni) / enc)
    tie = one if mut == "ties_1_0" else half          # (1/0: the whole gradient to the first operand)

    def gmax(x, y):
        return torch.where(x > y, one, torch.where(x == y, tie, zero))

    def gmin(x, y):
        return torch.where(x < y, one, torch.where(x == y, tie, zero))

    def passes(v):
        return torch.where((v > 0) if mut == "clamp_gt" else (v >= 0), one, zero)

    pw, ph = passes(rbx - ltx), passes(rby - lty)
    d_ov = [-gmax(ax, bx) * pw * h, -gmax(ay, by) * ph * w, gmin(az, bz) * pw * h, gmin(aw, bw) * ph * w]
    d_a1 = [-(aw - ay), -(az - ax), (aw - ay), (az - ax)]
    qw, qh = passes(ex2 - ex1), passes(ey2 - ey1)
    gate = enc_raw > eps
    d_enc = [torch.where(gate, v, zero) for v in
             (-gmin(ax, bx) * qw * eh, -gmin(ay, by) * qh * ew, gmax(az, bz) * qw * eh, gmax(aw, bw) * qh * ew)]
    cf = c.coef.to(dtype)
    g, mag = [], []
    for q in range(4):
        d_uni = torch.where(uni_raw > eps, d_a1[q] - d_ov[q], zero)
        m_uni = torch.where(uni_raw > eps, d_a1[q].abs() + d_ov[q].abs(), zero)
        t_enc = zero * d_uni if mut == "no_enclose_term" else uni / (enc * enc) * d_enc[q]
        g.append(cf * (-d_ov[q] / uni + ov / (uni * uni) * d_uni - d_uni / enc + t_enc))
        # (the reference's autograd adds the enclosing-area term as d_enc / enc - (enc - uni) / enc^2 d_enc: both magnitudes)
        mag.append(d_ov[q].abs() / uni + ov / (uni * uni) * m_uni + m_uni / enc
                   + (1 / enc + (enc - uni).abs() / (enc * enc)) * d_enc[q].abs())
    return rows, torch.stack(g, 1), cf.abs() * torch.stack(mag, 1).max(1)[0]


PAIR_SHAPES = [(0, 8), (8, 0), (1, 1), (17, 31), (300, 3)]


def pair_boxes(m, n):
    """[m, 4] x [n, 4] from the family: the predictions against the targets, the second list started elsewhere"""
    a = family_boxes(m, affine=True)[0]
    b = family_boxes(n + 5, affine=True)[1][5:] if (m, n) != (1, 1) else family_boxes(1)[1]
    return a, b.reshape(n, 4)


# ---------------------------------------------------------------------------------------------------------------------
# coder
# ---------------------------------------------------------------------------------------------------------------------
MAX_SHAPE = (40, 60)
CODER_N = (0, 1, 257)
B2D_PARAMS = [(None, 0.1), (16.0, 0.1), (8.0, 0.1), (7.5, 0.01)]


def d2b_case(n):
    """points and distances whose decoded coordinates are, in turn: exactly 0, exactly on the border, outside below, outside
    above, inside ((H, W) = MAX_SHAPE); all values are multiples of 1/2, so the decode is exact"""
    g = _gen(6000 + n)
    H, W = MAX_SHAPE
    pts = torch.stack([torch.randint(0, 2 * W + 1, (n,), generator=g) / 2.0, torch.randint(0, 2 * H + 1, (n,), generator=g) / 2.0], 1)
    i = torch.arange(n)
    x1 = torch.tensor([0.0, W, -3.0, W + 5.0, 12.5])[i % 5]
    y1 = torch.tensor([7.5, 0.0, H, -0.5, H + 2.0, 3.0])[i % 6]
    x2 = torch.tensor([W, 20.0, W + 0.5, 0.0, -1.0, 33.0, W])[i % 7]
    y2 = torch.tensor([H, 0.0, 11.0, H + 9.0, -2.5])[i % 5]
    dist = torch.stack([pts[:, 0] - x1, pts[:, 1] - y1, x2 - pts[:, 0], y2 - pts[:, 1]], 1)
    dout = torch.randn(n, 4, generator=g)
    return NS(name=f"d2b{n}", n=n, pts=pts.reshape(n, 2), dist=dist.reshape(n, 4), dout=dout, want=torch.stack([x1, y1, x2, y2], 1).reshape(n, 4))


def d2b_oracle(c, max_shape, dtype, mut=None):
    """O.distance2bbox plus the reference's clamp (transforms.py:176-181: x to [0, W], y to [0, H], after the decode), and the
    gradient w.r.t. the distances under `dout`.  torch's clamp passes the gradient at equality with a bound."""
    d = _leaf(c.dist, dtype)
    box = O.distance2bbox(c.pts.to(dtype), d)
    if max_shape is not None:
        H, W = max_shape
        raw = box
        box = torch.stack([raw[:, 0].clamp(min=0, max=W), raw[:, 1].clamp(min=0, max=H),
                           raw[:, 2].clamp(min=0, max=W), raw[:, 3].clamp(min=0, max=H)], 1)
    (box * c.dout.to(dtype)).sum().backward()
    grad = d.grad if d.grad is not None else torch.zeros_like(d.detach())
    if mut == "zero_at_border" and max_shape is not None:
        lim = torch.tensor([W, H, W, H], dtype=dtype)
        grad = torch.where((raw.detach() <= 0) | (raw.detach() >= lim), torch.zeros((), dtype=dtype), grad)
    return box.detach(), grad


def b2d_case(n, max_dis, eps):
    """boxes whose distances are, in turn: 0, negative, inside, exactly at the bound fl32(max_dis - eps) (from a point at 0, so
    that the difference is exact), beyond it"""
    g = _gen(6100 + n)
    hi = b2d_bound(max_dis, eps) if max_dis is not None else 9.25
    i = torch.arange(n)
    pts = torch.randint(0, 81, (n, 2), generator=g) / 2.0
    pts[i % 5 == 3] = 0.0
    want = torch.stack([torch.tensor([0.0, -2.5, 3.25, hi, hi + 4.0])[(i + k) % 5] for k in (0, 1, 2, 3)], 1).reshape(n, 4)
    want[i % 5 == 3] = torch.tensor([hi, hi, hi + 1.0, 0.5])
    box = torch.stack([pts[:, 0] - want[:, 0], pts[:, 1] - want[:, 1], pts[:, 0] + want[:, 2], pts[:, 1] + want[:, 3]], 1)
    return NS(name=f"b2d{n}_{max_dis}", n=n, pts=pts.reshape(n, 2), box=box.reshape(n, 4), max_dis=max_dis, eps=eps, hi=hi)


def b2d_bound(max_dis, eps):
    """the kernel's upper bound: max_dis - eps in fp32 arithmetic"""
    return float(torch.tensor(max_dis, dtype=F32) - torch.tensor(eps, dtype=F32))


def b2d_oracle(c, dtype):
    if c.max_dis is None:            # transforms.py:221-230: no clamp without max_dis
        p, b = c.pts.to(dtype), c.box.to(dtype)
        return torch.stack([p[:, 0] - b[:, 0], p[:, 1] - b[:, 1], b[:, 2] - p[:, 0], b[:, 3] - p[:, 1]], -1)
    return O.bbox2distance(c.pts.to(dtype), c.box.to(dtype), c.max_dis, c.eps)


# ---------------------------------------------------------------------------------------------------------------------
# reductions (losses/utils.py:30-65) and the small kernels
# ---------------------------------------------------------------------------------------------------------------------
def reduce_ref(rows, weight, reduction, avg_factor, loss_weight=1.0):
    """loss_weight * weight_reduce_loss(rows, weight, reduction, avg_factor) in the reference's order, any dtype"""
    loss = rows if weight is None else rows * weight
    if avg_factor is None:
        if reduction == "mean":
            loss = O.weight_reduce(rows, weight, None)
        elif reduction == "sum":
            loss = loss.sum()
    elif reduction == "mean":
        loss = O.weight_reduce(rows, weight, avg_factor)
    elif reduction != "none":
        raise ValueError('avg_factor can not be used with reduction="sum"')
    return loss_weight * loss


def reduce_scale(reduction, avg_factor, n, loss_weight=1.0):
    """the factor of the weighted row sum (None: reduction='none')"""
    if reduction == "none":
        return None
    if reduction == "sum":
        return loss_weight
    return loss_weight / n if avg_factor is None else loss_weight / (avg_factor + EPS32)


WSUM_N = (0, 1, 63, 64, 1023, 1024, 1025, 5000)
SMALL_N = (0, 1, 255, 256, 257)


def wsum_case(n, weighted):
    """small integers and a power-of-two scale: the f64 sum is exact in any order, the fp32 result has one right value"""
    g = _gen(7000 + n)
    rows = torch.randint(-8, 9, (n,), generator=g).float()
    w = torch.randint(0, 4, (n,), generator=g).float() if weighted else None
    scale = 0.125
    want = float((rows.double() * (w.double() if weighted else 1.0)).sum()) * scale
    assert want == float(torch.tensor(want, dtype=F32))
    return NS(n=n, rows=rows, weight=w, scale=scale, want=want)


def wsum_real_case(n=5000, avg_factor=37.0):
    g = _gen(7100 + n)
    rows, w = torch.rand(n, generator=g) * 3.0, torch.rand(n, generator=g)
    scale = 1.0 / (avg_factor + EPS32)
    return NS(n=n, rows=rows, weight=w, scale=scale, want=float((rows.double() * w.double()).sum()) * scale)


def wsum_restate(c, mut=None):
    """wsum_kernel: products and sum in f64, times scale, rounded to fp32 once"""
    w = c.weight.double() if (c.weight is not None and mut != "weight_ignored") else 1.0
    return torch.tensor(float((c.rows.double() * w).sum()) * c.scale, dtype=F64).to(F32)


def small_case(n, weighted, seed=7200):
    g = _gen(seed + n)
    return NS(n=n, rows=torch.randn(n, generator=g), weight=torch.rand(n, generator=g) if weighted else None,
              scale=float(torch.tensor(0.3 / 37.0, dtype=F32)), upstream=torch.tensor([1.7], dtype=F32))


def rows_mul_restate(c):
    v = c.rows * torch.tensor(c.scale, dtype=F32)
    return v if c.weight is None else v * c.weight


def loss_coef_restate(c):
    v = (c.upstream * torch.tensor(c.scale, dtype=F32)).expand(c.n)
    return v.clone() if c.weight is None else v * c.weight


ATSS_A = (1, 255, 257)
ATSS_GT_LABELS = (7, 0, 39, 79, 3)


def atss_case(A):
    """hand-written (IoU bits << 32 | 0xffffffff - gt) keys: unassigned (0), gt 0, gt G - 1, one in between"""
    G = len(ATSS_GT_LABELS)
    pat = [(0.9, 0), None, (0.25, G - 1), (1.0, 2), None, (0.5, 0), (1e-3, G - 1)]
    keys, gt_inds, ov, labels = [], [], [], []
    for a in range(A):
        e = pat[a % len(pat)]
        if e is None:
            keys.append(0); gt_inds.append(0); ov.append(-100000000.0); labels.append(-1)
        else:
            iou = torch.tensor(e[0], dtype=F32)
            bits = int(iou.view(torch.int32)) & 0xffffffff
            k = (bits << 32) | (0xffffffff - e[1])
            keys.append(k - (1 << 64) if k >= (1 << 63) else k)
            gt_inds.append(e[1] + 1); ov.append(float(iou)); labels.append(ATSS_GT_LABELS[e[1]])
    return NS(A=A, keys=torch.tensor(keys, dtype=torch.int64), gt_labels=torch.tensor(ATSS_GT_LABELS, dtype=torch.int64),
              gt_inds=torch.tensor(gt_inds, dtype=torch.int64), max_ov=torch.tensor(ov, dtype=F32),
              labels=torch.tensor(labels, dtype=torch.int64))


# ---------------------------------------------------------------------------------------------------------------------
# the 4x rule: one table of the operators under it
# ---------------------------------------------------------------------------------------------------------------------
def _giou_scales(c):
    """rows are under the equality rule; the scale given for them (the magnitudes 1 - iou + (enc - union) / enc adds) only
    serves the modules' reduced values"""
    rows64, _, gscale = giou_restate(c, dtype=F64)
    return 3.0 + 0 * rows64, gscale


RULE_OPS = {
    # name: (cases, oracle(case, dtype) -> (rows, grad), scales(case) -> (rows, grad), restate(case, mut) -> (rows, grad, ...))
    "qfl": (qfl_cases, qfl_oracle, qfl_scales, qfl_restate),
    "dfl": (dfl_cases, dfl_oracle, dfl_scales, dfl_restate),
    "kd": (kd_cases, kd_oracle, kd_scales, kd_restate),
    "integral": (integral_cases, integral_oracle, integral_scales, integral_restate),
    "giou": (giou_cases, giou_oracle, _giou_scales, giou_restate),
}

MUTATIONS = {
    "qfl": ["bg_sigma", "bg_as_last_class", "no_label_ge0"],
    "dfl": ["swap_wl_wr", "right_bin_dl"],
    "kd": ["T_not_T2", "sum_not_mean", "t_log_t"],
    "giou": ["ties_1_0", "clamp_gt", "no_enclose_term"],
    "integral": ["b_not_b_minus_e"],
}


@functools.lru_cache(maxsize=None)
def ref64(op):
    """[(case, rows64, grad64, rows scale, grad scale)]: computed once, shared, left unchanged"""
    cases, oracle, scales, _ = RULE_OPS[op]
    out = []
    for c in cases():
        rows, grad = oracle(c, F64)
        rs, gs = scales(c)
        out.append((c, rows, grad, rs, gs))
    return out


@functools.lru_cache(maxsize=None)
def e32(op):
    """(E32 of the rows, E32 of the gradient): the fp32 yardstick (the oracle in float32 on the CPU) against ref64"""
    oracle = RULE_OPS[op][1]
    er, eg = [], []
    for c, rows, grad, rs, gs in ref64(op):
        r32, g32 = oracle(c, F32)
        er.append(nerr(r32, rows, rs))
        eg.append(nerr(g32, grad, gs))
    return worst(er), worst(eg)


def figures(op, fn):
    """worst row-normalised errors (rows, gradient) of fn(case) -> (rows or None, grad or None, ...) against ref64"""
    er, eg = [], []
    for c, rows, grad, rs, gs in ref64(op):
        got = fn(c)
        if got[0] is not None:
            er.append(nerr(got[0], rows, rs))
        if got[1] is not None:
            eg.append(nerr(got[1], grad, gs))
    return worst(er), worst(eg)
