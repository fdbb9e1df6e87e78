"""Plain torch-CPU references, inputs and case tables of the three Winograd F(2x2,3x3) kernels of winograd.hip (wino_conv_kernel,
wino_x3_kernel, wino_x3p_kernel) and of the GroupNorm statistics that wino_x3p_kernel's output stage accumulates (gn_part,
wino_gn_finalize_kernel), for tests/test_gpu_wino_exact.py to run and tests/test_wino_refs_cpu.py to reason about.  No GPU and no
project kernel is touched here.

With x in {-1, 0, 1} and weights in {-4, 0, 4}, U = G g G^T and V = B^T d B are small integers (one bf16 limb holds them; the other
two limbs are zero), every product and every fp32 sum of the 16 transform-domain GEMMs, of the output transform, of the epilogues
(scales in {0.5, 1, 2, -1}, integer shifts and residuals), of the column sums and of the per-item GroupNorm sums is an integer or
half-integer far below 2^24 -- exact in any order.  So the kernels must reproduce the fp64 convolution at every element, and
mean_rstd is one fp64 formula on the same numbers on both sides.  test_wino_refs_cpu.py asserts those conditions on the references.

`cover` restates wino_plan's cover of a map by block regions (interior 4x8-tile blocks, a bottom strip, a right strip), `stored`
what each block of a region stores (wino_decode's y0 / x0 / yl / xl)."""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F

import reduce_refs as R

BN, BNP = 64, 128                 # output channels per item: wino_conv_kernel / wino_x3_kernel, wino_x3p_kernel
MAX_SEG = R.MAX_SEG
GN_PART_FLOATS = 32               # floats per item in gn_part: 16 groups x (sum, sum of squares)
ITEM_PIXELS = 128                 # a block is 32 tiles of 2x2 pixels


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------
# wino_plan's cover, restated
# ---------------------------------------------------------------------------------------------
def cover(H, W):
    """the block regions of an H x W map, in wino_plan's order.  Each: kind, first tile (ty0, tx0), nby x nbx blocks of
    (32 >> code) x (1 << code) tiles (code = add_region's lbw: 1 = 16x2, 2 = 8x4, 3 = 4x8, 4 = 2x16), and the tile (ty1, tx1) at or
    beyond which the block's tiles belong to another region"""
    TH, TW = (H + 1) // 2, (W + 1) // 2
    out = []

    def add(kind, ty0, tx0, nby, nbx, code, ty1, tx1):
        if nby > 0 and nbx > 0:
            out.append(dict(kind=kind, ty0=ty0, tx0=tx0, nby=nby, nbx=nbx, code=code, ty1=ty1, tx1=tx1))
    nby, nbx = TH // 4, TW // 8
    add("interior", 0, 0, nby, nbx, 3, 4 * nby, 8 * nbx)
    rb = TH - 4 * nby
    if rb > 0:
        bh = 2 if rb <= 2 else 4
        bw = 32 // bh
        add("bottom", 4 * nby, 0, 1, cdiv(TW, bw), 4 if bw == 16 else 3, TH, TW)
    cbw = TW - 8 * nbx
    if cbw > 0 and nby > 0:
        bw = 2 if cbw <= 2 else 4 if cbw <= 4 else 8
        bh = 32 // bw
        add("right", 0, 8 * nbx, cdiv(4 * nby, bh), 1, {2: 1, 4: 2, 8: 3}[bw], 4 * nby, TW)
    return out


def blocks_per_image(H, W):
    return sum(r["nby"] * r["nbx"] for r in cover(H, W))


def items_per_image(H, W, Cout, couts_per_item):
    """64 per item: the last item may be partly empty; 128 per item: only where Cout % 128 == 0"""
    assert couts_per_item == BN or Cout % BNP == 0
    return blocks_per_image(H, W) * cdiv(Cout, couts_per_item)


def list_blocks(sizes, N):
    """WinoDesc::blocks_per_nb of a launch: what erd_wino_x3_gn_ws_bytes / (32 * 4 * (Cout / 128)) reports"""
    return N * sum(blocks_per_image(h, w) for h, w in sizes)


def region_block0(sizes, N):
    """block0 of every region of a launch, in order: [(level, kind, block0)]"""
    out, b = [], 0
    for lvl, (h, w) in enumerate(sizes):
        for r in cover(h, w):
            out.append((lvl, r["kind"], b))
            b += N * r["nby"] * r["nbx"]
    return out


def stored(H, W):
    """per block of every region: (code, y0, y1, x0, x1), the pixel rectangle [y0, y1) x [x0, x1) it stores (possibly empty)"""
    out = []
    for r in cover(H, W):
        bh, bw = 32 >> r["code"], 1 << r["code"]
        yl, xl = min(H, 2 * r["ty1"]), min(W, 2 * r["tx1"])
        for by in range(r["nby"]):
            for bx in range(r["nbx"]):
                y0, x0 = 2 * (r["ty0"] + by * bh), 2 * (r["tx0"] + bx * bw)
                out.append((r["code"], y0, max(y0, min(y0 + 2 * bh, yl)), x0, max(x0, min(x0 + 2 * bw, xl))))
    return out


def census_key(H, W):
    """(TH % 4, TW % 8, interior rows > 0, interior columns > 0)"""
    TH, TW = (H + 1) // 2, (W + 1) // 2
    return TH % 4, TW % 8, TH // 4 > 0, TW // 8 > 0


# ---------------------------------------------------------------------------------------------
# the shape sweep
# ---------------------------------------------------------------------------------------------
SWEEP_H, SWEEP_W = 18, 34
SWEEP_LISTS_PER_H = 7
SWEEP_N = 2


def sweep_lists(H0):
    """the seven level lists of sweep row H0 (1..18): list k holds the widths k + 1, k + 8, ... <= 34 and level j the height
    1 + (H0 - 1 + 4 j) mod 18, so a launch mixes heights, widths and strip shapes -- over H0 = 1..18 every (H, W) occurs once"""
    out = []
    for k in range(SWEEP_LISTS_PER_H):
        ws = list(range(k + 1, SWEEP_W + 1, 7))
        out.append([(1 + (H0 - 1 + 4 * j) % SWEEP_H, w) for j, w in enumerate(ws)])
    return out


def fpn_sizes(h, w):
    """the five head levels (strides 8 .. 128) of a padded h x w batch"""
    out = [(cdiv(h, 8), cdiv(w, 8))]
    while len(out) < 5:
        out.append((cdiv(out[-1][0], 2), cdiv(out[-1][1], 2)))
    return out


# padded batch sizes RandomResize between (1333, 480) and (1333, 800) produces: both ends of the range and three between them
MS_BATCHES = [(480, 640), (544, 736), (608, 1024), (704, 1184), (800, 1344)]
MS_LISTS = [fpn_sizes(h, w) for h, w in MS_BATCHES]
CIN256_LIST = [(18, 34), (13, 21), (7, 11), (4, 5), (1, 2)]       # the one list of the forms test at Cin = 256
RAGGED_COUTS = (80, 68, 70)
GN_COUT = 256


# ---------------------------------------------------------------------------------------------
# integer inputs (numpy PCG64: the same bits on every machine)
# ---------------------------------------------------------------------------------------------
W_MAG, RES_MAX, SHIFT_MAX = 4, 8, 3
BN_SCALES = (0.5, 1.0, 2.0, -1.0)


def int_x(seed, N, A, Cin):
    return R.ints(seed, -1, 1, N, A, Cin)


def int_w(seed, Cout, Cin):
    """[Cout, 3, 3, Cin] (OHWI): +-4 with probability 2 / Cin, else 0"""
    g = R._rng(seed)
    hit = g.random((Cout, 3, 3, Cin)) < 2.0 / Cin
    sign = g.integers(0, 2, size=hit.shape) * 2 - 1
    return torch.from_numpy((W_MAG * hit * sign).astype(np.float32))


def bn_scale_shift(seed, Cout):
    ch = torch.arange(Cout)
    return torch.tensor(BN_SCALES)[(ch * 3 + ch // 8) % 4], R.ints(seed, -SHIFT_MAX, SHIFT_MAX, Cout)


def residual_mask(seed, N, A, Cout):
    return R.ints(seed, -RES_MAX, RES_MAX, N, A, Cout), R.ints(seed + 1, 0, 1, N, A, Cout) * 2 - 1


# ---------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------
def _levels_nchw(t, sizes):
    return [t[:, sl].reshape(t.shape[0], h, w, t.shape[2]).permute(0, 3, 1, 2) for sl, (h, w) in zip(R.level_slices(sizes), sizes)]


def _cat(levels):
    return torch.cat([t.permute(0, 2, 3, 1).reshape(t.shape[0], -1, t.shape[1]) for t in levels], 1)


def conv_ref(x_cat, w_ohwi, sizes):
    """fp64 conv3x3 stride 1 pad 1 per level of a level-concatenated [N, A, Cin] buffer -> [N, A, Cout] fp64"""
    w = w_ohwi.permute(0, 3, 1, 2).double()
    return _cat([F.conv2d(xl.double(), w, None, 1, 1) for xl in _levels_nchw(x_cat, sizes)])


def dgrad_ref(dy_cat, w_ohwi, sizes):
    """the input gradient of conv_ref under dy [N, A, Cout] -> [N, A, Cin] fp64, by autograd"""
    w = w_ohwi.permute(0, 3, 1, 2).double()
    out = []
    for dyl in _levels_nchw(dy_cat, sizes):
        x = torch.zeros((dyl.shape[0], w.shape[1]) + tuple(dyl.shape[2:]), dtype=torch.float64, requires_grad=True)
        out.append(torch.autograd.grad(F.conv2d(x, w, None, 1, 1), x, dyl.double())[0])
    return _cat(out)


def exact_f32(t64):
    t32 = t64.float()
    assert torch.equal(t32.double(), t64)
    return t32


# Winograd F(2x2, 3x3) transform matrices
G_MAT = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]], dtype=torch.float64)
BT_MAT = torch.tensor([[1.0, 0.0, -1.0, 0.0], [0.0, 1.0, 1.0, 0.0], [0.0, -1.0, 1.0, 0.0], [0.0, 1.0, 0.0, -1.0]], dtype=torch.float64)


def wino_U(w_ohwi):
    """G g G^T of every (cout, cin): [Cout, Cin, 4, 4] fp64"""
    g = w_ohwi.permute(0, 3, 1, 2).double()
    return torch.einsum("ij,ocjk,lk->ocil", G_MAT, g, G_MAT)


def wino_V(x_cat, sizes):
    """B^T d B of every 4x4 input patch (2x2-pixel tiles, zero padding) of every level: list of [N, Cin, tiles, 4, 4] fp64"""
    out = []
    for xl in _levels_nchw(x_cat, sizes):
        N, Cc, H, W = xl.shape
        TH, TW = (H + 1) // 2, (W + 1) // 2
        xp = F.pad(xl.double(), (1, 2 * TW + 1 - W, 1, 2 * TH + 1 - H))
        d = xp.unfold(2, 4, 2).unfold(3, 4, 2).reshape(N, Cc, TH * TW, 4, 4)
        out.append(torch.einsum("ij,nctjk,lk->nctil", BT_MAT, d, BT_MAT))
    return out


# ---------------------------------------------------------------------------------------------
# cases: the data of one launch, computed once per process and shared by the tests that need it
# ---------------------------------------------------------------------------------------------
def forms_cases(H0):
    """[(sizes, N, Cin)] of sweep row H0 for the all-kernels / all-forms test (Cout = 128); row 1 also carries the list at
    Cin = 256 and the five multi-scale lists (N = 1)"""
    out = [(s, SWEEP_N, 64) for s in sweep_lists(H0)]
    if H0 == 1:
        out += [(CIN256_LIST, SWEEP_N, 256)]
    if 2 <= H0 <= 1 + len(MS_LISTS):
        out += [(MS_LISTS[H0 - 2], 1, 64)]
    return out


def gn_cases(H0):
    """[(sizes, N, Cin)] of sweep row H0 for the fused-statistics test (Cout = 256): every list at (Cin 64, N 3) and (Cin 256, N 1),
    one list of the row at the two other combinations"""
    lists = sweep_lists(H0)
    out = [(s, 3, 64) for s in lists] + [(s, 1, 256) for s in lists]
    k = H0 % SWEEP_LISTS_PER_H
    return out + [(lists[k], 1, 64), (lists[k], 3, 256)]


# the multi-scale lists of the fused-statistics test: Cin = 64 at both N, Cin = 256 on the smallest batch
GN_MS_CASES = [(MS_LISTS[2], 3, 64), (MS_LISTS[1], 1, 64), (MS_LISTS[3], 1, 64), (MS_LISTS[0], 1, 256), (MS_LISTS[0], 3, 256)]
GN_STALE_SMALL = [(2, 2), (2, 3), (1, 17)]       # run behind each of them on the workspace it leaves: three items per image


def _seed(sizes, N, Cin, Cout):
    s = 7 * N + 13 * Cin + Cout
    for h, w in sizes:
        s = (s * 131 + 37 * h + w) % 1000003
    return 100000 + 10 * s


@functools.lru_cache(maxsize=12)
def _conv_case(sizes, N, Cin, Cout):
    A = R.total_rows(sizes)
    seed = _seed(sizes, N, Cin, Cout)
    x, w = int_x(seed, N, A, Cin), int_w(seed + 1, Cout, Cin)
    return dict(sizes=list(sizes), N=N, Cin=Cin, Cout=Cout, A=A, seed=seed, x=x, w=w, c=exact_f32(conv_ref(x, w, sizes)))


def conv_case(sizes, N, Cin, Cout):
    """x [N, A, Cin], w [Cout, 3, 3, Cin] and c = the integer convolution [N, A, Cout] as fp32 (checked exact).  Do not modify."""
    return _conv_case(tuple(sizes), N, Cin, Cout)


def forms_refs(case):
    """the expected results of forms (b), (c) -- with the mask and without --, (d) of the forms test, and their inputs"""
    N, A, Cin, Cout, seed, c = (case[k] for k in ("N", "A", "Cin", "Cout", "seed", "c"))
    scale, shift = bn_scale_shift(seed + 2, Cout)
    res, mask = residual_mask(seed + 3, N, A, Cout)
    dy = int_x(seed + 5, N, A, Cout)
    out_b = exact_f32((c.double() * scale.double() + shift.double()).clamp_min(0.0))
    out_r = exact_f32(c.double() + res.double())                        # residual alone: no mask zeroes what lies outside the map
    out_c = exact_f32(out_r.double() * (mask > 0))
    return dict(scale=scale, shift=shift, res=res, mask=mask, dy=dy, out_b=out_b, out_c=out_c, out_r=out_r,
                colsum=exact_f32(out_c.double().sum((0, 1))), colsum_r=exact_f32(out_r.double().sum((0, 1))),
                colsum_abs=out_r.double().abs().sum((0, 1)),
                dx=exact_f32(dgrad_ref(dy, case["w"], case["sizes"])))


# ---------------------------------------------------------------------------------------------
# the large mean-to-std case (non-integer data)
# ---------------------------------------------------------------------------------------------
RATIO_SIZES, RATIO_N, RATIO_C = [(25, 42), (13, 21), (7, 11), (4, 6), (2, 3)], 3, 256
RATIO_TARGETS = (0, 3, 10, 30)
# x = |randn| has mean 0.80 and std 0.60 per value: the sum of a pixel's 256 channels is 204 +- 9.6.  A constant k on the CENTRE tap
# adds k * that sum to the He-scaled part (variance 2 E[x^2] = 2), so r = |mean| / std ~ 204 k / sqrt(2 + 92 k^2), which saturates at
# 21.  (A constant on all nine taps saturates near 3 on the small levels: zero padding removes a third or more of a border pixel's
# taps.)  k from that formula for r = 3 and 10; r = 30 is out of reach, the largest r the construction gives is within its factor 2.
RATIO_K = {0: 0.0, 3: 0.0210, 10: 0.0786, 30: 1.0}


def ratio_inputs(target):
    """(x [3, A, 256], w [256, 3, 3, 256], gamma, beta): post-ReLU-like activations, He-scaled weights plus a per-output-channel
    constant +-k (the sign alternates by group of 8 channels) on the centre tap"""
    A = R.total_rows(RATIO_SIZES)
    x = R.randn(9100, RATIO_N, A, RATIO_C).abs()
    w = R.randn(9101, RATIO_C, 3, 3, RATIO_C, scale=(2.0 / (9 * RATIO_C)) ** 0.5)
    sign = 1.0 - 2.0 * ((torch.arange(RATIO_C) // 8) % 2)
    w[:, 1, 1, :] += (RATIO_K[target] * sign).view(-1, 1)
    return x, w, 0.5 + R.rand(9102, RATIO_C), R.randn(9103, RATIO_C, scale=0.3)


def group_moments(c, sizes, G=R.GN_G):
    """(mean, var) [N, nseg, G] in fp64, the variance as the mean of squared deviations"""
    N, A, Cc = c.shape
    mean, var = (torch.empty((N, len(sizes), G), dtype=torch.float64) for _ in range(2))
    for i, sl in enumerate(R.level_slices(sizes)):
        blk = c[:, sl].double().reshape(N, -1, G, Cc // G)
        mean[:, i] = blk.mean((1, 3))
        var[:, i] = ((blk - mean[:, i].view(N, 1, G, 1)) ** 2).mean((1, 3))
    return mean, var
