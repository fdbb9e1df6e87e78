"""Plain torch-CPU references of the reduction-shaped kernels of elementwise.hip -- ReLU backward with column sums, column sums,
GroupNorm + ReLU forward and backward over level-concatenated [N][A][C] buffers -- and the case tables that
tests/test_gpu_reduce_exact.py runs and tests/test_reduce_refs_cpu.py reasons about.  No GPU and no project kernel is touched here.

With integer-valued inputs every sum these kernels form is exact in any order (float and double atomics included), so the GPU
tests hold them to BIT equality; the `*_max_partial_sum` functions bound the largest intermediate value of each such test from
its shapes and value ranges (the CPU test asserts < 2^24; values stored as bf16 stay <= 256).  The launch-geometry functions
restate the launchers (erd_relu_bwd_colsum, erd_colsum, make_chunks at 128 and 512 rows) so that every case names the branch it
reaches: column groups, row lanes, rows per workgroup, workgroups, the last workgroup's rows, and what each row lane's share of
them does to the unrolled loops."""
from __future__ import annotations

import numpy as np
import torch

F32_EXACT, BF16_EXACT = 2 ** 24, 2 ** 8       # integers up to these are exact in fp32 / bf16

# ---------------------------------------------------------------------------------------------
# launch geometry, restated from erd_amd/csrc/elementwise.hip
# ---------------------------------------------------------------------------------------------
GN_ROWS, GN_STAT_ROWS = 128, 512              # rows per workgroup: apply kernels / statistics kernels
GN_C, GN_G, GN_EPS = 256, 32, 1e-5            # the one instantiation that is built
GN_STAT_LANES = 16                            # row lanes of a statistics workgroup (16 float4 columns x 16 lanes)
GN_STATS_UNROLL, GN_BWD_STATS_UNROLL = 4, 2   # rows in flight per lane: `r + 48 < r1` step 64, `r + 16 < r1` step 32
MAX_SEG = 5                                   # ERD_MAX_SEG
RELU_WANT, RELU_UNROLL = 512, 4               # erd_relu_bwd_colsum: workgroups aimed at; rows in flight per lane
COLSUM_RPB, COLSUM_MAX_WGS = 64, 2048         # erd_colsum: rows per workgroup, doubled while there are more workgroups than this


def cdiv(a, b):
    return -(-a // b)


def relu_geometry(npix, C):
    """erd_relu_bwd_colsum's choices for npix rows of C channels, or None where it refuses C"""
    C4 = C // 4
    if C % 4 or not (C4 % 16 == 0 or 256 % C4 == 0):
        return None
    cw4 = 16 if C4 % 16 == 0 else C4            # float4 columns per workgroup
    gy, lanes = C4 // cw4, 256 // cw4           # column groups (grid y), row lanes
    unit = RELU_UNROLL * lanes                  # rows one pass of the unrolled loop covers
    ranges = max(RELU_WANT // gy, 1)
    rpb = cdiv(cdiv(npix, ranges), unit) * unit
    wgs = cdiv(npix, rpb)
    return dict(cw4=cw4, gy=gy, lanes=lanes, unit=unit, rpb=rpb, wgs=wgs, last=npix - (wgs - 1) * rpb)


def colsum_geometry(rows, C):
    rpb = COLSUM_RPB
    while cdiv(rows, rpb) > COLSUM_MAX_WGS:
        rpb *= 2
    wgs = cdiv(rows, rpb)
    return dict(rpb=rpb, wgs=wgs, last=rows - (wgs - 1) * rpb, column_passes=cdiv(C, 256))


def level_chunks(sizes, rows):
    """make_chunks: [(chunks, rows of the last chunk)] per level"""
    return [(cdiv(h * w, rows), (h * w - 1) % rows + 1) for h, w in sizes]


def lane_rows(rows, lanes):
    """rows each of `lanes` row lanes takes of a workgroup's `rows` rows (lane l: l, l + lanes, ...)"""
    return [max(0, cdiv(rows - l, lanes)) for l in range(lanes)]


def lane_paths(rows, lanes, unroll):
    """what the lanes of one workgroup do: the set of 'idle' / 'tail' / 'unrolled' / 'unrolled+tail'.  A lane with n rows runs
    n // unroll passes of the unrolled loop (its condition asks for `unroll` rows still ahead) and n % unroll of the tail loop."""
    out = set()
    for n in lane_rows(rows, lanes):
        p, t = divmod(n, unroll)
        out.add("idle" if n == 0 else "unrolled+tail" if p and t else "unrolled" if p else "tail")
    return out


def relu_paths(npix, C):
    """lane_paths over the full workgroups and the last one"""
    g = relu_geometry(npix, C)
    full = lane_paths(g["rpb"], g["lanes"], RELU_UNROLL) if g["wgs"] > 1 else set()
    return full | lane_paths(g["last"], g["lanes"], RELU_UNROLL)


def gn_stat_paths(sizes, unroll):
    """per level: lane_paths over its full 512-row chunks and its last one"""
    out = []
    for chunks, last in level_chunks(sizes, GN_STAT_ROWS):
        full = lane_paths(GN_STAT_ROWS, GN_STAT_LANES, unroll) if chunks > 1 else set()
        out.append(full | lane_paths(last, GN_STAT_LANES, unroll))
    return out


# ---------------------------------------------------------------------------------------------
# value ranges and generators (numpy PCG64: the same bits on every machine)
# ---------------------------------------------------------------------------------------------
C_MAX, DY_MAX, Y_MAX = 4, 3, 2                # integer-valued inputs: c in [-4, 4], dy in [-3, 3], y in [-2, 2]
PRELOAD_MAX = 8                               # accumulators handed in pre-loaded hold integers in [-8, 8]


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def ints(seed, lo, hi, *shape):
    """integer-valued fp32 in [lo, hi]"""
    return torch.from_numpy(_rng(seed).integers(lo, hi + 1, size=shape).astype(np.float32))


def randn(seed, *shape, scale=1.0, shift=0.0):
    return torch.from_numpy((shift + scale * _rng(seed).standard_normal(shape)).astype(np.float32))


def rand(seed, *shape):
    return torch.from_numpy(_rng(seed).random(shape).astype(np.float32))


def relu_y(seed, *shape):
    """integer-valued y in [-2, 2] whose zeros alternate between +0.0 and -0.0 (neither is `> 0`)"""
    y = ints(seed, -Y_MAX, Y_MAX, *shape)
    flat = y.view(-1)
    z = (flat == 0).nonzero().view(-1)
    flat[z[1::2]] = -0.0
    return y


def as_map(npix):
    """npix rows as an (N, H, W) map with N >= 2 wherever npix has a small factor"""
    N = next((n for n in (2, 3, 5, 7) if npix % n == 0 and npix > n), 1)
    rest = npix // N
    H = max(d for d in range(1, int(rest ** 0.5) + 1) if rest % d == 0)
    return N, H, rest // H


# ---------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------
RELU_DENSE_CS = (4, 8, 32, 64, 128, 256, 2048)
# one map per C with at least 3 workgroups and a ragged last one; C = 64's is long enough for rpb = 2 units, and its last workgroup
# (122 rows on 16 lanes: 8 or 7 each) is where a lane runs the unrolled loop AND the tail
RELU_BIG = {4: (2, 30, 50), 8: (2, 23, 29), 32: (2, 13, 17), 64: (2, 131, 127), 128: (2, 9, 11), 256: (2, 67, 93), 2048: (2, 7, 11)}
RELU_BF16_C = 256
RELU_REFUSED_CS = (68, 80)                    # C / 4 = 17 and 20: neither a multiple of 16 nor a divisor of 256


def relu_dense_maps(C):
    """[(N, H, W)]: 1, unit - 1, unit, unit + 1 rows and the big map"""
    unit = relu_geometry(1, C)["unit"]
    return [as_map(n) for n in (1, unit - 1, unit, unit + 1)] + [RELU_BIG[C]]


GN_LEVEL_LISTS = [[(25, 42), (13, 21), (7, 11), (4, 6), (2, 3)],      # 1050 rows = 512 + 512 + 26
                  [(16, 32)],                                         # exactly one statistics chunk, four apply chunks
                  [(19, 27)],                                         # 513 rows
                  [(1, 17), (3, 11), (7, 7), (8, 8), (5, 13)],        # 17 / 33 / 49 / 64 / 65: on and one past each unroll step
                  [(16, 16), (1, 1)],                                 # a one-row level behind a two-apply-chunk level
                  [(1, 1), (3, 43)]]                                  # a one-row level first
GN_NS = (1, 3)
GN_MASK_LISTS = (0, 3)                        # the lists of the mask-agreement and bf16 statistics tests

# (C, level list, N): level views of an [N, A, C] buffer, use_relu = False
RELU_STRIDED = [(256, li, N) for li in (0, 4) for N in (1, 3)] + [(64, 0, 3)]

COLSUM_CS, COLSUM_ROWS = (4, 68, 70, 256, 260, 1000), (1, 63, 64, 65, 4097)
COLSUM_LONG = (131073, 4)                     # 2049 workgroups at 64 rows: rpb doubles to 128
COLSUM_BF16_CS = (68, 256)


def level_slices(sizes):
    out, off = [], 0
    for h, w in sizes:
        out.append(slice(off, off + h * w))
        off += h * w
    return out


def total_rows(sizes):
    return sum(h * w for h, w in sizes)


# ---------------------------------------------------------------------------------------------
# comparisons (shared by the GPU tests and by the CPU test that shows mutated references fail them)
# ---------------------------------------------------------------------------------------------
def bits(t):
    """the bit patterns of an fp32 / bf16 tensor (so that -0 != +0 and NaN == the same NaN)"""
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


def same_bits(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and torch.equal(bits(got), bits(want))


def ulp_distance(a, b):
    """fp32 tensors -> how many representable values apart they are (int64; huge where either is NaN)"""
    def key(t):
        i = t.contiguous().view(torch.int32).long()
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)        # monotone in the value; -0 and +0 coincide
    d = (key(a) - key(b)).abs()
    return torch.where(torch.isnan(a) | torch.isnan(b), torch.full_like(d, 2 ** 40), d)


def relerr(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


# ---------------------------------------------------------------------------------------------
# ReLU backward + column sum, column sum
# ---------------------------------------------------------------------------------------------
def relu_bwd_colsum_ref(y, dy, use_relu):
    """(dz in the dtype of dy, colsum[C] in fp64).  dz = dy where y > 0, else +0.0 -- the value of dy * (y > 0), with the sign of
    zero the kernel's select gives (the product would be -0.0 under a negative dy; the two compare equal as numbers)"""
    dz = torch.where(y > 0, dy, torch.zeros_like(dy)) if use_relu else dy
    return dz, dz.double().reshape(-1, dy.shape[-1]).sum(0)


def colsum_ref(x):
    return x.double().reshape(-1, x.shape[-1]).sum(0)


def level_row_index(N, A, off, rows, img_of=None):
    """buffer row (of the [N * A] rows of an [N, A, C] buffer) of each of the N * rows logical rows of the level view that starts at
    row `off`: the strided branch's index rule, row r -> image r / rows.  `img_of(r, rows)` replaces the division (the CPU test
    shows that another rule changes the sums)"""
    r = torch.arange(N * rows, dtype=torch.int64)
    img = r // rows if img_of is None else img_of(r, rows)
    return (img * A + off + (r - img * rows)).clamp(0, N * A - 1)


def relu_colsum_max_partial_sum(npix, preload=PRELOAD_MAX):
    """every row at DY_MAX and of one sign, on top of a pre-loaded accumulator"""
    return preload + npix * DY_MAX


def colsum_max_partial_sum(rows):
    return rows * DY_MAX


# ---------------------------------------------------------------------------------------------
# GroupNorm + ReLU over [N][A][C], statistics per (image, level, group)
# ---------------------------------------------------------------------------------------------
def _eps32(eps):
    """the launcher takes eps as a float and widens it: this is the number both sides add to the variance"""
    return float(np.float32(eps))


def gn_stats_ref(c, sizes, G=GN_G, eps=GN_EPS):
    """[N, nseg, G, 2] (mean, rstd) in fp64 by the kernels' formula: var = E[x^2] - mean^2, clamped at 0"""
    N, A, Cc = c.shape
    out = torch.empty((N, len(sizes), G, 2), dtype=torch.float64)
    for i, sl in enumerate(level_slices(sizes)):
        blk = c[:, sl].double().reshape(N, -1, G, Cc // G)
        m = float(blk.shape[1] * blk.shape[3])
        mean = blk.sum((1, 3)) / m
        var = ((blk * blk).sum((1, 3)) / m - mean * mean).clamp_min(0.0)
        out[:, i, :, 0], out[:, i, :, 1] = mean, 1.0 / torch.sqrt(var + _eps32(eps))
    return out


def _per_channel(mr_level, Cc):
    """[N, G, 2] -> mean, rstd as [N, 1, C]"""
    G = mr_level.shape[1]
    return [mr_level[:, :, k].repeat_interleave(Cc // G, dim=1).unsqueeze(1) for k in (0, 1)]


def gn_fwd_ref(c, gamma, beta, sizes, G=GN_G, eps=GN_EPS):
    """(y, pre) in fp64: pre = (c - mean) * rstd * gamma + beta, y = relu(pre)"""
    mr = gn_stats_ref(c, sizes, G, eps)
    pre = torch.empty(c.shape, dtype=torch.float64)
    for i, sl in enumerate(level_slices(sizes)):
        mean, rstd = _per_channel(mr[:, i], c.shape[2])
        pre[:, sl] = (c[:, sl].double() - mean) * rstd * gamma.double() + beta.double()
    return pre.clamp_min(0.0), pre


def gn_bwd_ref(c, dy, gamma, mask, sizes, G=GN_G, eps=GN_EPS):
    """(dc [N, A, C], dgamma [C], dbeta [C]) in fp64 of y = relu(groupnorm(c)) under dy, with the ReLU mask GIVEN ([N, A, C] bool)"""
    N, A, Cc = c.shape
    mr = gn_stats_ref(c, sizes, G, eps)
    dc = torch.empty(c.shape, dtype=torch.float64)
    dgamma, dbeta = torch.zeros(Cc, dtype=torch.float64), torch.zeros(Cc, dtype=torch.float64)
    for i, sl in enumerate(level_slices(sizes)):
        mean, rstd = _per_channel(mr[:, i], Cc)
        xh = (c[:, sl].double() - mean) * rstd
        dm = dy[:, sl].double() * mask[:, sl]
        dgamma += (dm * xh).sum((0, 1))
        dbeta += dm.sum((0, 1))
        dh = dm * gamma.double()

        def group_mean(t):
            g = t.reshape(N, -1, G, Cc // G).mean((1, 3))                  # [N, G]
            return g.repeat_interleave(Cc // G, dim=1).unsqueeze(1)
        dc[:, sl] = rstd * (dh - group_mean(dh) - xh * group_mean(dh * xh))
    return dc, dgamma, dbeta


def gn_xhat_f32(c, mr, sizes):
    """fl(fl(c - mean) * rstd) in fp32 from a GIVEN fp32 mean_rstd [N, nseg, G, 2]: what all three kernels compute first (a
    subtraction followed by a multiplication: nothing there for a compiler to contract)"""
    xh = torch.empty(c.shape, dtype=torch.float32)
    for i, sl in enumerate(level_slices(sizes)):
        mean, rstd = _per_channel(mr[:, i].float(), c.shape[2])
        xh[:, sl] = (c[:, sl].float() - mean) * rstd
    return xh


def gn_pre_f32(c, mr, gamma, beta, sizes, fused):
    """the affine xh * gamma + beta in fp32 both ways a compiler may evaluate it: `fused` = one rounding (an fma; here the exact
    fp32 x fp32 product plus beta in fp64, rounded once), else the product rounded, then the sum rounded"""
    xh = gn_xhat_f32(c, mr, sizes)
    if fused:
        return (xh.double() * gamma.double() + beta.double()).float()
    return xh * gamma + beta


def gn_apply_f32(c, mr, gamma, beta, sizes, fused=False):
    """the forward's output in fp32 from a GIVEN mean_rstd.  With beta = 0 and gamma a power of two the product is exact, so both
    evaluation orders give the same bits and the GPU's y can be held to them."""
    return gn_pre_f32(c, mr, gamma, beta, sizes, fused).clamp_min(0.0)


def gn_stats_max_partial_sum(sizes, G=GN_G, Cc=GN_C):
    """sum of squares of one (image, level, group) with every value at C_MAX"""
    return max(h * w for h, w in sizes) * (Cc // G) * C_MAX * C_MAX


def gn_dbeta_max_partial_sum(sizes, N, preload=PRELOAD_MAX):
    return preload + N * total_rows(sizes) * DY_MAX


# ---- inputs ---------------------------------------------------------------------------------------
GN_POW2_GAMMAS = (0.5, 1.0, 2.0, -1.0)


def gn_int_c(li, N):
    """integer c in [-4, 4].  In a one-row level the even groups hold one value eight times: variance exactly 0."""
    sizes = GN_LEVEL_LISTS[li]
    c = ints(2000 + 10 * li + N, -C_MAX, C_MAX, N, total_rows(sizes), GN_C)
    for sl in level_slices(sizes):
        if sl.stop - sl.start == 1:
            row = c[:, sl.start].view(N, GN_G, GN_C // GN_G)
            row[:, ::2] = row[:, ::2, :1]
    return c


def gn_pow2_gamma():
    ch = torch.arange(GN_C)
    return torch.tensor(GN_POW2_GAMMAS)[(ch * 3 + ch // 8) % 4]


def gn_random_inputs(li, N):
    """(c, gamma, beta) at the scale of test_groupnorm_relu_fwd_bwd"""
    A = total_rows(GN_LEVEL_LISTS[li])
    return (randn(2100 + 10 * li + N, N, A, GN_C, scale=2.0, shift=0.3), 0.5 + rand(2101 + 10 * li + N, GN_C),
            randn(2102 + 10 * li + N, GN_C, scale=0.3))


# ---- the adversarial beta of the mask-agreement test ----------------------------------------------
def adversarial_targets(sizes, N, Cc=GN_C):
    """(image, buffer row, channel) index tensors of one element per channel: channel ch targets (image, level) number
    ch mod (N * nseg), at that pair's chosen row -- every channel is used, every (image, level) about C / (N * nseg) times"""
    ch = torch.arange(Cc)
    pair = ch % (N * len(sizes))
    n, lvl = pair // len(sizes), pair % len(sizes)
    sl = level_slices(sizes)
    row = torch.tensor([sl[l].start + (5 * i + 11 * l + 1) % (sl[l].stop - sl[l].start) for i, l in zip(n.tolist(), lvl.tolist())])
    return n, row, ch


def adversarial_beta(c, mr, gamma, sizes):
    """beta[ch] = -fl(xh * gamma[ch]) at channel ch's target element, xh in fp32 from the GIVEN mean_rstd.  There the unfused affine
    fl(xh * gamma) + beta is exactly 0 (mask off) and the fused one is the product's rounding residual: positive about half the
    time.  Kernels that evaluate the affine differently disagree on the ReLU mask at these elements."""
    n, row, ch = adversarial_targets(sizes, c.shape[0], c.shape[2])
    xh = gn_xhat_f32(c, mr, sizes)[n, row, ch]
    return -(xh * gamma), (n, row, ch)


def gn_mask_dy(seed, shape, targets):
    """integer dy in [-3, 3] with |dy| >= 1 at the target elements"""
    dy = ints(seed, -DY_MAX, DY_MAX, *shape)
    n, row, ch = targets
    at = dy[n, row, ch]
    dy[n, row, ch] = torch.where(at == 0, torch.full_like(at, 2.0), at)
    return dy
