"""Plain torch-CPU references of the data-movement ("glue") kernels of elementwise.hip -- stem, max-pool, FPN top-down add and its
adjoint, per-level scale, channel padding, fp32 -> bf16 -- and the case tables that tests/test_gpu_glue_exact.py runs and
tests/test_glue_refs_cpu.py reasons about.  No GPU and no project kernel is touched here.

All of these kernels are selections, copies, single IEEE operations or sums.  With integer-valued inputs the sums are exact in
any order, so the GPU tests hold them to BIT equality; the `*_max_partial_sum` functions below bound the largest intermediate
value of each such test from its shapes and value ranges (the CPU test asserts < 2^24 for fp32 and <= 256 for bf16), and the
launch-geometry functions restate the launchers of elementwise.hip so that every case names the branch it reaches."""
from __future__ import annotations

import itertools

import numpy as np
import torch
import torch.nn.functional as F

# ---------------------------------------------------------------------------------------------
# launch geometry, restated from erd_amd/csrc/elementwise.hip (the CPU test prints / asserts what each case reaches)
# ---------------------------------------------------------------------------------------------
ST_TH, ST_TW, STEM_GRID = 8, 32, 512          # stem: 8x32 output pixels per tile, persistent grid of at most 512 workgroups
MAXPOOL_CAP, UPSAMPLE_CAP, PAD_CAP, BF16_CAP = 8192, 4096, 8192, 4096     # grid caps (workgroups of 256 threads)
GN_ROWS = 128                                 # rows per workgroup of the level-chunked kernels
F32_EXACT, BF16_EXACT = 2 ** 24, 2 ** 8       # integers up to these are exact in fp32 / bf16


def conv_out(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def stem_tiles(N, H, W):
    """(tiles, workgroups, most tiles one workgroup runs, workgroups that run that many)"""
    OH, OW = conv_out(H, 7, 2, 3), conv_out(W, 7, 2, 3)
    tiles = -(-OW // ST_TW) * -(-OH // ST_TH) * N
    grid = min(tiles, STEM_GRID)
    most = -(-tiles // grid)
    return tiles, grid, most, tiles - (most - 1) * grid


def blocks_wanted(work_items):
    """workgroups an uncapped grid of 256 threads would have; a case is 'past the cap' when this exceeds the kernel's cap"""
    return -(-work_items // 256)


def level_chunks(sizes):
    """[(chunks, rows of the last chunk)] per level"""
    return [(-(-h * w // GN_ROWS), (h * w - 1) % GN_ROWS + 1) for h, w in sizes]


# ---------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------
STEM_IN_MAX, STEM_SCALES, STEM_SHIFT_MAX = 8, (1.0, 2.0, 0.5, -1.0), 3
STEM_BIG = (259, 1099)                         # OH = 130, OW = 550: 17 x 18 tiles per image, both ragged
STEM_SHAPES = [(2, 67, 93), (2,) + STEM_BIG, (4,) + STEM_BIG, (1, 5, 70), (1, 1, 1), (1, 6, 6), (1, 7, 33)]

MAXPOOL_SIZES = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 3), (33, 48), (34, 47)]
MAXPOOL_CS, MAXPOOL_NS = (4, 64, 68), (1, 3)
MAXPOOL_BIG = (1, 726, 726, 64)

# (H, W) <- (h, w).  The first six are the stride-2 pairs of a ResNet / FPN; for every one of them `y >> 1` IS the index rule, so
# the last two (ratios 3 and 7/3, 9/4) are what tells the kernel's general rule from a hard-wired 2x
UPSAMPLE_PAIRS = [((10, 14), (5, 7)), ((25, 42), (13, 21)), ((13, 21), (7, 11)), ((1, 1), (1, 1)), ((1, 2), (1, 1)),
                  ((3, 4), (2, 2)), ((6, 9), (2, 3)), ((7, 9), (3, 4))]
UPSAMPLE_N, UPSAMPLE_C = 2, 12
UPSAMPLE_BIG = (2, (100, 168), (50, 84), 256)          # forward past the cap; the backward's grid is over the COARSE map, so ...
UPSAMPLE_BIG_BWD = (4, (100, 168), (50, 84), 256)      # ... it takes four images to cross it
UPSAMPLE_STRIDED = ((25, 42), (13, 21))
UPSAMPLE_INT_MAX = 8

LEVEL_C, LEVEL_N, LEVEL_INT_MAX = 68, 3, 3
LEVEL_LISTS = [[(25, 42), (13, 21), (7, 11), (4, 6), (2, 3)], [(8, 16)], [(3, 43)], [(16, 16), (1, 1)]]
LEVEL_ALPHAS = (0.5, 1.0, 2.0, -4.0)

PAD_CCP = [(70, 72), (10, 12), (1, 4), (129, 132), (68, 68)]
PAD_ROWS = (1, 273)
PAD_WEIGHT = (1, 70 * 9 * 256, 72 * 9 * 256)
PAD_BIG = (30000, 70, 72)

BF16_NS = (1, 2, 3, 4, 5, 7, 1023, 8388611)
BN_FOLD_NS = (1, 255, 256, 257, 2048)


# ---------------------------------------------------------------------------------------------
# stem
# ---------------------------------------------------------------------------------------------
def stem_ref(x, w, scale, shift):
    """x NCHW, w OIHW [64,3,7,7] -> relu(conv7x7 s2 p3 * scale + shift) as NHWC fp64"""
    y = F.conv2d(x.double(), w.double(), None, 2, 3)
    y = F.relu(y * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1))
    return y.permute(0, 2, 3, 1).contiguous()


STEM_EXTRA_TAPS = [(0, 0), (0, 6), (6, 0), (6, 6), (3, 3)]


def delta_taps(rnd):
    """[(input channel, kh, kw)] of the single 1 of each of the 64 output channels in round `rnd` (0..2)"""
    taps = [(rnd,) + divmod(c, 7) for c in range(49)]
    taps += [(ci, kh, kw) for ci in range(3) for kh, kw in STEM_EXTRA_TAPS]
    assert len(taps) == 64
    return taps


def delta_weights(rnd):
    """OIHW [64,3,7,7] of zeros and ones: every output value of the stem is then ONE input pixel or an exact zero of the padding,
    so the fp32 matrix-core result is exact whatever the order of accumulation.  Over rounds 0..2 every (c, kh, kw) is hit."""
    w = torch.zeros(64, 3, 7, 7)
    for co, (ci, kh, kw) in enumerate(delta_taps(rnd)):
        w[co, ci, kh, kw] = 1.0
    return w


def stem_exact_inputs(N, H, W):
    """integer image in [-8, 8]; per-channel scale from {1, 2, 0.5, -1}; small integer shift.  Image n is the same for every N."""
    x = torch.cat([torch.from_numpy(np.random.Generator(np.random.PCG64(900 + n)).integers(
        -STEM_IN_MAX, STEM_IN_MAX + 1, size=(1, 3, H, W)).astype(np.float32)) for n in range(N)])
    co = torch.arange(64)
    scale = torch.tensor(STEM_SCALES)[(co * 5 + co // 4) % 4]
    shift = ((co * 7) % (2 * STEM_SHIFT_MAX + 1) - STEM_SHIFT_MAX).float()
    return x, scale, shift


def stem_max_partial_sum():
    """one non-zero product per output (a delta weight), then * scale + shift"""
    return STEM_IN_MAX * max(abs(s) for s in STEM_SCALES) + STEM_SHIFT_MAX


# ---------------------------------------------------------------------------------------------
# FPN top-down add (nearest upsample) and its adjoint
# ---------------------------------------------------------------------------------------------
def nearest_src(H, h):
    """source index of every destination index 0..H-1 under the kernel's integer rule min(y * h // H, h - 1).
    It equals the index F.interpolate(mode='nearest') picks (floor(y * float(h / H))) for every (h, 2h) and (h, 2h-1), the pairs a
    stride-2 backbone produces.  For other pairs the two can differ where the float product lands just under an integer:
    (26 <- 44), (30 <- 58) and (65 <- 110) are examples.  That is a known property of the kernel's rule, not a defect."""
    return torch.clamp(torch.arange(H, dtype=torch.int64) * h // H, max=h - 1)


def upsample_add_ref(fine, coarse):
    """NHWC: fine + coarse[nearest]; one add per element, in the dtype of the inputs"""
    sy, sx = nearest_src(fine.shape[1], coarse.shape[1]), nearest_src(fine.shape[2], coarse.shape[2])
    return fine + coarse[:, sy][:, :, sx]


def upsample_add_bwd_ref(dfine, dcoarse):
    """NHWC: dcoarse + (sum of dfine over the fine pixels that read each coarse pixel), in fp64"""
    sy, sx = nearest_src(dfine.shape[1], dcoarse.shape[1]), nearest_src(dfine.shape[2], dcoarse.shape[2])
    N, _, W, Cc = dfine.shape
    rows = torch.zeros((N, dcoarse.shape[1], W, Cc), dtype=torch.float64).index_add_(1, sy, dfine.double())
    return dcoarse.double().index_add(2, sx, rows)


def upsample_bwd_max_partial_sum(H, W, h, w, vmax=UPSAMPLE_INT_MAX):
    """|dcoarse| + the largest fan-in of a coarse pixel times |dfine|"""
    fan = int(torch.bincount(nearest_src(H, h), minlength=h).max()) * int(torch.bincount(nearest_src(W, w), minlength=w).max())
    return vmax + fan * vmax


# ---------------------------------------------------------------------------------------------
# per-level scale over [N][A][C]
# ---------------------------------------------------------------------------------------------
def level_slices(sizes):
    out, off = [], 0
    for h, w in sizes:
        out.append(slice(off, off + h * w))
        off += h * w
    return out


def level_scale_ref(x, alphas, sizes):
    """x * alpha[level]: one multiply per element, in the dtype of x"""
    y = torch.empty_like(x)
    for i, sl in enumerate(level_slices(sizes)):
        y[:, sl] = x[:, sl] * alphas[i]
    return y


def level_scale_bwd_ref(x, dy, alphas, sizes):
    """(dx = dy * alpha[level] in the dtype of dy, dalphas[level] = sum(dy * x) in fp64)"""
    dx = level_scale_ref(dy, alphas, sizes)
    dal = torch.stack([(dy[:, sl].double() * x[:, sl].double()).sum() for sl in level_slices(sizes)])
    return dx, dal


def level_scale_max_partial_sum(sizes, N=LEVEL_N, Cc=LEVEL_C, vmax=LEVEL_INT_MAX):
    """every product at its largest and of one sign, over the largest level of all images (dalphas is one sum per level)"""
    return N * max(h * w for h, w in sizes) * Cc * vmax * vmax


# ---------------------------------------------------------------------------------------------
def pad_channels_ref(src, Cp):
    return F.pad(src, (0, Cp - src.shape[-1]))


# ---------------------------------------------------------------------------------------------
# fp32 -> bf16
# ---------------------------------------------------------------------------------------------
BF16_EXPONENTS = (1, 64, 127, 128, 200, 254)
BF16_HIGH_KEPT = (0b000000, 0b101010, 0b111111)         # bits 22..17 of the mantissa
BF16_DROPPED = (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF)


def bf16_edge_bits():
    """int64 bit patterns of bf16_edge_values(), in order"""
    bits = [(s << 31) | (e << 23) | (hi << 17) | (low << 16) | d
            for e, s, low, hi, d in itertools.product(BF16_EXPONENTS, (0, 1), (0, 1), BF16_HIGH_KEPT, BF16_DROPPED)]
    bits += [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF]      # +-0, +-inf, +-FLT_MAX
    return torch.tensor(bits, dtype=torch.int64)


def bf16_edge_values():
    """fp32 values at which a float -> bf16 rounding can go wrong, built from bit patterns: for six exponent fields from the
    smallest normal to the largest and both signs, every combination of the kept mantissa's low bit (0 / 1: the 'even' of nearest
    even), three patterns of its upper six bits, and six values of the 16 dropped bits -- zero, just above zero, just below the
    tie, the tie, just above it, all ones.  The rows whose kept mantissa is all ones carry into the exponent when they round up,
    and at exponent field 254 that carry is the overflow to infinity.  +-0, +-inf and +-FLT_MAX are added.

    NaNs are left out (which payload a conversion keeps is not defined alike on every device) and so are denormals (whether they
    are flushed is decided by the mode register of the launch); neither occurs in weights."""
    b = bf16_edge_bits()
    return (b - ((b >> 31) << 32)).to(torch.int32).view(torch.float32)


def bits16(t):
    """bf16 tensor -> its bit patterns as int16 (what the tests compare, so that -0 != +0)"""
    return t.contiguous().view(torch.int16)
