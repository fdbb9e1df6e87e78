"""Plain torch-CPU references, inputs, case table and a host model ("census") of the two activation-stationary kernels for thin 1x1
convolutions, conv_thin_x3_kernel and conv_thin_bf16_kernel (erd_amd/csrc/conv_thin.hip), for tests/test_gpu_thin_exact.py to run and
tests/test_thin_refs_cpu.py to reason about.  No GPU and no project kernel is touched here.

Exactness.  The value scheme is igemm_refs': activations in {-1, 0, 1}, weights in {-2 .. 2}, scale in {0.5, 1, 2}, small-integer
shift / residual / accumulate base, masks in {-1, 0, 1}, per-segment alphas that are powers of two.  One bf16 limb holds every
multiplicand, every partial sum over K <= 512 terms is an integer of magnitude <= 2 K, and every result is a multiple of 1/4 far below
2^24 / 4: an output element has ONE right value whatever the order of the additions and however the work is cut into ranges.  A
bf16-stored output is that value rounded once.  Column sums add the exact fp32 values BEFORE a bf16-stored output is rounded for
storage (both the thin and the stream-K kernel sum what they computed, not what they stored): sums of integers, which float atomics
add exactly in any order.

Geometry.  N = 2 images, three segments whose OUTPUT maps have 9 x 15, 4 x 6 and 2 x 2 pixels: 270 + 48 + 8 GEMM rows in 3 + 1 + 1 = 5
pixel tiles of 128 rows.  The third tile of the first segment has 14 rows (wave 0 partly filled, waves 1-3 empty), the last segment 8.
Four tiles would not do: by the kernels' T wg / G formula no work range crosses a tile boundary at G = 16, 24 or 32 then.  Stride-2
forward inputs are 18 x 29, 7 x 11 and 3 x 3: the even height leaves a last input row that must never be read.  A case names its GEMM:
K contracted channels -> C output channels; C = 352 (11 blocks of 32) where the reduced grid has 16 or 24 workgroups, 608 (19 blocks)
where it has 32.

Census.  `thin_kind` restates the dispatch predicates conv_thin_x3_ok / conv_thin_bf16_ok, `per_cu` / `grid` the grid of launch_thin /
launch_thin_bf16, `work_ranges` and `tile_segment` the kernels' work decode, as functions of the usable CU count (defaults of every
ERD_* switch)."""
from __future__ import annotations

import collections
import functools

import torch

import igemm_refs as R
from igemm_refs import cdiv, usable_cus, xcd_contiguous      # noqa: F401  (the census of both files shares them)

N = R.N
SIZES = ((9, 15), (4, 6), (2, 2))           # output pixels per segment
S2_IN = ((18, 29), (7, 11), (3, 3))         # 1 x 1 / stride 2 / pad 0 inputs that produce SIZES
ALPHAS = (0.5, 4.0, 2.0)                    # per segment: three different powers of two, none of them 1
CUS, FEW = R.CUS, R.FEW
TILE, BLOCK = 128, 32                       # pixel rows of a tile, output channels of a block: one (tile, block) pair is a work unit

# igemm_refs' fields (and its epi flags) + views: every map is a level view of one concatenated [N, A, C] buffer; alias: the residual
# IS the output; served: the launch runs on a thin kernel (False: the dispatch must refuse it)
Case = collections.namedtuple("Case", R.Case._fields + ("views", "alias", "served"))


def _c(name, mode, form, K, C, epi="", k=1, stride=1, bf=False, few=True, views=False, alias=False, served=True):
    return Case(name, mode, form, K, C, k, stride, epi, bf, bf, few, views, alias, served)


X3_FWD = (("plain", "", {}), ("srR", "srR", {}), ("sa", "sa", {}), ("s2", "sr", dict(stride=2)), ("alias", "R", dict(alias=True)))
DGRADS = ("", "A", "m", "Am", "mc", "AmC")          # together: all four (residual, mask) instantiations; column sums in one and eight rows
BF_C = {64: 608, 128: 608, 256: 352, 512: 352}
CASES = (
    # ---- three-limb mode: K = 128 on 16 workgroups, K = 64 on 24
    [_c(f"x3-fwd-{K}to352-{n}", "f32x3", "fwd", K, 352, e, **kw) for K in (128, 64) for n, e, kw in X3_FWD] +
    [_c(f"x3-dgrad-{K}to352-{e or 'plain'}", "f32x3", "dgrad", K, 352, e) for K in (128, 64) for e in DGRADS] +
    # ---- bf16 mode, maps stored bf16: K = 64 / 128 on 32 workgroups, K = 256 on 24 (16 with residual AND mask), K = 512 on 16
    [_c(f"bf16-{form}-{K}to{BF_C[K]}-{e or 'plain'}", "bf16", form, K, BF_C[K], e, bf=True)
     for K in (64, 128, 256, 512) for form, e in (("fwd", "srR"), ("dgrad", ""), ("dgrad", "AmC"))] +
    [_c("bf16-fwd-128to608-s2", "bf16", "fwd", 128, 608, "sr", stride=2, bf=True)] +
    # ---- level views of concatenated buffers: in_nstride / out_nstride differ from h w C
    [_c("x3-dgrad-128to352-views", "f32x3", "dgrad", 128, 352, "RmC", views=True),
     _c("bf16-dgrad-256to352-views", "bf16", "dgrad", 256, 352, "RmC", bf=True, views=True)] +
    # ---- the whole chip: one unit per workgroup
    [_c("x3-fwd-128to352-srR-full", "f32x3", "fwd", 128, 352, "srR", few=False),
     _c("x3-dgrad-64to352-AmC-full", "f32x3", "dgrad", 64, 352, "AmC", few=False),
     _c("bf16-fwd-128to608-srR-full", "bf16", "fwd", 128, 608, "srR", bf=True, few=False),
     _c("bf16-dgrad-512to352-AmC-full", "bf16", "dgrad", 512, 352, "AmC", bf=True, few=False)] +
    # ---- launches the predicates refuse: they run on the stream-K kernel
    [_c("refused-K96", "f32x3", "fwd", 96, 352, "sr", served=False),
     _c("refused-C136", "f32x3", "fwd", 128, 136, "sr", served=False),
     _c("refused-3x3", "f32x3", "fwd", 64, 352, "sr", k=3, served=False),
     _c("refused-residual-on-one-segment", "f32x3", "fwd", 128, 352, "srP", served=False),
     _c("refused-fp32-mode", "f32", "fwd", 128, 352, "sr", served=False),
     _c("refused-bf16-mode-fp32-maps", "bf16", "fwd", 128, 352, "sr", served=False)])
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ---------------------------------------------------------------------------------------------
# inputs and the exact result
# ---------------------------------------------------------------------------------------------
def maps(case):
    """(input sizes, output sizes) per segment of the launch's tensors"""
    return (S2_IN if case.stride == 2 else SIZES), SIZES


@functools.lru_cache(maxsize=None)
def inputs(name):
    """igemm_refs.build_inputs on this file's maps and alphas"""
    case = BY_NAME[name]
    return R.build_inputs(case, *maps(case), alphas=ALPHAS)


def exact(case, d):
    """(outputs per segment in the storage type of the case, column sums [C] or None) for the inputs d: igemm_refs.build_expected"""
    return R.build_expected(case, d, maps(case)[1])


@functools.lru_cache(maxsize=None)
def expected(name):
    return exact(BY_NAME[name], inputs(name))


def without(name, key):
    """the result with one epilogue operand left out ("alpha", "res" -- the accumulate base counts as one --, "mask"), or None when
    the case has no such operand"""
    d = dict(inputs(name))
    if key == "res":
        key = "base" if "base" in d else "res"
    if key not in d:
        return None
    del d[key]
    return exact(BY_NAME[name], d)[0]


def unit_blocks(outs):
    """[pixel tile][channel block] -> the (rows of the tile) x 32 block of the outputs, tiles in the kernels' order"""
    tiles = []
    for y in outs:
        y2 = y.reshape(-1, y.shape[-1])
        for r0 in range(0, y2.shape[0], TILE):
            tiles.append([y2[r0:r0 + TILE, c0:c0 + BLOCK] for c0 in range(0, y2.shape[1], BLOCK)])
    return tiles


# ---------------------------------------------------------------------------------------------
# the census: the dispatch predicates, the grid and the work decode of conv_thin.hip, restated
# ---------------------------------------------------------------------------------------------
Desc = collections.namedtuple("Desc", "rows Cin Cout ntaps wrow wk0 w_x3 w_bf16 in_bf16 out_bf16 res mask in_elems out_elems")


def desc(case):
    """what kernels.conv_forward / conv_dgrad put into the launch descriptor, as far as the thin predicates and launchers read it"""
    ins, outs = maps(case)
    e = case.epi
    res = tuple(("R" in e or "A" in e or ("P" in e and i == 0)) for i in range(len(outs)))
    if case.views:      # the image stride of a level view is the whole concatenated buffer's
        ie, oe = [N * sum(h * w for h, w in ins) * case.K] * len(ins), [N * sum(h * w for h, w in outs) * case.C] * len(outs)
    else:
        ie, oe = [N * h * w * case.K for h, w in ins], [N * h * w * case.C for h, w in outs]
    return Desc(tuple(N * h * w for h, w in outs), case.K, case.C, case.k * case.k, case.k * case.k * case.K, 0,
                case.mode == "f32x3" and case.K % 4 == 0, case.mode == "bf16", case.ab, case.ob, res, tuple(["m" in e] * len(outs)),
                tuple(ie), tuple(oe))


def _common_ok(d, esize):
    if d.Cout % 32 != 0 or d.wrow % 8 != 0 or d.wk0 % 8 != 0 or d.ntaps != 1:
        return False
    if any(r != d.res[0] for r in d.res) or any(m != d.mask[0] for m in d.mask):      # instantiated per presence of the LAUNCH
        return False
    return all(n * esize < 0x7fffffff for n in d.in_elems + d.out_elems)               # 32-bit buffer byte offsets


def thin_kind(d):
    """"x3" / "bf16": the thin kernel erd_conv_igemm hands the launch to; None: the stream-K kernel (conv_thin_x3_ok / conv_thin_bf16_ok)"""
    if d.w_bf16:
        ok = not d.w_x3 and d.in_bf16 and d.out_bf16 and d.Cin in (64, 128, 256, 512) and _common_ok(d, 2)
        return "bf16" if ok else None
    ok = d.w_x3 and not d.in_bf16 and not d.out_bf16 and d.Cin in (64, 128) and _common_ok(d, 4)
    return "x3" if ok else None


def per_cu(kind, d):
    """workgroups per CU the launchers size the persistent grid for"""
    ks = d.Cin // 16
    if kind == "x3":
        return 3 if ks == 4 else 2
    return 4 if ks <= 8 else (2 if (ks > 16 or (d.res[0] and d.mask[0])) else 3)


def instantiation(kind, d):
    ks, r, m = d.Cin // 16, str(d.res[0]).lower(), str(d.mask[0]).lower()
    return f"conv_thin_x3_kernel<{ks}, 1, {r}, {m}>" if kind == "x3" else f"conv_thin_bf16_kernel<{ks}, {r}, {m}>"


def work_ranges(T, G):
    """ranges[wg] = (first unit, end unit) of the workgroup at position wg of the work order (block index b runs position
    xcd_contiguous(b, G)); a unit t is block t % nb of pixel tile t // nb"""
    return tuple((T * wg // G, T * (wg + 1) // G) for wg in range(G))


def tile_segment(rows, mt):
    """segment of pixel tile mt (the kernels' decode loop: the last segment takes what is left)"""
    seg = 0
    while seg < len(rows) - 1:
        tiles = cdiv(rows[seg], TILE)
        if mt < tiles:
            break
        mt -= tiles
        seg += 1
    return seg


Census = collections.namedtuple("Census", "kind inst G T nb mtiles ranges mid_starts tile_crossings seg_crossings units3 units2 ring_steps")


def census(case, physical=CUS, reserve=None):
    """the launch's grid and, over its workgroups, how many (a) start in the middle of a tile, (b) span a tile boundary, (c) span a
    segment boundary, (d) own at least three (two) units; ring_steps: the most LDS-ring steps of one workgroup"""
    d = desc(case)
    kind = thin_kind(d)
    assert kind is not None, case.name
    reserve = reserve_of(case, physical) if reserve is None else reserve
    mtiles, nb = sum(cdiv(r, TILE) for r in d.rows), d.Cout // BLOCK
    T = mtiles * nb
    G = min(T, per_cu(kind, d) * usable_cus(physical, reserve))
    rg = work_ranges(T, G)
    last = lambda lo, hi: (hi - 1) // nb
    return Census(kind, instantiation(kind, d), G, T, nb, mtiles, rg,
                  sum(1 for lo, hi in rg if lo % nb),
                  sum(1 for lo, hi in rg if lo // nb != last(lo, hi)),
                  sum(1 for lo, hi in rg if tile_segment(d.rows, lo // nb) != tile_segment(d.rows, last(lo, hi))),
                  sum(1 for lo, hi in rg if hi - lo >= 3), sum(1 for lo, hi in rg if hi - lo >= 2),
                  max(hi - lo for lo, hi in rg) * (2 if kind == "bf16" and d.Cin == 512 else 1))


def reserve_of(case, physical=CUS):
    return physical - FEW if case.few else 0
