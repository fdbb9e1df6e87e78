"""Plain torch-CPU references, data and case tables of the per-step derived-weight kernels -- weight_transpose_kernel<float | __bf16>,
weight_transpose_x3_kernel and split3_kernel (conv_mfma.hip), wino_weight_kernel and wino_weight_x3_kernel (winograd.hip), their batched
form weight_prep_kernel (prep.hip) and bn_fold_batch_kernel (elementwise.hip) -- for tests/test_gpu_prep_exact.py to run and
tests/test_prep_refs_cpu.py to reason about.  No GPU and no project kernel is touched here.

Exactness.  Every one of these operations is data movement plus a handful of individually rounded fp32 operations: a product with the
row scale, the additions and (exact) halvings of U = G g G^T in a fixed order, round-to-nearest-even conversions to bf16 and the exact
remainders of the three-limb split.  None of the expressions has a product feeding an addition, so a compiler has nothing to contract:
the right answer is known to the bit and the GPU tests compare bits.  (The BN fold is the exception: sqrtf, a division and a product
feeding a subtraction; it keeps the bound of test_bn_fold_sizes.)

Layouts are written as reshape / permute / zero padding of [Cout, Cin, ...] tensors, from the layout comments of the sources; the flat
index arithmetic of the kernels is restated once, in tests/test_prep_refs_cpu.py, as a Python loop over a small case.

Data.  The integer weights of the convolution tests ({-4, 0, 4}) have all-zero mid and lo limbs, so they cannot see how the lower limb
planes are placed; `weights24` draws normal x 2^k values whose 24-bit significands fill all three limbs, and `EDGE_BITS` lists the
values at which a limb split can go wrong (signed zeros, exact bf16 values, ties at the first and at the second limb in both
to-even directions).  Weights are OHWI: [Cout, ntaps, Cin]."""
from __future__ import annotations

import collections
import functools

import numpy as np
import torch

import reduce_refs as R
from reduce_refs import cdiv

F32, BF16, U16 = torch.float32, torch.bfloat16, torch.uint16


# ---------------------------------------------------------------------------------------------
# data (numpy PCG64: the same bits on every machine)
# ---------------------------------------------------------------------------------------------
K_SPREAD = 20            # weights24: binary exponents spread over +-20 around the normal's own

# fp32 bit patterns at which a three-limb split can go wrong
EDGE_BITS = (
    0x00000000, 0x80000000,             # +0, -0
    0x3F800000, 0xBFC00000,             # 1.0, -1.5: exact bf16 values (mid = lo = 0)
    0x42F70000, 0x2F810000,             # 123.5, 2^-32 (1 + 2^-7): exact bf16 values far from 1
    0x3F808000, 0x3F818000,             # 1 + 2^-8: tie, to even = down; 1 + 2^-7 + 2^-8: tie, to even = up
    0xBF808000, 0xBF818000,             # ... and their negatives
    0x3F802020, 0x3F802060,             # 1 + 2^-10 (1 + 2^-8) and 1 + 2^-10 (1 + 2^-7 + 2^-8): ties at the SECOND limb, down and up
    0xBF802020, 0xBF802060,
    0x3F80807F, 0x3F807FFF,             # one fp32 ulp above / below a first-limb tie
    0x3FFFFFFF, 0x497FFFFF,             # all-ones significands: every limb rounds up
    0x34ABCDEF, 0xC9FEDCBA,             # small and large, all limbs busy
)


def edge_values():
    """EDGE_BITS as an fp32 tensor"""
    return torch.from_numpy(np.array(EDGE_BITS, dtype=np.uint32).view(np.float32).copy())


def weights24(seed, *shape, edges=True):
    """fp32 normal x 2^k, k uniform in [-K_SPREAD, K_SPREAD]: random 24-bit significands, magnitudes (and limb remainders, 2^-16 of
    them) far from the fp32 subnormal range.  With `edges` the first values (flat order) of a tensor at least twice as long as the edge
    list are that list (a shorter one keeps its random values: the list's zeros and exact bf16 values would leave its lower limbs empty)."""
    g = R._rng(seed)
    v = g.standard_normal(shape) * np.exp2(g.integers(-K_SPREAD, K_SPREAD + 1, size=shape))
    t = torch.from_numpy(v.astype(np.float32)).reshape(shape)
    if edges:
        e = edge_values()
        if t.numel() >= 2 * e.numel():
            t.view(-1)[:e.numel()] = e
    return t


def rowscale24(seed, Cout):
    """a row scale of random 24-bit values in about [0.5, 1.5) with a NEGATIVE last row and, from two rows on, a ZERO middle row"""
    s = torch.from_numpy((0.5 + R._rng(seed).random(Cout)).astype(np.float32))
    s[-1] = -s[-1]
    if Cout >= 2:
        s[(Cout - 1) // 2] = 0.0
    return s


def bits16(t):
    """a bf16 tensor as uint16 bit patterns"""
    return t.contiguous().view(U16)


# ---------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------
def limbs_ref(x):
    """[3, *x.shape] uint16: hi = bf16(x), r = x - hi in fp32, mid = bf16(r), lo = bf16(r - mid); torch's CPU conversion rounds to
    nearest even.  Both remainders are exact in fp32 (<= 16 and <= 8 significant bits), so lo is exact too and hi + mid + lo == x."""
    assert x.dtype == F32
    hi = x.to(BF16)
    r = x - hi.float()
    mid = r.to(BF16)
    lo = (r - mid.float()).to(BF16)
    return bits16(torch.stack([hi, mid, lo]))


def limbs_value(planes):
    """uint16 limb planes -> their fp32 values"""
    return planes.view(BF16).float()


def split3_ref(x):
    """[3][n]"""
    return limbs_ref(x.reshape(-1))


def transpose_ref(w, rowscale, flip, out, _scale_by="co", _reverse=True):
    """dst[ci][t'][co] = fl32(w[co][t][ci] * rowscale[co]), t' = ntaps - 1 - t under flip; `out`: "f32" as is, "bf16" rounded once
    (uint16 bits), "x3" the three limb planes [3][Cin][ntaps][Cout] (uint16 bits).  (`_scale_by`, `_reverse`: the deliberate
    mistakes of the sensitivity test.)"""
    Cout, ntaps, Cin = w.shape
    v = w
    if rowscale is not None:
        if _scale_by == "co":
            v = w * rowscale.reshape(Cout, 1, 1)
        else:
            v = w * rowscale[torch.arange(Cin) % Cout].reshape(1, 1, Cin)
    if flip and _reverse:
        v = v.flip(1)
    d = v.permute(2, 1, 0).contiguous()
    if out == "f32":
        return d
    if out == "bf16":
        return bits16(d.to(BF16))
    assert out == "x3"
    return limbs_ref(d)


def wino_U_f32(w, flip):
    """[Cout, Cin, 4, 4] fp32, U = G g G^T in the kernels' operation order: the column stage t1 = 0.5 ((g0 + g1) + g2),
    t2 = 0.5 ((g0 - g1) + g2), t0 = g0, t3 = g2 over the tap rows, then the same over the columns of t.  Every addition is one fp32
    addition, the halvings are exact; under flip tap 3a + b is read from 8 - (3a + b)."""
    Cout, ntaps, Cin = w.shape
    assert ntaps == 9 and w.dtype == F32
    g = (w.flip(1) if flip else w).reshape(Cout, 3, 3, Cin).permute(0, 3, 1, 2)        # [co, ci, a, b]

    def stage(x0, x1, x2):
        return [x0, 0.5 * ((x0 + x1) + x2), 0.5 * ((x0 - x1) + x2), x2]
    t = torch.stack(stage(g[:, :, 0], g[:, :, 1], g[:, :, 2]), 2)                       # [co, ci, i, b]
    return torch.stack(stage(t[..., 0], t[..., 1], t[..., 2]), 3).contiguous()          # [co, ci, i, j]


def _pad_rows(U, rows, value=0.0):
    pad = torch.full((rows - U.shape[0],) + tuple(U.shape[1:]), value, dtype=U.dtype)
    return torch.cat([U, pad], 0)


def wino_image_ref(w, flip, _pad_value=0.0):
    """the fp32 image [16][ceil16(Cout) / 16][Cin / 16][4][16][4], indexed (xi = 4 i + j, co / 16, ci / 16, (ci % 16) / 4, co % 16,
    ci % 4); rows past Cout are zero"""
    Cout, _, Cin = w.shape
    assert Cin % 16 == 0
    cop = cdiv(Cout, 16) * 16
    U = _pad_rows(wino_U_f32(w, flip).reshape(Cout, Cin, 16), cop, _pad_value)
    U = U.reshape(cop // 16, 16, Cin // 16, 4, 4, 16)              # (co / 16, co % 16, ci / 16, kq, ci % 4, xi)
    return U.permute(5, 0, 2, 3, 1, 4).contiguous()


def wino_image_x3_ref(w, flip, _pad_value=0.0, _lane_major="half"):
    """the three-limb image [16][3][ceil32(Cout) / 32][Cin / 16][64][8] (uint16 bits): limbs_ref(wino_U_f32) at lane =
    (ci % 16 / 8) * 32 + co % 32, last index ci % 8; rows past Cout are zero bits"""
    Cout, _, Cin = w.shape
    assert Cin % 16 == 0
    cop = cdiv(Cout, 32) * 32
    U = _pad_rows(wino_U_f32(w, flip).reshape(Cout, Cin, 16), cop, _pad_value)
    L = limbs_ref(U).reshape(3, cop // 32, 32, Cin // 16, 2, 8, 16)   # (limb, co / 32, co % 32, ci / 16, ci % 16 / 8, ci % 8, xi)
    if _lane_major == "half":
        L = L.permute(6, 0, 1, 3, 4, 2, 5)
    else:                                                          # the deliberate mistake: lane = (co % 32) * 2 + ci % 16 / 8
        L = L.permute(6, 0, 1, 3, 2, 4, 5)
    return L.reshape(16, 3, cop // 32, Cin // 16, 64, 8).contiguous()


def wino_image_elems(Cout, Cin):
    return 16 * cdiv(Cout, 16) * 16 * Cin


def wino_image_x3_elems(Cout, Cin):
    return 16 * 3 * cdiv(Cout, 32) * 32 * Cin


def eps32(eps):
    """the launchers take eps as a float: this is the number both sides add to the variance"""
    return float(np.float32(eps))


def bn_fold_ref(gamma, beta, mean, var, eps, double=False):
    """(scale, shift): s = gamma * (1 / sqrt(var + eps)), shift = beta - mean * s, each operation rounded to fp32 -- or, with `double`,
    all of it in fp64 on the same fp32 eps (the reference of test_bn_fold_sizes, written as the kernel writes it)"""
    if double:
        gamma, beta, mean, var = gamma.double(), beta.double(), mean.double(), var.double()
        e = eps32(eps)
    else:
        e = torch.tensor(eps32(eps), dtype=F32)
    s = gamma * (1.0 / torch.sqrt(var + e))
    return s, beta - mean * s


KINDS = (0, 1, 2, 3, 4)      # weight_prep_kernel: transpose to fp32, to bf16, Winograd image, limb planes, three-limb Winograd image


def prep_blocks(kind, Cout, ntaps, Cin):
    """erd_weight_prep_blocks restated: workgroups of 256 threads an item of the batched kernel takes"""
    if kind == 2:
        return cdiv(cdiv(Cout, 16) * 16 * Cin, 256)
    if kind == 3:
        return cdiv(Cout * ntaps * Cin, 256)
    if kind == 4:
        return cdiv(cdiv(Cout, 32) * 32 * Cin, 256)
    return cdiv(Cin, 32) * cdiv(Cout, 32) * ntaps


# ---------------------------------------------------------------------------------------------
# comparison: the first element that differs, named
# ---------------------------------------------------------------------------------------------
def first_diff(got, want):
    """flat index of the first element whose BITS differ, or None"""
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    ne = (R.bits(got).reshape(-1) != R.bits(want).reshape(-1)).nonzero()
    return None if ne.numel() == 0 else int(ne[0])


def where_transposed(flat, Cout, ntaps, Cin):
    plane, r = divmod(flat, Cin * ntaps * Cout)
    ci, r = divmod(r, ntaps * Cout)
    t, co = divmod(r, Cout)
    return dict(plane=plane, position=t, co=co, ci=ci)


def where_image(flat, Cout, Cin):
    xi, cb, kb, kq, c16, c4 = np.unravel_index(flat, (16, cdiv(Cout, 16), Cin // 16, 4, 16, 4))
    return dict(plane=0, position=int(xi), co=int(cb * 16 + c16), ci=int(kb * 16 + kq * 4 + c4))


def where_image_x3(flat, Cout, Cin):
    xi, limb, cb, kb, lane, e = np.unravel_index(flat, (16, 3, cdiv(Cout, 32), Cin // 16, 64, 8))
    return dict(plane=int(limb), position=int(xi), co=int(cb * 32 + lane % 32), ci=int(kb * 16 + (lane // 32) * 8 + e))


def where_planes(flat, n):
    plane, i = divmod(flat, n)
    return dict(plane=plane, position=i, co=None, ci=None)


def explain(got, want, where):
    """None if the bits agree, else a message that names the first differing element as (plane, position, co, ci)"""
    f = first_diff(got, want)
    if f is None:
        return None
    g, w = R.bits(got).reshape(-1)[f], R.bits(want).reshape(-1)[f]
    mask = 0xFFFFFFFF if got.dtype == F32 else 0xFFFF
    n = int((R.bits(got).reshape(-1) != R.bits(want).reshape(-1)).sum())
    return f"first of {n} differing elements at flat {f} {where(f)}: got bits {int(g) & mask:#x}, want {int(w) & mask:#x}"


# ---------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------
T_SIZES = (1, 3, 31, 32, 33, 64, 65, 100)          # below, on and past the 32 x 33 tile edge, one to four tiles
T_NTAPS = (1, 9, 49)
T_OUTS = ("f32", "bf16", "x3")
TCase = collections.namedtuple("TCase", "Cout ntaps Cin flip rs seed")


def _transpose_cases():
    """for every (ntaps, flip, row scale) all eight sizes as Cout, each paired with another size as Cin by a rotation -- so that all
    eight occur as Cin too"""
    out = []
    for ti, nt in enumerate(T_NTAPS):
        for flip in (0, 1):
            for rs in (0, 1):
                shift = 1 + 2 * ti + flip + 3 * rs
                for i, v in enumerate(T_SIZES):
                    out.append(TCase(v, nt, T_SIZES[(i + shift) % len(T_SIZES)], flip, rs, 7000 + 2 * len(out)))
    return tuple(out)


T_CASES = _transpose_cases()


@functools.lru_cache(maxsize=None)
def transpose_inputs(case):
    """(w [Cout, ntaps, Cin], row scale [Cout] or None)"""
    return weights24(case.seed, case.Cout, case.ntaps, case.Cin), (rowscale24(case.seed + 1, case.Cout) if case.rs else None)


W_COUTS = (1, 15, 16, 17, 31, 32, 33, 68, 70, 80, 128)
W_CINS = (16, 32, 48, 64, 80)
WCase = collections.namedtuple("WCase", "Cout Cin flip")
W_CASES = tuple(WCase(co, ci, f) for ci in W_CINS for co in W_COUTS for f in (0, 1))


@functools.lru_cache(maxsize=None)
def wino_inputs(case, data):
    """[Cout, 9, Cin]: "int" the {-4, 0, 4} weights of the convolution tests, "w24" the 24-bit data"""
    seed = 8000 + 1000 * case.flip + 7 * case.Cout + case.Cin
    if data == "int":
        import wino_refs
        return wino_refs.int_w(seed, case.Cout, case.Cin).reshape(case.Cout, 9, case.Cin)
    return weights24(seed, case.Cout, 9, case.Cin)


SPLIT3_NS = (1, 255, 256, 257, 70001)


@functools.lru_cache(maxsize=None)
def split3_inputs(n):
    return weights24(8800 + n, n)


# ---- the batched kernel --------------------------------------------------------------------------
Item = collections.namedtuple("Item", "kind Cout ntaps Cin flip rs")

# (Cout, ntaps, Cin) per kind: [exactly one block], [a hundred blocks and more], [ragged shapes of the single-item cases]
_T_ONE, _T_BIG, _T_RAG = [(31, 1, 3), (1, 1, 1), (32, 1, 32)], [(100, 49, 65), (65, 9, 100), (33, 49, 33)], [(3, 9, 31), (64, 1, 33), (100, 9, 1)]
_POOLS = {
    0: (_T_ONE, _T_BIG, _T_RAG),
    1: (_T_ONE, _T_BIG, _T_RAG),
    2: ([(15, 9, 16), (1, 9, 16), (16, 9, 16)], [(128, 9, 80), (68, 9, 64)], [(70, 9, 48), (17, 9, 32), (33, 9, 16)]),
    3: ([(3, 9, 3), (1, 1, 1), (16, 1, 16)], [(65, 9, 100), (33, 49, 33)], [(257, 1, 1), (17, 9, 32), (31, 1, 33)]),
    4: ([(1, 9, 16), (31, 9, 16)], [(128, 9, 80), (70, 9, 64)], [(33, 9, 48), (80, 9, 16), (17, 9, 32)]),      # (never one block: >= 2)
}


def kind_tour(n=len(KINDS)):
    """a closed walk over the kinds that takes every ordered pair (a, b), a == b included, exactly once: n * n + 1 entries"""
    unused = {a: list(range(n)) for a in range(n)}
    stack, tour = [0], []
    while stack:
        a = stack[-1]
        if unused[a]:
            stack.append(unused[a].pop())
        else:
            tour.append(stack.pop())
    return tour[::-1]


def _mixed_table():
    """40 items: the tour of the kinds, ten more at random, shapes dealt per kind from its pools in turn; the last four put a
    588-block item in front of two one-block items in front of a 108-block item"""
    kinds = kind_tour() + [int(k) for k in R._rng(8900).integers(0, len(KINDS), size=10)]
    turn = collections.Counter()
    out = []
    for pos, kind in enumerate(kinds):
        pools = _POOLS[kind]
        pool = pools[turn[kind] % 3]
        Cout, ntaps, Cin = pool[(turn[kind] // 3) % len(pool)]
        turn[kind] += 1
        out.append(Item(kind, Cout, ntaps, Cin, 0 if kind == 3 else pos % 2, int(kind < 2 and (pos // 2) % 2 == 0)))
    out += [Item(0, 100, 49, 65, 1, 1), Item(3, 16, 1, 16, 0, 0), Item(2, 15, 9, 16, 1, 0), Item(1, 65, 9, 100, 0, 1)]
    return tuple(out)


TABLES = {
    "alone-0": (Item(0, 65, 9, 33, 1, 1),),
    "alone-1": (Item(1, 33, 49, 100, 1, 1),),
    "alone-2": (Item(2, 70, 9, 48, 1, 0),),
    "alone-3": (Item(3, 31, 9, 33, 0, 0),),
    "alone-4": (Item(4, 33, 9, 48, 1, 0),),
    "mixed": _mixed_table(),
    "first-has-one-block": (Item(2, 15, 9, 16, 0, 0), Item(0, 100, 9, 65, 1, 1), Item(4, 70, 9, 32, 1, 0), Item(3, 65, 9, 100, 0, 0)),
    "last-has-one-block": (Item(1, 65, 49, 33, 1, 0), Item(4, 17, 9, 48, 0, 0), Item(3, 33, 49, 33, 0, 0), Item(0, 1, 1, 1, 0, 1)),
    "one-block-items-only": (Item(3, 16, 1, 16, 0, 0), Item(0, 31, 1, 3, 0, 1), Item(2, 1, 9, 16, 1, 0), Item(1, 32, 1, 32, 0, 0)),
}


def item_blocks(it):
    return prep_blocks(it.kind, it.Cout, it.ntaps, it.Cin)


def item_out(it):
    """(elements, bytes per element) of an item's destination"""
    n = it.Cout * it.ntaps * it.Cin
    return {0: (n, 4), 1: (n, 2), 2: (wino_image_elems(it.Cout, it.Cin), 4), 3: (3 * n, 2),
            4: (wino_image_x3_elems(it.Cout, it.Cin), 2)}[it.kind]


@functools.lru_cache(maxsize=None)
def table_inputs(name):
    """[(w, row scale or None)] of a table's items"""
    return tuple((weights24(9000 + 40 * sorted(TABLES).index(name) + 2 * j, it.Cout, it.ntaps, it.Cin),
                  rowscale24(9500 + 2 * j, it.Cout) if it.rs else None) for j, it in enumerate(TABLES[name]))


def item_ref(it, w, rs):
    """the destination of one item of the batched kernel, flat"""
    if it.kind in (0, 1):
        return transpose_ref(w, rs, it.flip, "f32" if it.kind == 0 else "bf16").reshape(-1)
    if it.kind == 2:
        return wino_image_ref(w, it.flip).reshape(-1)
    if it.kind == 3:
        return split3_ref(w).reshape(-1)
    return wino_image_x3_ref(w, it.flip).reshape(-1)


def item_where(it):
    if it.kind in (0, 1):
        return lambda f: where_transposed(f, it.Cout, it.ntaps, it.Cin)
    if it.kind == 2:
        return lambda f: where_image(f, it.Cout, it.Cin)
    if it.kind == 3:
        return lambda f: where_planes(f, it.Cout * it.ntaps * it.Cin)
    return lambda f: where_image_x3(f, it.Cout, it.Cin)


# ---- the batched BN fold -------------------------------------------------------------------------
BN_NS = (1, 255, 256, 257, 1000)
BN_EPS = (1e-5, 1e-3, 1e-4, 1e-6, 2e-5)
BN_BOUND = 1e-6              # test_bn_fold_sizes: max |got - ref64| / max |ref64|, for the scale and for the shift


@functools.lru_cache(maxsize=None)
def bn_inputs(j):
    """(gamma, beta, mean, var) of item j: running variances in [0.5, 1.5); means a quarter the size of the betas, so that the shift
    beta - mean * s of a ONE-element item -- whose maximum norm is that element -- does not come out of a cancellation"""
    n = BN_NS[j]
    return (0.5 + R.rand(9701 + 10 * j, n), R.randn(9702 + 10 * j, n), R.randn(9703 + 10 * j, n, scale=0.25), 0.5 + R.rand(9704 + 10 * j, n))
