"""Plain torch-CPU references, inputs and case tables of the four weight-gradient kernels of conv_mfma.hip (conv_wgrad_kernel,
conv_wgrad_row3_kernel, conv_wgrad_row3_x3_kernel, conv_wgrad_bf16_kernel), for tests/test_gpu_wgrad_exact.py to run and
tests/test_wgrad_refs_cpu.py to reason about.  No GPU and no project kernel is touched here.

With x in {-1, 0, 1} and dz in {-2, ..., 2} every multiplicand is one bf16 limb (the other two limbs are zero), every bf16 rounding is
the identity, and every product and every fp32 sum over the pixels of a case is an integer of magnitude <= 2 * pixels, far below
2^24 -- exact in any order.  So every kernel must reproduce the integer weight gradient at every element of every partial slab,
whatever its summation order.  test_wgrad_refs_cpu.py asserts those conditions on the cases.

`units` restates which pixels of the concatenated K axis (segment, image, row, column -- in that order) a kernel's K-slice holds, and
`split_units` which slices split s of a launch sums: per = ceil(slices / nsplit), split s = slices [s * per, (s + 1) * per).
  * one tap per workgroup: a slice is BK consecutive pixels of the axis, BK = 16 (conv_wgrad_kernel, conv_wgrad_row3_x3_kernel<2, 2,
    false>) or 64 (conv_wgrad_bf16_kernel);
  * three taps per workgroup (conv_wgrad_row3_kernel, conv_wgrad_row3_x3_kernel<.., true>): one slice per (segment, image, row,
    16-column chunk).
The shapes (GEOM, ROW3_SIZES, N; tests/test_gpu_wgrad_tables.py runs real-valued data over the same ones) are the smallest that
straddle image and segment boundaries, wrap rows inside a pass, have maps narrower than 16 pixels and leave the last split short or
empty."""
from __future__ import annotations

import functools

import torch

N = 2
# one tap: output sizes per segment, and the input sizes of the 3x3 / stride-2 / pad-1 form that produce them
GEOM = {
    "narrow": dict(out=[(7, 11), (4, 6)], in_s2=[(13, 21), (8, 12)]),                      # every map narrower than 16: per-lane decode
    "wide": dict(out=[(6, 19), (3, 37), (4, 6)], in_s2=[(11, 37), (5, 73), (8, 12)]),      # row wraps, image and segment crossings in a pass
}
CONV = {"1x1": (1, 1, 0), "3x3s2": (3, 2, 1)}
ROW3_SIZES = [(13, 21), (7, 11), (20, 36)]


def _nsplits(ns):
    """1, the first split count that leaves the last split short, the first that leaves exactly one split empty"""
    per = lambda s: -(-ns // s)
    short = next(s for s in range(2, ns) if (s - 1) * per(s) < ns < s * per(s))
    empty = next(s for s in range(2, ns + 2) if (s - 2) * per(s) < ns <= (s - 1) * per(s))
    return [1, short, empty]


ONE_TAP_CHANNELS = [(128, 136), (68, 128)]                 # (Cin, Cout): every channel tile ragged on one side
THREE_TAP_CHANNELS = [(64, 64), (128, 80), (68, 136)]
BK_F32, BK_BF16, CHUNK = 16, 64, 16


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------
def geometry(case):
    """case = ("one", geom, conv) | ("row3",) -> (sizes_in, sizes_out, k, stride, pad)"""
    if case[0] == "row3":
        return tuple(ROW3_SIZES), tuple(ROW3_SIZES), 3, 1, 1
    _, geom, conv = case
    k, stride, pad = CONV[conv]
    out = tuple(GEOM[geom]["out"])
    return (tuple(GEOM[geom]["in_s2"]) if stride == 2 else out), out, k, stride, pad


ONE_TAP_CASES = [("one", geom, conv) for geom in sorted(GEOM) for conv in sorted(CONV)]
ROW3_CASE = ("row3",)


def pixels(sizes_out):
    return N * sum(h * w for h, w in sizes_out)


@functools.lru_cache(maxsize=None)
def inputs(case, Cin, Cout, seed=0):
    """x [N, sum ih*iw, Cin] in {-1, 0, 1} and dz [N, sum h*w, Cout] in {-2 .. 2}, fp32, from a seeded CPU generator"""
    sizes_in, sizes_out = geometry(case)[:2]
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.randint(-1, 2, (N, sum(h * w for h, w in sizes_in), Cin), generator=g).float()
    dz = torch.randint(-2, 3, (N, sum(h * w for h, w in sizes_out), Cout), generator=g).float()
    return x, dz


# ---------------------------------------------------------------------------------------------
# the K axis: units, slices, splits
# ---------------------------------------------------------------------------------------------
def units(sizes_out, three_taps, bk=BK_F32):
    """the K-slices of a launch, in order: each a list of pixel indices of the concatenated axis (segment, image, row, column)"""
    if not three_taps:
        P = pixels(sizes_out)
        return [list(range(lo, min(P, lo + bk))) for lo in range(0, P, bk)]
    out, base = [], 0
    for h, w in sizes_out:
        for n in range(N):
            for a in range(h):
                row = base + (n * h + a) * w
                out += [list(range(row + c, row + min(w, c + CHUNK))) for c in range(0, w, CHUNK)]
        base += N * h * w
    return out


def split_units(us, nsplit):
    """the slices of every split: per = ceil(slices / nsplit); a split past the end is empty"""
    per = cdiv(len(us), nsplit)
    return [us[s * per:(s + 1) * per] for s in range(nsplit)]


def split_counts(nslices):
    """1, the first split count that leaves the last split short and the first that leaves exactly one split empty (for the 16-pixel
    and the row-chunk slices: _nsplits; a launch of 64-pixel slices may be too short to have the former)"""
    try:
        return _nsplits(nslices)
    except StopIteration:
        per = lambda s: cdiv(nslices, s)
        return [1, next(s for s in range(2, nslices + 2) if (s - 2) * per(s) < nslices <= (s - 1) * per(s))]


# ---------------------------------------------------------------------------------------------
# the integer weight gradient of a set of pixels
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _operands(case, Cin, Cout, seed=0):
    """Z [P, Cout] and X [taps, P, Cin] along the concatenated axis, fp64: X[t, p] is the input pixel tap t of output pixel p reads (zeros
    in the padding)"""
    sizes_in, sizes_out, k, stride, pad = geometry(case)
    x, dz = inputs(case, Cin, Cout, seed)
    Z, X, oi, oo = [], [], 0, 0
    for (ih, iw), (h, w) in zip(sizes_in, sizes_out):
        Z.append(dz[:, oo:oo + h * w].reshape(N * h * w, Cout).double())
        xl = torch.zeros(N, ih + 2 * k, iw + 2 * k, Cin, dtype=torch.float64)
        xl[:, k:k + ih, k:k + iw] = x[:, oi:oi + ih * iw].reshape(N, ih, iw, Cin).double()
        taps = []
        for ky in range(k):
            for kx in range(k):
                y0, x0 = k + ky - pad, k + kx - pad
                taps.append(xl[:, y0:y0 + stride * h:stride, x0:x0 + stride * w:stride].reshape(N * h * w, Cin))
        X.append(torch.stack(taps))
        oi, oo = oi + ih * iw, oo + h * w
    return torch.cat(Z), torch.cat(X, 1)


def wgrad_of(case, Cin, Cout, pix, seed=0):
    """[Cout, k*k, Cin] fp32: sum over the pixels `pix` of the axis of dz[p, co] * x[p + tap t, ci] -- integers, exact in fp32"""
    Z, X = _operands(case, Cin, Cout, seed)
    idx = torch.tensor(sorted(pix), dtype=torch.long)
    g = torch.einsum("po,tpi->oti", Z[idx], X[:, idx])
    assert float(g.abs().max() if g.numel() else 0) < 2 ** 24 and torch.equal(g, g.round())
    return g.float()


@functools.lru_cache(maxsize=None)
def slabs(case, Cin, Cout, three_taps, bk, nsplit, seed=0):
    """[nsplit, Cout, k*k, Cin]: what every partial slab of a launch holds (an empty split: zeros)"""
    us = units(geometry(case)[1], three_taps, bk)
    return torch.stack([wgrad_of(case, Cin, Cout, [p for u in su for p in u], seed) for su in split_units(us, nsplit)])


# ---------------------------------------------------------------------------------------------
# erd_conv_wgrad's choice of kernel, restated
# ---------------------------------------------------------------------------------------------
def instantiation(mode, three_taps, Cin, Cout, x_bf16=False, dz_bf16=False):
    """the kernel erd_conv_wgrad launches for a descriptor of this mode (defaults of every ERD_* switch)"""
    assert Cin % 4 == 0 and Cout % 4 == 0
    t = lambda b: "true" if b else "false"
    if mode == "bf16":
        return f"conv_wgrad_bf16_kernel<{t(x_bf16)}, {t(dz_bf16)}>"
    if mode == "f32x3":
        return f"conv_wgrad_row3_x3_kernel<{2 if Cout > 64 else 1}, 1, true>" if three_taps else "conv_wgrad_row3_x3_kernel<2, 2, false>"
    assert mode == "f32"
    if three_taps:
        return "conv_wgrad_row3_kernel" + ("<1, 2, 1>" if Cout <= 64 else "<1, 3, 1>" if Cout <= 96 else "<2, 2, 2>")
    return "conv_wgrad_kernel<128, 128, 16, 4>"


def tile(inst):
    """(output channels, input channels) of a workgroup of that kernel"""
    name, args = inst.split("<")
    a = [s.strip() for s in args.rstrip(">").split(",")]
    if name == "conv_wgrad_row3_x3_kernel":
        return 64 * int(a[0]), 64 * int(a[1])
    if name == "conv_wgrad_row3_kernel":
        return 32 * int(a[0]) * int(a[1]), 128
    return 128, 128
