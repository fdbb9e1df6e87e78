"""GPU: the kernels that move data between the convolutions -- stem, max-pool, FPN top-down add and its adjoint, per-level scale,
channel padding, fp32 -> bf16, BN fold -- against the plain CPU references of tests/glue_refs.py.

All but the numeric stem test and the BN fold are selections, copies, single IEEE operations, or sums of small integers (exact in
any order: tests/test_glue_refs_cpu.py bounds every partial sum), so they are held to BIT equality: one wrong pixel fails.  Every
output is pre-filled with NaN, so an element the kernel does not write fails too.  Which branch each case reaches (tiles per
workgroup, chunks per level, grid caps crossed) is computed from the launchers' constants in glue_refs.py and asserted in the CPU
test."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import glue_refs as R
import golden_inputs as G

NAN = float("nan")
F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(scope="module")
def K():
    from erd_amd import kernels
    assert torch.cuda.is_available()
    return kernels


def nans(shape, dtype=F32):
    return torch.full(tuple(shape), NAN, dtype=dtype, device="cuda")


def dev(*ts):
    """GPU copies, to be bound to names that outlive the launch: a raw pointer does not keep a temporary's memory alive"""
    return tuple(t.cuda() for t in ts)


def ints(seed, lo, hi, *shape):
    """integer-valued fp32 in [lo, hi]"""
    return G.randint(seed, lo, hi + 1, *shape).float()


def relerr(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def assert_same(got, want, what=""):
    """torch.equal, with a message that names the first element that differs"""
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not torch.equal(got, want):
        bad = (got != want) | (torch.isnan(got) != torch.isnan(want))
        first = [int(v) for v in bad.nonzero()[0]]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ ({int(torch.isnan(got).sum())} NaN); "
                             f"first at {first}: got {float(got[tuple(first)])}, want {float(want[tuple(first)])}")


# ---------------------------------------------------------------------------------------------
# stem
# ---------------------------------------------------------------------------------------------
def run_stem(K, x, w_oihw, scale, shift):
    """erd_stem_conv7x7_bn_relu alone: the UN-pooled NHWC map"""
    N, _, H, W = x.shape
    y = nans((N, R.conv_out(H, 7, 2, 3), R.conv_out(W, 7, 2, 3), 64))
    xg, wg, sc, sh = dev(x, w_oihw.permute(0, 2, 3, 1).contiguous(), scale, shift)
    K.call("erd_stem_conv7x7_bn_relu", K._p(xg), K._p(wg), K._p(sc), K._p(sh), K._p(y), N, H, W, K._stream())
    return y


@pytest.mark.parametrize("rnd", [0, 1, 2])
def test_stem_exact_persistent_tiles(K, rnd):
    """2x and 4x 3x259x1099 (612 and 1224 tiles on 512 workgroups): workgroups 0..99 run two tiles -- the prefetch behind the MFMAs and
    the stash into the other LDS buffer -- and at 4x workgroups 0..199 run three: the first buffer is used again.  Delta weights make
    every output one input pixel (or a zero of the padding) times a power of two plus a small integer: exact."""
    N, (H, W) = 4, R.STEM_BIG
    assert [R.stem_tiles(n, H, W)[2:] for n in (2, 4)] == [(2, 100), (3, 200)]
    x, scale, shift = R.stem_exact_inputs(N, H, W)
    w = R.delta_weights(rnd)
    want = R.stem_ref(x, w, scale, shift).float()            # image n does not depend on N: one reference serves both
    for n in (2, 4):
        assert_same(run_stem(K, x[:n].contiguous(), w, scale, shift), want[:n], f"stem {n}x3x{H}x{W} round {rnd}")


@pytest.mark.parametrize("N,H,W", [R.STEM_SHAPES[0]] + R.STEM_SHAPES[3:])
def test_stem_exact_small_images(K, N, H, W):
    """one tile per workgroup; images smaller than the 7x7 filter (every tap but a few reads padding) and one-row tiles"""
    x, scale, shift = R.stem_exact_inputs(N, H, W)
    for rnd in range(3):
        w = R.delta_weights(rnd)
        assert_same(run_stem(K, x, w, scale, shift), R.stem_ref(x, w, scale, shift).float(), f"stem {N}x3x{H}x{W} round {rnd}")


def test_stem_numeric_edges(K):
    """random weights at the two-tiles-per-workgroup size, fp64 reference, the project's bound -- on the whole map and, each
    normalised by ITS OWN maximum, on the border strips: the last (ragged) tile row and column, the first row and column"""
    N, (H, W) = 2, R.STEM_BIG
    x = G.randn(931, N, 3, H, W)
    w = G.randn(932, 64, 3, 7, 7, scale=0.1)
    scale, shift = 0.5 + G.rand(933, 64), G.randn(934, 64, scale=0.1)
    got = run_stem(K, x, w, scale, shift).cpu().double()
    want = R.stem_ref(x, w, scale, shift)
    OH, OW = want.shape[1:3]
    r0, c0 = (OH - 1) // R.ST_TH * R.ST_TH, (OW - 1) // R.ST_TW * R.ST_TW
    assert (OH - r0, OW - c0) == (2, 6)                                       # both last tiles are ragged
    strips = {"whole map": (slice(None), slice(None)), "last tile row": (slice(r0, OH), slice(None)),
              "last tile column": (slice(None), slice(c0, OW)), "first row": (slice(0, 1), slice(None)),
              "first column": (slice(None), slice(0, 1))}
    errs = {k: relerr(got[:, sy, sx], want[:, sy, sx]) for k, (sy, sx) in strips.items()}
    print("stem relerr:", errs)
    assert not bool(torch.isnan(got).any())
    for k, e in errs.items():
        assert e < 2e-5, (k, e)


# ---------------------------------------------------------------------------------------------
# max-pool 3x3 s2 p1
# ---------------------------------------------------------------------------------------------
def run_maxpool(K, x_nhwc, dtype):
    N, H, W, Cc = x_nhwc.shape
    out = nans((N, R.conv_out(H, 3, 2, 1), R.conv_out(W, 3, 2, 1), Cc), dtype)
    xg, = dev(x_nhwc)
    K.call("erd_maxpool3x3s2", K._p(xg), K._p(out), N, H, W, Cc, K._mt(out), K._stream())
    return out


def maxpool_ref(x_nhwc):
    return F.max_pool2d(x_nhwc.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous()


def check_maxpool(K, x, what):
    want = maxpool_ref(x)
    assert_same(run_maxpool(K, x, F32), want, what + " f32")
    assert_same(run_maxpool(K, x, BF16), want.to(BF16), what + " bf16")       # a selection, then one rounding


@pytest.mark.parametrize("Cc", R.MAXPOOL_CS)
def test_maxpool_negative_windows(K, Cc):
    """STRICTLY negative maps (the product only ever feeds a ReLU output): a maximum that starts at 0, or padding read as 0, shows
    in every window / every border window.  1- and 2-pixel maps, odd and even sizes, C != 64."""
    for N in R.MAXPOOL_NS:
        for i, (H, W) in enumerate(R.MAXPOOL_SIZES):
            x = -(G.randn(1000 + 10 * i + N, N, H, W, Cc).abs() + 0.01)
            assert float(x.max()) < 0
            check_maxpool(K, x, f"maxpool {N}x{H}x{W}x{Cc} negative")


def test_maxpool_mixed_sign(K):
    check_maxpool(K, G.randn(1101, 3, 34, 47, 68), "maxpool 3x34x47x68 mixed")


def test_maxpool_past_grid_cap(K):
    """131769 output pixels x 16 float4 > 8192 x 256 threads: the grid-stride loop runs twice"""
    x = -(G.randn(1102, *R.MAXPOOL_BIG).abs() + 0.01)
    check_maxpool(K, x, "maxpool 1x726x726x64")


# ---------------------------------------------------------------------------------------------
# FPN top-down add (nearest upsample) and its adjoint
# ---------------------------------------------------------------------------------------------
def check_upsample_fwd(K, N, HW, hw, Cc, dtype, seed):
    fine, coarse = G.randn(seed, N, *HW, Cc).to(dtype), G.randn(seed + 1, N, *hw, Cc).to(dtype)
    f = fine.cuda()
    K.upsample_add_(f, coarse.cuda())
    # fp32: one add.  bf16: both sides widen exactly, add in fp32 and round once to nearest even
    assert_same(f, R.upsample_add_ref(fine.float(), coarse.float()).to(dtype), f"upsample_add {HW}<-{hw} {dtype}")


def check_upsample_bwd(K, N, HW, hw, Cc, dtype, seed):
    dfine = ints(seed, -R.UPSAMPLE_INT_MAX, R.UPSAMPLE_INT_MAX, N, *HW, Cc)
    dcoarse = ints(seed + 1, -R.UPSAMPLE_INT_MAX, R.UPSAMPLE_INT_MAX, N, *hw, Cc)
    dcoarse[dcoarse == 0] = 5.0                                               # `+=`: nothing to add into is no test of it
    dc = dcoarse.to(dtype).cuda()
    K.upsample_add_bwd_(dfine.to(dtype).cuda(), dc)
    assert_same(dc, R.upsample_add_bwd_ref(dfine, dcoarse).to(dtype), f"upsample_add_bwd {HW}<-{hw} {dtype}")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_upsample_add_pairs(K, dtype):
    for i, (HW, hw) in enumerate(R.UPSAMPLE_PAIRS):
        check_upsample_fwd(K, R.UPSAMPLE_N, HW, hw, R.UPSAMPLE_C, dtype, 1200 + 4 * i)
        check_upsample_bwd(K, R.UPSAMPLE_N, HW, hw, R.UPSAMPLE_C, dtype, 1202 + 4 * i)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_upsample_add_batch_strided_views(K, dtype):
    """both maps are `buf[:, :H]` of a taller buffer (image stride != H*W*C); the rows outside the views keep their NaN fill"""
    N, Cc, (HW, hw) = R.UPSAMPLE_N, R.UPSAMPLE_C, R.UPSAMPLE_STRIDED
    (H, W), (h, w) = HW, hw

    def bufs():
        return nans((N, H + 3, W, Cc), dtype), nans((N, h + 3, w, Cc), dtype)
    fbuf, cbuf = bufs()
    fine, coarse = G.randn(1301, N, H, W, Cc).to(dtype), G.randn(1302, N, h, w, Cc).to(dtype)
    fbuf[:, :H] = fine.cuda()
    cbuf[:, :h] = coarse.cuda()
    assert fbuf[:, :H].stride(0) == (H + 3) * W * Cc and not fbuf[:, :H].is_contiguous()
    K.upsample_add_(fbuf[:, :H], cbuf[:, :h])
    assert_same(fbuf[:, :H], R.upsample_add_ref(fine.float(), coarse.float()).to(dtype), "strided upsample_add")
    assert_same(cbuf[:, :h], coarse, "strided upsample_add: coarse")
    assert bool(torch.isnan(fbuf[:, H:]).all()) and bool(torch.isnan(cbuf[:, h:]).all())

    fbuf, cbuf = bufs()
    dfine, dcoarse = ints(1303, -8, 8, N, H, W, Cc), ints(1304, 1, 8, N, h, w, Cc)
    fbuf[:, :H] = dfine.to(dtype).cuda()
    cbuf[:, :h] = dcoarse.to(dtype).cuda()
    K.upsample_add_bwd_(fbuf[:, :H], cbuf[:, :h])
    assert_same(cbuf[:, :h], R.upsample_add_bwd_ref(dfine, dcoarse).to(dtype), "strided upsample_add_bwd")
    assert_same(fbuf[:, :H], dfine.to(dtype), "strided upsample_add_bwd: dfine")
    assert bool(torch.isnan(fbuf[:, H:]).all()) and bool(torch.isnan(cbuf[:, h:]).all())


def test_upsample_add_past_grid_cap(K):
    """2x100x168x256 is 2.15 M float4 > 4096 x 256 threads.  The adjoint's grid runs over the COARSE map (0.54 M float4 at that
    size: not capped), so it also runs at four images (1.08 M)"""
    N, HW, hw, Cc = R.UPSAMPLE_BIG
    check_upsample_fwd(K, N, HW, hw, Cc, F32, 1401)
    check_upsample_bwd(K, N, HW, hw, Cc, F32, 1403)
    N, HW, hw, Cc = R.UPSAMPLE_BIG_BWD
    check_upsample_bwd(K, N, HW, hw, Cc, F32, 1405)


# ---------------------------------------------------------------------------------------------
# per-level scale
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("li", range(len(R.LEVEL_LISTS)))
def test_level_scale_chunks(K, li):
    """levels of 9 / 3 / 1 / 1 / 1 chunks with ragged last chunks, exactly one chunk (128 rows), one row past it (129), and a
    one-row level behind a two-chunk one"""
    sizes, N, Cc = R.LEVEL_LISTS[li], R.LEVEL_N, R.LEVEL_C
    A = sum(h * w for h, w in sizes)
    lv = K.make_levels(sizes)
    al = torch.tensor([R.LEVEL_ALPHAS[i % 4] for i in range(len(sizes))])
    # forward: one multiply
    x = G.randn(1500 + li, N, A, Cc)
    al_r = 0.5 + G.rand(1510 + li, len(sizes))
    y = nans((N, A, Cc))
    xg, ag = dev(x, al_r)
    K.call("erd_level_scale", K._p(xg), K._p(ag), K._p(y), N, A, Cc, C.byref(lv), K._stream())
    assert_same(y, R.level_scale_ref(x, al_r, sizes), f"level_scale {sizes}")
    # backward: integers, power-of-two alphas -> dx and the per-level sums are exact
    xi, dyi = ints(1520 + li, -3, 3, N, A, Cc), ints(1530 + li, -3, 3, N, A, Cc)
    dx, dal = nans((N, A, Cc)), nans((len(sizes),))
    xg, dyg, ag = dev(xi, dyi, al)
    K.call("erd_level_scale_bwd", K._p(xg), K._p(dyg), K._p(ag), K._p(dx), K._p(dal), N, A, Cc, C.byref(lv), K._stream())
    dx_ref, dal_ref = R.level_scale_bwd_ref(xi, dyi, al, sizes)
    assert_same(dx, dx_ref, f"level_scale_bwd dx {sizes}")
    assert_same(dal, dal_ref.float(), f"level_scale_bwd dalphas {sizes}")
    assert torch.equal(dal_ref, dal_ref.float().double())


# ---------------------------------------------------------------------------------------------
# channel padding
# ---------------------------------------------------------------------------------------------
def check_pad(K, rows, Cc, Cp, seed):
    src = G.randn(seed, rows, Cc)
    out = nans((rows, Cp))
    sg, = dev(src)
    K.call("erd_pad_channels", K._p(sg), K._p(out), rows, Cc, Cp, K._stream())
    assert_same(out, R.pad_channels_ref(src, Cp), f"pad_channels {rows}x{Cc}->{Cp}")
    assert_same(K.pad_channels(src.cuda(), Cp), R.pad_channels_ref(src, Cp), f"K.pad_channels {rows}x{Cc}->{Cp}")


def test_pad_channels(K):
    for i, (Cc, Cp) in enumerate(R.PAD_CCP):
        for rows in R.PAD_ROWS:
            check_pad(K, rows, Cc, Cp, 1600 + 2 * i + (rows > 1))
    check_pad(K, *R.PAD_WEIGHT, 1650)              # the weight form of the 70-class head: wk.reshape(1, -1)
    check_pad(K, *R.PAD_BIG, 1651)                 # 30000 x 72 values > 8192 x 256 threads


# ---------------------------------------------------------------------------------------------
# fp32 -> bf16
# ---------------------------------------------------------------------------------------------
def edge_values_of_length(n, rot):
    """bf16_edge_values() rotated by `rot` and cycled to n values"""
    v = R.bf16_edge_values().roll(rot)
    return v.repeat(-(-n // v.numel()))[:n].contiguous()


def check_to_bf16(K, src, what):
    want = R.bits16(src.to(BF16))
    assert torch.equal(R.bits16(K.to_bf16(src.cuda()).cpu()), want), what + " (to_bf16)"
    dst = torch.full((src.numel(),), -1, dtype=torch.int16, device="cuda").view(BF16)       # 0xFFFF: a NaN
    K.to_bf16_into(src.cuda(), dst)
    got = R.bits16(dst.cpu())
    if not torch.equal(got, want):
        bad = (got != want).nonzero().view(-1)
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} of {src.numel()} differ; first at {i}: "
                             f"{int(src.view(torch.int32)[i]) & 0xFFFFFFFF:#010x} -> {int(got[i]) & 0xFFFF:#06x}, want "
                             f"{int(want[i]) & 0xFFFF:#06x}")


@pytest.mark.parametrize("n", R.BF16_NS)
def test_to_bf16_bits(K, n):
    """bit patterns against torch's CPU conversion (round to nearest even): random values at every tail length and past the
    4096-workgroup cap (n = 8388611: 2097152 float4 + a 3-value tail)"""
    check_to_bf16(K, G.randn(1700, n, scale=3.0), f"to_bf16 random n={n}")


def test_to_bf16_edge_values(K):
    """ties both ways, carries into the exponent, overflow to infinity, +-0, +-inf, +-FLT_MAX: through the float4 body, and --
    every one of them -- through each tail slot"""
    ne = R.bf16_edge_values().numel()
    for n in (ne, ne + 1, ne + 2, ne + 3, 1, 2, 3, 5, 7):
        for rot in (0, 1, 2, 3):
            check_to_bf16(K, edge_values_of_length(n, rot), f"to_bf16 edges n={n} rot={rot}")
    # every edge value through tail slots 0, 0..1 and 0..2: conversions of length t from / into slices at multiples of 64 values
    edge = R.bf16_edge_values()
    for t in (1, 2, 3):
        k = -(-ne // t)
        src = torch.zeros(k, 64)
        src[:, :t] = edge_values_of_length(k * t, 0).view(k, t)
        sg = src.cuda()
        dst = torch.full((k, 64), 0x1234, dtype=torch.int16, device="cuda").view(BF16)
        for j in range(k):
            K.to_bf16_into(sg[j, :t], dst[j, :t])
        want = torch.full((k, 64), 0x1234, dtype=torch.int16)
        want[:, :t] = R.bits16(src[:, :t].to(BF16))
        assert torch.equal(R.bits16(dst.cpu()), want), f"to_bf16 edges through a {t}-value tail"


def test_to_bf16_into_flat_parameter_slices(K):
    """engine.FlatParams converts buckets of the flat buffer: slices that start at multiples of 64 floats.  The values on both sides
    of the destination slice stay as they were."""
    total = 64 * 40
    src = G.randn(1710, total, scale=2.0)
    sg = src.cuda()
    for start, n in [(64, 1), (64, 2), (128, 3), (192, 5), (64, 7), (256, 1023), (320, 1024), (64, 64 * 38), (0, total)]:
        dst = torch.full((total,), 0x1234, dtype=torch.int16, device="cuda").view(BF16)
        K.to_bf16_into(sg[start:start + n], dst[start:start + n])
        want = torch.full((total,), 0x1234, dtype=torch.int16)
        want[start:start + n] = R.bits16(src[start:start + n].to(BF16))
        assert torch.equal(R.bits16(dst.cpu()), want), (start, n)
    assert torch.equal(sg.cpu(), src)


# ---------------------------------------------------------------------------------------------
# BN fold
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.BN_FOLD_NS)
def test_bn_fold_sizes(K, n):
    """less than, exactly, one more than one workgroup, and eight of them; fp64 reference, the project's bound"""
    g, b, m, v = 0.5 + G.rand(1801, n), G.randn(1802, n), G.randn(1803, n), 0.5 + G.rand(1804, n)
    sc, sh = nans((n,)), nans((n,))
    gg, bg, mg, vg = dev(g, b, m, v)
    K.call("erd_bn_fold", K._p(gg), K._p(bg), K._p(mg), K._p(vg), 1e-5, K._p(sc), K._p(sh), n, K._stream())
    s_ref = g.double() / torch.sqrt(v.double() + float(np.float32(1e-5)))
    errs = relerr(sc.cpu().double(), s_ref), relerr(sh.cpu().double(), b.double() - m.double() * s_ref)
    print("bn_fold relerr:", n, errs)
    assert not bool(torch.isnan(sc).any() | torch.isnan(sh).any())
    assert errs[0] < 1e-6 and errs[1] < 1e-6
