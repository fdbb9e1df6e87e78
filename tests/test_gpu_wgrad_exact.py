"""GPU: the four weight-gradient kernels of conv_mfma.hip (conv_wgrad_kernel, conv_wgrad_row3_kernel, conv_wgrad_row3_x3_kernel,
conv_wgrad_bf16_kernel) against the integer references of tests/wgrad_refs.py, EXACTLY and PER PARTIAL SLAB: with x in {-1, 0, 1} and
dz in {-2 .. 2} every limb, bf16 rounding, product and fp32 sum is an integer far below 2^24 (tests/test_wgrad_refs_cpu.py asserts it),
so slab s of a launch has one right value at every element -- the gradient over exactly the K-slices of split s, as wgrad_refs
enumerates them -- whatever the order of the additions.  A pixel counted twice, not at all, into the wrong split or the wrong tap, a
slab element left unwritten (the slabs start as NaN) or written by the wrong channel fails.  An empty split's slab is all zeros.

Every launch goes through erd_conv_wgrad with nsplit set by hand, then erd_wgrad_reduce for the summed dW.  The eleven instantiations
the launcher's defaults choose are reached (test_wgrad_refs_cpu.py); ERD_WGRAD_VARIANT=0 (conv_wgrad_kernel<128, 128, 32, 2>, a tuning
aid) is read once per process by the library and stays out of this file."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import wgrad_refs as Wr

NAN = float("nan")


@pytest.fixture()
def K():
    from erd_amd import kernels as K
    yield K
    K.set_compute(K.DEFAULT_COMPUTE)


def assert_exact(got, want, what):
    """every element equal, none NaN; the message names the first element that differs"""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    if not torch.equal(got, want):
        bad = ~(got == want)
        first = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ ({int(torch.isnan(got).sum())} NaN); first at "
                             f"{first}: got {float(got[first])}, want {float(want[first])}")


def desc(K, mode, xg, dg, case, three_taps, ngroups=1):
    """the launch descriptor kernels._wgrad_desc builds for these maps (xg / dg: [N, pixels, C] on the GPU, fp32 or bf16)"""
    sizes_in, sizes_out, k, stride, pad = Wr.geometry(case)
    K.set_compute(mode)
    xs, dzs = K.level_views(xg, sizes_in), K.level_views(dg, sizes_out)
    xoff = tuple((t.data_ptr() - xg.data_ptr()) // xg.element_size() for t in xs)
    zoff = tuple((t.data_ptr() - dg.data_ptr()) // dg.element_size() for t in dzs)
    d, _, _, _, _, Cout, Cin, is_row3 = K._wgrad_desc(xs, dzs, k, stride, pad, xoff, zoff, ngroups)
    assert d.limbs3 == (1 if mode == "f32x3" else 0) and d.bf16_multiplicands == (1 if mode == "bf16" else 0)
    assert is_row3 == (three_taps and mode != "bf16")
    assert (d.x_bf16, d.dz_bf16) == (int(xg.dtype == torch.bfloat16), int(dg.dtype == torch.bfloat16))
    d.x, d.dz = xg.data_ptr(), dg.data_ptr()
    return d


def launch(K, d, nsplit, shape):
    """erd_conv_wgrad at a split count of our choosing into NaN-filled slabs; returns (slabs, dW after erd_wgrad_reduce) on the CPU"""
    d.nsplit = nsplit
    part = torch.full((nsplit * d.ngroups,) + shape, NAN, device="cuda")
    d.part = part.data_ptr()
    K.call("erd_conv_wgrad", C.byref(d), K._stream())
    dWs = []
    for g in range(d.ngroups):
        dW = torch.full(shape, NAN, device="cuda")
        K.wgrad_reduce(part[g * nsplit:(g + 1) * nsplit], nsplit, dW, None, dW, False, None)
        dWs.append(dW)
    torch.cuda.synchronize()
    return part.cpu(), torch.stack(dWs).cpu()


def check(K, mode, case, Cin, Cout, three_taps, bk, x_bf16=False, dz_bf16=False):
    x, dz = Wr.inputs(case, Cin, Cout)
    xg = x.cuda().bfloat16() if x_bf16 else x.cuda()
    dg = dz.cuda().bfloat16() if dz_bf16 else dz.cuda()
    k = Wr.geometry(case)[2]
    nslices = len(Wr.units(Wr.geometry(case)[1], three_taps, bk))
    for nsplit in Wr.split_counts(nslices):
        d = desc(K, mode, xg, dg, case, three_taps)
        got, dW = launch(K, d, nsplit, (Cout, k * k, Cin))
        want = Wr.slabs(case, Cin, Cout, three_taps, bk, nsplit)
        what = f"{Wr.instantiation(mode, three_taps, Cin, Cout, x_bf16, dz_bf16)} {case} {Cin} -> {Cout} nsplit {nsplit}"
        for s in range(nsplit):
            assert_exact(got[s], want[s], f"{what}: slab {s}")
        assert_exact(dW[0], want.sum(0), f"{what}: reduced dW")


@pytest.mark.parametrize("Cin,Cout", Wr.ONE_TAP_CHANNELS)
@pytest.mark.parametrize("case", Wr.ONE_TAP_CASES, ids=lambda c: "-".join(c[1:]))
@pytest.mark.parametrize("mode", ["f32", "f32x3"])
def test_one_tap_slabs(K, mode, case, Cin, Cout):
    """conv_wgrad_kernel<128, 128, 16, 4> / conv_wgrad_row3_x3_kernel<2, 2, false>: slices of 16 pixels of the concatenated axis"""
    check(K, mode, case, Cin, Cout, False, Wr.BK_F32)


@pytest.mark.parametrize("Cin,Cout", Wr.THREE_TAP_CHANNELS)
@pytest.mark.parametrize("mode", ["f32", "f32x3"])
def test_three_tap_slabs(K, mode, Cin, Cout):
    """conv_wgrad_row3_kernel<1, 2, 1 | 1, 3, 1 | 2, 2, 2> / conv_wgrad_row3_x3_kernel<1 | 2, 1, true>: one slice per 16-column row chunk"""
    check(K, mode, Wr.ROW3_CASE, Cin, Cout, True, Wr.BK_F32)


@pytest.mark.parametrize("x_bf16,dz_bf16", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("Cin,Cout", Wr.ONE_TAP_CHANNELS)
@pytest.mark.parametrize("case", Wr.ONE_TAP_CASES, ids=lambda c: "-".join(c[1:]))
def test_bf16_slabs(K, case, Cin, Cout, x_bf16, dz_bf16):
    """conv_wgrad_bf16_kernel<x stored as bf16, dz stored as bf16>: slices of 64 pixels"""
    check(K, "bf16", case, Cin, Cout, False, Wr.BK_BF16, x_bf16, dz_bf16)


@pytest.mark.parametrize("case,Cin,Cout", [(Wr.ROW3_CASE, 128, 80), (("one", "wide", "3x3s2"), 68, 128)], ids=["three-taps", "one-tap"])
def test_grouped_launch_is_its_single_launches(K, case, Cin, Cout):
    """erd_wgrad_desc::ngroups = 2: slabs [g * nsplit, (g + 1) * nsplit) are bit for bit what a launch of group g alone writes, and both
    are the integer gradient of that group's maps"""
    three_taps = case == Wr.ROW3_CASE
    k = Wr.geometry(case)[2]
    maps = [tuple(t.cuda() for t in Wr.inputs(case, Cin, Cout, seed)) for seed in (0, 1)]
    nsplit = Wr.split_counts(len(Wr.units(Wr.geometry(case)[1], three_taps)))[1]
    d = desc(K, "f32x3", *maps[0], case, three_taps, ngroups=2)
    for g, (xg, dg) in enumerate(maps):
        d.gx[g], d.gdz[g] = xg.data_ptr(), dg.data_ptr()
    both, dW = launch(K, d, nsplit, (Cout, k * k, Cin))
    for g, (xg, dg) in enumerate(maps):
        alone, dW1 = launch(K, desc(K, "f32x3", xg, dg, case, three_taps), nsplit, (Cout, k * k, Cin))
        want = Wr.slabs(case, Cin, Cout, three_taps, Wr.BK_F32, nsplit, seed=g)
        for s in range(nsplit):
            assert_exact(alone[s], want[s], f"group {g} alone: slab {s}")
            assert_exact(both[g * nsplit + s], alone[s], f"group {g} of the grouped launch: slab {s}")
        assert_exact(dW[g], dW1[0], f"group {g}: reduced dW")
