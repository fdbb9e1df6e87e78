"""GPU: the pixel-offset tables of the three-limb weight-gradient kernels (conv_wgrad_row3_x3_kernel, one tap and three taps per
workgroup).  The one-tap form tabulates four 16-pixel slices per pass from a wave-uniform position that is stepped from pass to pass;
a pass that straddles an image or a segment, a map narrower than 16 pixels and the end of the pixel axis take the per-lane decode.
Shapes are chosen to break the tables, not to load the chip: slices that straddle image and segment boundaries, row wraps inside a
pass, taps in the padding, ragged channel tiles, a pixel count that is no multiple of 16, and split-K counts that leave the last
split short or one split empty.  Every case goes through erd_conv_wgrad and erd_wgrad_reduce with nsplit set by hand, is held
against an fp64 dW with the bound of test_gpu_f32x3 (as close as the fp32-MFMA kernel at the same split count, floor 3e-7), and is
run twice for bit equality."""
import ctypes as C
import functools
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

import golden_inputs as G

from wgrad_refs import CONV, GEOM, N, ROW3_SIZES, _nsplits      # the shapes and split counts (shared with test_gpu_wgrad_exact.py)


def _slices_one_tap(geom):
    return (N * sum(h * w for h, w in GEOM[geom]["out"]) + 15) // 16


def _slices_row3():
    return N * sum(h * ((w + 15) // 16) for h, w in ROW3_SIZES)


def test_the_cases_are_what_they_claim():
    for geom in GEOM:
        npix = N * sum(h * w for h, w in GEOM[geom]["out"])
        assert npix % 16 != 0
        for (h, w), (ih, iw) in zip(GEOM[geom]["out"], GEOM[geom]["in_s2"]):
            assert ((ih + 2 - 3) // 2 + 1, (iw + 2 - 3) // 2 + 1) == (h, w)
    for ns in (_slices_one_tap("narrow"), _slices_one_tap("wide"), _slices_row3()):
        _, short, empty = _nsplits(ns)
        per_s, per_e = -(-ns // short), -(-ns // empty)
        assert 0 < ns - (short - 1) * per_s < per_s                       # the last split is short
        assert (empty - 1) * per_e >= ns > (empty - 2) * per_e            # exactly the last split is empty


@pytest.fixture()
def K():
    from erd_amd import kernels as K
    yield K
    K.set_compute(K.DEFAULT_COMPUTE)


def _rel64(a, b):
    return float((a.double() - b).norm() / (b.norm() + 1e-300))


@functools.lru_cache(maxsize=None)
def _case(sizes_in, sizes_out, Cin, Cout, k, stride, pad):
    """inputs on the GPU and the fp64 dW [Cout, k, k, Cin] (computed once per shape)"""
    x = G.randn(51, N, sum(h * w for h, w in sizes_in), Cin)
    dz = G.randn(52, N, sum(h * w for h, w in sizes_out), Cout)
    ref = torch.zeros(Cout, Cin, k, k, dtype=torch.float64)
    oi = oo = 0
    for (ih, iw), (h, w) in zip(sizes_in, sizes_out):
        xl = x[:, oi:oi + ih * iw].reshape(N, ih, iw, Cin).permute(0, 3, 1, 2).double()
        dl = dz[:, oo:oo + h * w].reshape(N, h, w, Cout).permute(0, 3, 1, 2).double()
        ref += torch.nn.grad.conv2d_weight(xl, (Cout, Cin, k, k), dl, stride=stride, padding=pad)
        oi, oo = oi + ih * iw, oo + h * w
    return x.cuda(), dz.cuda(), ref.permute(0, 2, 3, 1).contiguous()


def _dw(K, mode, xg, dg, sizes_in, sizes_out, k, stride, pad, nsplit, row3):
    """dW at a split count of our choosing: erd_conv_wgrad into NaN-filled slabs, then erd_wgrad_reduce"""
    K.set_compute(mode)
    xs, dzs = K.level_views(xg, sizes_in), K.level_views(dg, sizes_out)
    xoff = tuple((t.data_ptr() - xg.data_ptr()) // 4 for t in xs)
    zoff = tuple((t.data_ptr() - dg.data_ptr()) // 4 for t in dzs)
    d, _, _, _, _, Cout, Cin, is_row3 = K._wgrad_desc(xs, dzs, k, stride, pad, xoff, zoff)
    assert d.limbs3 == (1 if mode == "f32x3" else 0) and is_row3 == row3
    d.x, d.dz, d.nsplit = xg.data_ptr(), dg.data_ptr(), nsplit
    part = torch.full((nsplit, Cout, k * k, Cin), float("nan"), device="cuda")
    d.part = part.data_ptr()
    K.call("erd_conv_wgrad", C.byref(d), K._stream())
    dW = torch.empty((Cout, k, k, Cin), device="cuda")
    K.wgrad_reduce(part, nsplit, dW, None, dW, False, None)
    torch.cuda.synchronize()
    return dW.cpu()


def _check(K, sizes_in, sizes_out, Cin, Cout, k, stride, pad, nsplit, row3):
    """the fp32-MFMA kernel is run at the SAME split count: both kernels then add the same pixels into one fp32 accumulator, and
    the length of that chain, not the table, sets most of either one's distance from fp64 (three taps, 64 -> 64, nsplit 1: fp32 MFMA
    7.97e-07, three-limb 7.36e-07; at the launch's own split count 2.6e-07 and 2.3e-07)"""
    xg, dg, ref = _case(tuple(sizes_in), tuple(sizes_out), Cin, Cout, k, stride, pad)
    err32 = _rel64(_dw(K, "f32", xg, dg, sizes_in, sizes_out, k, stride, pad, nsplit, row3), ref)
    a = _dw(K, "f32x3", xg, dg, sizes_in, sizes_out, k, stride, pad, nsplit, row3)
    b = _dw(K, "f32x3", xg, dg, sizes_in, sizes_out, k, stride, pad, nsplit, row3)
    err = _rel64(a, ref)
    print("weight gradient %d -> %d k%d s%d nsplit %d, rel L2 to fp64: fp32 MFMA %.2e | three-limb %.2e (crc %08x)"
          % (Cin, Cout, k, stride, nsplit, err32, err, zlib.crc32(a.numpy().tobytes())))
    assert not torch.isnan(a).any()
    assert err <= max(1.5 * err32, 3e-7), (err, err32)
    assert torch.equal(a, b)


@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("Cin,Cout", [(128, 136), (68, 128)])
@pytest.mark.parametrize("conv", sorted(CONV))
@pytest.mark.parametrize("geom", sorted(GEOM))
def test_one_tap_tables(K, geom, conv, Cin, Cout, which):
    k, stride, pad = CONV[conv]
    sizes_out = GEOM[geom]["out"]
    sizes_in = GEOM[geom]["in_s2"] if stride == 2 else sizes_out
    _check(K, sizes_in, sizes_out, Cin, Cout, k, stride, pad, _nsplits(_slices_one_tap(geom))[which], False)


@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("Cin,Cout", [(64, 64), (128, 80)])
def test_three_tap_tables(K, Cin, Cout, which):
    _check(K, ROW3_SIZES, ROW3_SIZES, Cin, Cout, 3, 1, 1, _nsplits(_slices_row3())[which], True)
