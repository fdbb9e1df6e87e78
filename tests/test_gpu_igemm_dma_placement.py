"""GPU: the three-limb implicit GEMM issues the LDS-DMA requests of K-slice kt + 1 one per MFMA gap of slice kt's first k16 step, in
straight-line code (the last slice of a tile is its own copy of the loop body), and a tile's first weight requests in front of its row
decode (conv_mfma.hip, GL path of conv_igemm_kernel).  A request that is misplaced (into the buffer being read), missing (a slice with
fewer gaps than requests), not waited for, or still in flight when the next tile's prologue refills the buffers changes bits or leaves
NaNs (every output starts as NaN), so every form is compared BIT FOR BIT with the register-staged path (ERD_IG_GLDS=0: global ->
registers -> ds_write -- code the request placement does not touch).

All cases: N = 2, two segments of 7 x 11 and 4 x 6 pixels = 202 rows (the second M-tile of the first segment is ragged).  The forms are
those of tools/dbg/epi_bitcompare.py: forward (scale, shift, ReLU; + residual), input gradient (plain; mask; mask + accumulate)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import golden_inputs as G

SIZES = [(7, 11), (4, 6)]
N = 2


@pytest.fixture()
def K():
    from erd_amd import kernels as K
    keep = K.WINOGRAD
    K.set_compute("f32x3")
    K.WINOGRAD = False
    yield K
    K.WINOGRAD = keep
    K.set_compute(K.DEFAULT_COMPUTE)


def both(monkeypatch, run):
    """run() under register staging and under LDS-DMA: lists of tensors, compared bit for bit"""
    monkeypatch.setenv("ERD_IG_GLDS", "0")
    ref = run()
    monkeypatch.setenv("ERD_IG_GLDS", "1")
    got = run()
    assert len(ref) == len(got) and len(got) > 0
    for i, (a, b) in enumerate(zip(ref, got)):
        assert not torch.isnan(b).any(), i
        assert not torch.isnan(a).any(), i
        assert torch.equal(a, b), (i, float((a - b).abs().max()))


def nan_like(shape):
    return torch.full(shape, float("nan"), device="cuda")


def gemm_forms(K, seed, Cin, Cout, k=1, stride=1, sizes=SIZES):
    """a closure that runs the five forms of a K = k * k * Cin -> Cout GEMM on maps whose OUTPUT has `sizes` pixels per segment; the input
    gradient forms contract over the same K (the gradient of a Cout -> Cin convolution) when the layer is a 1x1 one"""
    p = k // 2
    ins = [(2 * h - 1, 2 * w - 1) for h, w in sizes] if stride == 2 else sizes      # (3 x 3 / stride 2 / pad 1: 13 x 21 and 7 x 11)
    for (ih, iw), (h, w) in zip(ins, sizes):
        assert K.conv_out_size(ih, k, stride, p) == h and K.conv_out_size(iw, k, stride, p) == w
    xs = [G.randn(seed + i, N, ih, iw, Cin).cuda() for i, (ih, iw) in enumerate(ins)]
    w = (G.randn(seed + 10, Cout, k, k, Cin) * (2.0 / (k * k * Cin)) ** 0.5).cuda()
    sc, sh = (0.5 + G.rand(seed + 11, Cout)).cuda(), G.randn(seed + 12, Cout, scale=0.1).cuda()
    ident = [G.randn(seed + 20 + i, N, h, wd, Cout).cuda() for i, (h, wd) in enumerate(sizes)]
    # 1x1: the input gradient of a convolution Cout -> Cin, so that its contraction runs over Cin as well
    wg = (G.randn(seed + 13, Cin, 1, 1, Cout) * (2.0 / Cin) ** 0.5).cuda() if k == 1 else None
    dys = [G.randn(seed + 30 + i, N, h, wd, Cin).cuda() for i, (h, wd) in enumerate(sizes)]
    masks = [G.randn(seed + 40 + i, N, h, wd, Cout).cuda() for i, (h, wd) in enumerate(sizes)]
    base = [G.randn(seed + 50 + i, N, h, wd, Cout).cuda() for i, (h, wd) in enumerate(sizes)]

    def run():
        res = []
        ys = [nan_like((N, h, wd, Cout)) for h, wd in sizes]
        K.conv_forward(xs, w, ys, k, stride, p, scale=sc, shift=sh, relu=True)
        res += [y.clone() for y in ys]
        ys = [nan_like((N, h, wd, Cout)) for h, wd in sizes]
        K.conv_forward(xs, w, ys, k, stride, p, scale=sc, shift=sh, res=ident, relu=True)
        res += ys
        if wg is not None:
            wt = K.weight_transpose(wg)
            dxs = [nan_like((N, h, wd, Cout)) for h, wd in sizes]
            K.conv_dgrad(dys, wt, dxs, 1, 1, 0)
            res += dxs
            dxs = [nan_like((N, h, wd, Cout)) for h, wd in sizes]
            K.conv_dgrad(dys, wt, dxs, 1, 1, 0, relu_mask=masks)
            res += dxs
            acc = [b.clone() for b in base]
            K.conv_dgrad(dys, wt, acc, 1, 1, 0, accumulate=True, relu_mask=masks)
            res += acc
        torch.cuda.synchronize()
        return res
    return run


@pytest.mark.parametrize("Cin,Cout", [
    (264, 136),      # tile-parallel (K < 512); nine slices, the last one 8 channels; chunks past Cin; the second N-tile ragged
    (520, 128),      # stream-K with fix-up (3 tiles x 17 slices on 6 workgroups); partial last slice
    (256, 64),       # the 128 x 64 instantiation (seven requests per slice); eight slices
], ids=["264to136", "520to128_streamk", "256to64"])
def test_1x1_forms_equal_register_staging_bit_for_bit(K, monkeypatch, Cin, Cout):
    both(monkeypatch, gemm_forms(K, 100 + Cin, Cin, Cout))


def test_3x3_stride2_with_padding_taps_equals_register_staging_bit_for_bit(K, monkeypatch):
    """3 x 3 / stride 2 / pad 1, 72 -> 136: K = 648 in 27 slices of which every third is 8 channels; padding taps come as zeros through
    `a_mask`, rows past the end through the row decode"""
    both(monkeypatch, gemm_forms(K, 700, 72, 136, k=3, stride=2))


def test_stride2_input_gradient_with_per_segment_taps_equals_register_staging_bit_for_bit(K, monkeypatch):
    """the merged parity classes of a 3 x 3 / stride-2 input gradient (`ST`: 4 + 2 + 2 + 1 taps in one launch, tiles of different K length),
    136 -> 72 channels, on both maps: plain, masked, masked + accumulating"""
    Cin, Cout = 72, 136      # of the forward convolution
    wt_src = (G.randn(800, Cout, 3, 3, Cin) * (2.0 / (9 * Cin)) ** 0.5).cuda()
    ins = [(13, 21), (7, 11)]
    dys = [G.randn(810 + i, N, h, w, Cout).cuda() for i, (h, w) in enumerate(SIZES)]
    masks = [G.randn(820 + i, N, h, w, Cin).cuda() for i, (h, w) in enumerate(ins)]
    base = [G.randn(830 + i, N, h, w, Cin).cuda() for i, (h, w) in enumerate(ins)]

    def run():
        wt = K.weight_transpose(wt_src)
        res = []
        for dy, (h, w), m, b in zip(dys, ins, masks, base):
            dx = nan_like((N, h, w, Cin))
            K.conv_dgrad([dy], wt, [dx], 3, 2, 1)
            res.append(dx)
            dx = nan_like((N, h, w, Cin))
            K.conv_dgrad([dy], wt, [dx], 3, 2, 1, relu_mask=[m])
            res.append(dx)
            acc = b.clone()
            K.conv_dgrad([dy], wt, [acc], 3, 2, 1, accumulate=True, relu_mask=[m])
            res.append(acc)
        torch.cuda.synchronize()
        return res
    both(monkeypatch, run)


def test_workgroups_that_run_several_tiles_back_to_back_reuse_the_buffers_cleanly(K, monkeypatch):
    """A grid smaller than the tile count: with all but eight CUs reserved the stream-K grid is 16 workgroups for 18 tiles of 17 slices
    (520 -> 768), so every workgroup ends one tile and starts the next -- whose prologue refills both buffers -- two or three times.
    A request of the previous tile still in flight would land on top of the new tile's first slices."""
    from erd_amd import _lib
    lib = _lib.load()
    prev = K.set_cu_reserve(0)
    try:
        cus = int(lib.erd_usable_cus())
        K.set_cu_reserve(max(cus - 8, 0))
        assert int(lib.erd_usable_cus()) == 8
        both(monkeypatch, gemm_forms(K, 900, 520, 768))
    finally:
        K.set_cu_reserve(prev)
