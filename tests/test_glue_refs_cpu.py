"""CPU: the references and case tables of tests/glue_refs.py, checked without a GPU -- against torch's own operators, and against the
exactness bounds (2^24 in fp32, 256 in bf16) and grid caps that the bit-equality tests of tests/test_gpu_glue_exact.py lean on."""
import pytest
import torch
import torch.nn.functional as F

import glue_refs as R


def _interp_index(H, h):
    """the source index F.interpolate(mode='nearest') picks for each of H destinations: interpolate an arange"""
    src = torch.arange(h, dtype=torch.float32).view(1, 1, h, 1)
    return F.interpolate(src, size=(H, 1), mode="nearest").view(H).long()


def test_nearest_src_is_interpolate_nearest_for_stride2_pairs():
    """every (h, 2h) and (h, 2h-1), h = 1..700: the kernel's integer rule and F.interpolate agree.  (They differ for other pairs --
    (26 <- 44), (30 <- 58), (65 <- 110): see glue_refs.nearest_src -- a known property of the rule, not something to fix.)"""
    for h in range(1, 701):
        for H in {2 * h, max(2 * h - 1, 1)}:
            assert torch.equal(R.nearest_src(H, h), _interp_index(H, h)), (H, h)
    assert [(H, h) for h, H in [(26, 44), (30, 58), (65, 110)] if not torch.equal(R.nearest_src(H, h), _interp_index(H, h))] \
        == [(44, 26), (58, 30), (110, 65)]
    for (H, W), (h, w) in R.UPSAMPLE_PAIRS:        # the two ratio-3 / ragged pairs of the table agree as well
        assert torch.equal(R.nearest_src(H, h), _interp_index(H, h)) and torch.equal(R.nearest_src(W, w), _interp_index(W, w))


def test_shift_by_one_is_the_rule_only_for_stride2_pairs():
    """why the table holds pairs that are not 2x: for (h, 2h) and (h, 2h-1) `y >> 1` is the whole rule, so only another ratio can
    tell the kernel's `y * h / H` from a hard-wired halving"""
    def halved(H, h):
        return torch.equal(R.nearest_src(H, h), torch.arange(H) >> 1)
    pairs = R.UPSAMPLE_PAIRS
    assert all(halved(H, h) and halved(W, w) for (H, W), (h, w) in pairs[:6])
    assert all(not halved(H, h) and not halved(W, w) for (H, W), (h, w) in pairs[6:]) and len(pairs) > 6


def _all_upsample_cases():
    cases = [(R.UPSAMPLE_N, HW, hw, R.UPSAMPLE_C) for HW, hw in R.UPSAMPLE_PAIRS]
    return cases + [(R.UPSAMPLE_N,) + R.UPSAMPLE_STRIDED + (R.UPSAMPLE_C,), R.UPSAMPLE_BIG, R.UPSAMPLE_BIG_BWD]


@pytest.mark.parametrize("N,HW,hw,Cc", [(1, HW, hw, 4) for HW, hw in R.UPSAMPLE_PAIRS] + [(1, (100, 168), (50, 84), 4)])
def test_upsample_refs_equal_interpolate_and_its_autograd(N, HW, hw, Cc):
    g = torch.Generator().manual_seed(HW[0] * 1000 + HW[1])
    fine = torch.randint(-8, 9, (N, *HW, Cc), generator=g).double()
    coarse = torch.randint(-8, 9, (N, *hw, Cc), generator=g).double()
    cr = coarse.permute(0, 3, 1, 2).clone().requires_grad_(True)
    up = F.interpolate(cr, size=HW, mode="nearest")
    assert torch.equal(R.upsample_add_ref(fine, coarse), fine + up.detach().permute(0, 2, 3, 1))
    up.backward(fine.permute(0, 3, 1, 2))
    assert torch.equal(R.upsample_add_bwd_ref(fine, coarse), coarse + cr.grad.permute(0, 2, 3, 1))


@pytest.mark.parametrize("rnd", [0, 1, 2])
def test_stem_ref_with_delta_weights_is_a_gather(rnd):
    x, scale, shift = R.stem_exact_inputs(2, 19, 37)
    got = R.stem_ref(x, R.delta_weights(rnd), scale, shift)
    OH, OW = R.conv_out(19, 7, 2, 3), R.conv_out(37, 7, 2, 3)
    assert got.shape == (2, OH, OW, 64) and got.dtype == torch.float64
    xp = F.pad(x, (3, 3, 3, 3)).double()
    for co, (ci, kh, kw) in enumerate(R.delta_taps(rnd)):
        px = xp[:, ci, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2]
        assert torch.equal(got[..., co], torch.relu(px * float(scale[co]) + float(shift[co]))), co
    assert torch.equal(got, got.float().double())                                 # exact in fp32 too


def test_delta_weights_cover_every_tap_and_keep_relu_busy():
    cover = sum(R.delta_weights(r) for r in range(3)).sum(0)                      # [ci][kh][kw]: output channels that read the tap
    assert bool((cover >= 1).all()) and all(int(R.delta_weights(r).sum()) == 64 for r in range(3))
    x, scale, shift = R.stem_exact_inputs(1, 19, 37)
    assert set(scale.tolist()) == set(R.STEM_SCALES) and float(shift.abs().max()) == R.STEM_SHIFT_MAX
    assert float(x.abs().max()) == R.STEM_IN_MAX and torch.equal(x, x.round())
    y = R.stem_ref(x, R.delta_weights(0), scale, shift)
    assert 0.2 < float((y == 0).double().mean()) < 0.8                            # both sides of the ReLU are populated


def test_exact_sum_cases_stay_exact():
    """the largest partial sum each bit-equality test can form, from its shapes and value ranges: an integer below 2^24 is exact
    in fp32 whatever the order of the additions, and one up to 256 is exact in bf16"""
    assert R.stem_max_partial_sum() < R.F32_EXACT
    for N, (H, W), (h, w), Cc in _all_upsample_cases():
        m = R.upsample_bwd_max_partial_sum(H, W, h, w)
        assert m < R.BF16_EXACT < R.F32_EXACT, ((H, W), (h, w), m)
    assert R.upsample_bwd_max_partial_sum(10, 14, 5, 7) == 8 + 4 * 8 and R.upsample_bwd_max_partial_sum(6, 9, 2, 3) == 8 + 9 * 8
    for sizes in R.LEVEL_LISTS:
        assert R.level_scale_max_partial_sum(sizes) < R.F32_EXACT, sizes
    assert R.level_scale_max_partial_sum(R.LEVEL_LISTS[0]) == 3 * 1050 * 68 * 9
    assert all(a * R.LEVEL_INT_MAX == float(torch.tensor(a * R.LEVEL_INT_MAX, dtype=torch.float32)) for a in R.LEVEL_ALPHAS)


def test_cases_reach_the_branches_they_are_named_for():
    """launch geometry restated from elementwise.hip: a later change of a cap or a tile size fails here and names the case to move"""
    assert [R.stem_tiles(*s)[:1] + R.stem_tiles(*s)[2:] for s in R.STEM_SHAPES[:3]] == [(20, 1, 20), (612, 2, 100), (1224, 3, 200)]
    assert [R.stem_tiles(*s)[0] for s in R.STEM_SHAPES[3:]] == [2, 1, 1, 1]
    N, H, W, Cc = R.MAXPOOL_BIG
    assert R.blocks_wanted(N * R.conv_out(H, 3, 2, 1) * R.conv_out(W, 3, 2, 1) * Cc // 4) > R.MAXPOOL_CAP
    assert all(R.blocks_wanted(n * ((H + 1) // 2) * ((W + 1) // 2) * c // 4) <= R.MAXPOOL_CAP
               for n in R.MAXPOOL_NS for c in R.MAXPOOL_CS for H, W in R.MAXPOOL_SIZES)
    N, (H, W), (h, w), Cc = R.UPSAMPLE_BIG
    assert R.blocks_wanted(N * H * W * Cc // 4) > R.UPSAMPLE_CAP >= R.blocks_wanted(N * h * w * Cc // 4)
    N, (H, W), (h, w), Cc = R.UPSAMPLE_BIG_BWD
    assert R.blocks_wanted(N * h * w * Cc // 4) > R.UPSAMPLE_CAP
    assert [R.level_chunks(s) for s in R.LEVEL_LISTS] == [[(9, 26), (3, 17), (1, 77), (1, 24), (1, 6)], [(1, 128)], [(2, 1)],
                                                          [(2, 128), (1, 1)]]
    rows, Cc, Cp = R.PAD_BIG
    assert R.blocks_wanted(rows * Cp) > R.PAD_CAP >= R.blocks_wanted(R.PAD_WEIGHT[0] * R.PAD_WEIGHT[2])
    assert [R.blocks_wanted(n // 4) > R.BF16_CAP for n in R.BF16_NS] == [False] * 7 + [True] and R.BF16_NS[-1] % 4 == 3
    assert sorted(n % 4 for n in R.BF16_NS[:6]) == [0, 1, 1, 2, 3, 3]


def test_level_scale_refs_equal_autograd():
    sizes = R.LEVEL_LISTS[0]
    A = sum(h * w for h, w in sizes)
    g = torch.Generator().manual_seed(5)
    x, dy = torch.randn(2, A, 8, generator=g, dtype=torch.float64), torch.randn(2, A, 8, generator=g, dtype=torch.float64)
    al = torch.tensor([0.9, 1.1, 1.3, -0.7, 2.0], dtype=torch.float64, requires_grad=True)
    xr = x.clone().requires_grad_(True)
    y = torch.cat([xr[:, sl] * al[i] for i, sl in enumerate(R.level_slices(sizes))], 1)
    assert torch.equal(R.level_scale_ref(x, al.detach(), sizes), y.detach())
    y.backward(dy)
    dx, dal = R.level_scale_bwd_ref(x, dy, al.detach(), sizes)
    assert torch.equal(dx, xr.grad) and torch.allclose(dal, al.grad, rtol=1e-12, atol=0)


def test_pad_channels_ref():
    src = torch.arange(1.0, 31.0).view(3, 10)
    out = R.pad_channels_ref(src, 12)
    assert out.shape == (3, 12) and torch.equal(out[:, :10], src) and not bool(out[:, 10:].any())
    assert torch.equal(R.pad_channels_ref(src, 10), src)


def test_bf16_edge_values_are_the_edges():
    v, b = R.bf16_edge_values(), R.bf16_edge_bits()
    assert v.dtype == torch.float32 and v.numel() == len(R.BF16_EXPONENTS) * 2 * 2 * 3 * 6 + 6
    assert torch.equal(v.view(torch.int32).long() & 0xFFFFFFFF, b)
    assert not bool(torch.isnan(v).any())
    expo = (b >> 23) & 0xFF
    assert bool(((expo != 0) | ((b & 0x7FFFFFFF) == 0)).all())                    # no denormal
    out = R.bits16(v.to(torch.bfloat16)).long() & 0xFFFF
    kept, tie = b >> 16, (b & 0xFFFF) == 0x8000
    assert bool((tie & (kept & 1 == 0) & (out == kept)).any())                    # tie to even: down ...
    assert bool((tie & (kept & 1 == 1) & (out == kept + 1)).any())                # ... and up
    assert bool((((b & 0xFFFF) == 0x7FFF) <= (out == kept)).all())                # just below the tie: always down
    assert bool((((b & 0xFFFF) == 0x8001) <= (out == kept + 1)).all())            # just above: always up
    finite = torch.isfinite(v)
    assert bool((finite & ((out & 0x7FFF) == 0x7F80)).any())                      # overflow to inf from a finite value
    assert bool((((out >> 7) & 0xFF) == ((expo + 1) & 0xFF)).any())               # a carry into the exponent
