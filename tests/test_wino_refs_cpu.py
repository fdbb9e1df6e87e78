"""CPU: the references, inputs, case tables and the restated block cover of tests/wino_refs.py, checked without a GPU -- the
exactness conditions that the bit-equality tests of tests/test_gpu_wino_exact.py lean on (integer U and V that one bf16 limb holds,
every sum below 2^24), a census of the block shapes the sweep reaches, the cover against winograd.hip's own text, and the input
condition of the large mean-to-std test."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import reduce_refs as R
import wino_refs as Wr

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "erd_amd", "csrc", "winograd.hip")
ROWS = range(1, Wr.SWEEP_H + 1)


def _all_forms_cases():
    return [(H0,) + c for H0 in ROWS for c in Wr.forms_cases(H0)]


# ---------------------------------------------------------------------------------------------
# the references against torch
# ---------------------------------------------------------------------------------------------
def test_conv_and_gradient_refs_equal_plain_torch():
    sizes, N, Cin, Cout = [(5, 7), (1, 1), (4, 3)], 2, 6, 10
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, R.total_rows(sizes), Cin, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, 3, 3, Cin, generator=g, dtype=torch.float64)
    dy = torch.randn(N, R.total_rows(sizes), Cout, generator=g, dtype=torch.float64)
    c, dx = Wr.conv_ref(x, w, sizes), Wr.dgrad_ref(dy, w, sizes)
    assert c.dtype == dx.dtype == torch.float64
    for sl, (h, ww) in zip(R.level_slices(sizes), sizes):
        xl = x[:, sl].reshape(N, h, ww, Cin).permute(0, 3, 1, 2).clone().requires_grad_(True)
        yl = F.conv2d(xl, w.permute(0, 3, 1, 2), None, 1, 1)
        yl.backward(dy[:, sl].reshape(N, h, ww, Cout).permute(0, 3, 1, 2))
        assert torch.allclose(c[:, sl], yl.detach().permute(0, 2, 3, 1).reshape(N, -1, Cout), rtol=1e-13, atol=1e-13)
        assert torch.allclose(dx[:, sl], xl.grad.permute(0, 2, 3, 1).reshape(N, -1, Cin), rtol=1e-13, atol=1e-13)
    # the transform matrices give the convolution: sum over cin of U * V, then A^T M A, tile by tile
    U, V = Wr.wino_U(w), Wr.wino_V(x, sizes)
    AT = torch.tensor([[1.0, 1.0, 1.0, 0.0], [0.0, 1.0, -1.0, -1.0]], dtype=torch.float64)
    for sl, (h, ww), v in zip(R.level_slices(sizes), sizes, V):
        TH, TW = (h + 1) // 2, (ww + 1) // 2
        y = torch.einsum("ij,notjk,lk->notil", AT, torch.einsum("ocjk,nctjk->notjk", U, v), AT)       # [N, Cout, tiles, 2, 2]
        y = y.reshape(N, Cout, TH, TW, 2, 2).permute(0, 2, 4, 3, 5, 1).reshape(N, 2 * TH, 2 * TW, Cout)[:, :h, :ww]
        assert torch.allclose(y.reshape(N, -1, Cout), c[:, sl], rtol=1e-12, atol=1e-12)


# ---------------------------------------------------------------------------------------------
# the cover
# ---------------------------------------------------------------------------------------------
def test_the_cover_is_a_partition_of_every_map():
    """every pixel of every map of the sweep (and of the multi-scale lists) is stored by exactly one block; a block never reaches
    beyond its 32 tiles"""
    maps = [(H, W) for H in ROWS for W in range(1, Wr.SWEEP_W + 1)] + [s for l in Wr.MS_LISTS for s in l]
    for H, W in maps:
        count = torch.zeros(H, W, dtype=torch.int32)
        rects = Wr.stored(H, W)
        assert len(rects) == Wr.blocks_per_image(H, W)
        for code, y0, y1, x0, x1 in rects:
            assert (y1 - y0) <= 2 * (32 >> code) and (x1 - x0) <= 2 * (1 << code)
            count[y0:y1, x0:x1] += 1
        assert bool((count == 1).all()), (H, W)
        assert len(Wr.cover(H, W)) <= 3


def test_the_cover_restates_the_source():
    src = open(SRC).read()
    for needle in ("const int nby = TH / 4, nbx = TW / 8;", "add_region(s, g.N, 0, 0, nby, nbx, 3, 4 * nby, 8 * nbx);",
                   "const int bh = rb <= 2 ? 2 : 4, bw = 32 / bh;",
                   "add_region(s, g.N, 4 * nby, 0, 1, (TW + bw - 1) / bw, bw == 16 ? 4 : 3, TH, TW);",
                   "if (cbw > 0 && nby > 0) {", "const int bw = cbw <= 2 ? 2 : cbw <= 4 ? 4 : 8, bh = 32 / bw;",
                   "add_region(s, g.N, 0, 8 * nbx, (4 * nby + bh - 1) / bh, 1, bw == 2 ? 1 : bw == 4 ? 2 : 3, 4 * nby, TW);",
                   "const int TH = (g.IH + 1) / 2, TW = (g.IW + 1) / 2;", "blocks += N * nby * nbx;",
                   "it.y0 = __builtin_amdgcn_readfirstlane(2 * (rg.ty0 + by * (32 >> lbw)));",
                   "it.x0 = __builtin_amdgcn_readfirstlane(2 * (rg.tx0 + (bx << lbw)));",
                   "it.yl = __builtin_amdgcn_readfirstlane(min(p.seg[rg.seg].H, 2 * rg.ty1));",
                   "it.xl = __builtin_amdgcn_readfirstlane(min(p.seg[rg.seg].W, 2 * rg.tx1));",
                   "return (size_t)d.blocks_per_nb * (Cout / BNP) * 32 * sizeof(float);"):
        assert needle in src, needle
    assert re.search(r"constexpr int BN = 64\b", src) and re.search(r"constexpr int BNP = 128\b", src)
    assert re.search(r"constexpr int MAXREG = 16\b", src) and 3 * Wr.MAX_SEG <= 16
    assert (Wr.BN, Wr.BNP, Wr.GN_PART_FLOATS) == (64, 128, 32)
    # a few covers by hand.  18 x 34: 9 x 17 tiles = two rows of two 4x8 blocks, a 2x16 bottom strip of one tile row, a 16x2 right strip
    assert [(r["kind"], r["nby"], r["nbx"], r["code"]) for r in Wr.cover(18, 34)] == \
        [("interior", 2, 2, 3), ("bottom", 1, 2, 4), ("right", 1, 1, 1)]
    assert [(r["kind"], r["nby"], r["nbx"], r["code"]) for r in Wr.cover(1, 1)] == [("bottom", 1, 1, 4)]
    assert [(r["kind"], r["nby"], r["nbx"], r["code"]) for r in Wr.cover(14, 22)] == \
        [("interior", 1, 1, 3), ("bottom", 1, 2, 3), ("right", 1, 1, 2)]
    assert Wr.items_per_image(18, 34, 256, 64) == 7 * 4 and Wr.items_per_image(18, 34, 256, 128) == 7 * 2
    assert Wr.items_per_image(18, 34, 70, 64) == 7 * 2
    assert Wr.region_block0([(18, 34), (1, 1)], 2) == [(0, "interior", 0), (0, "bottom", 8), (0, "right", 12), (1, "bottom", 14)]
    assert Wr.list_blocks([(18, 34), (1, 1)], 2) == 16


def test_the_sweep_is_what_it_claims():
    """every (H, W) with 1 <= H <= 18, 1 <= W <= 34 exactly once, five maps to a launch; every combination of TH % 4, TW % 8, interior
    rows or none, interior columns or none; every block-shape code; partial tiles in both directions; launches whose regions start
    at a block0 > 0 for every region kind"""
    seen, keys, codes, kinds_behind = [], set(), set(), set()
    for H0 in ROWS:
        lists = Wr.sweep_lists(H0)
        assert len(lists) == Wr.SWEEP_LISTS_PER_H and all(1 <= len(s) <= Wr.MAX_SEG for s in lists)
        assert sum(len(s) for s in lists) == Wr.SWEEP_W
        for s in lists:
            seen += s
            kinds_behind |= {kind for _, kind, b0 in Wr.region_block0(s, Wr.SWEEP_N) if b0 > 0}
            assert len({h for h, _ in s}) > 1 and len({w for _, w in s}) == len(s)
    assert sorted(seen) == [(H, W) for H in ROWS for W in range(1, Wr.SWEEP_W + 1)]
    for H, W in seen:
        keys.add(Wr.census_key(H, W))
        codes |= {r["code"] for r in Wr.cover(H, W)}
    # (a remainder of 0 without an interior row / column would be a map without tiles: every combination that exists)
    assert keys == {(a, b, c, d) for a in range(4) for b in range(8) for c in (False, True) for d in (False, True)
                    if (a or c) and (b or d)}
    assert len(keys) == 128 - 16 - 8 + 1
    assert codes == {1, 2, 3, 4}
    assert any(H % 2 for H, _ in seen) and any(W % 2 for _, W in seen) and any(H % 2 and W % 2 for H, W in seen)
    assert kinds_behind == {"interior", "bottom", "right"}
    # the multi-scale lists: (608, 1024) gives the list the RandomResize pipeline prints; both ends of the range are there
    assert Wr.fpn_sizes(608, 1024) == [(76, 128), (38, 64), (19, 32), (10, 16), (5, 8)]
    assert Wr.MS_LISTS[0][0] == (60, 80) and Wr.MS_LISTS[-1] == [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]
    assert all(480 <= h <= 800 and w <= 1344 and h % 32 == 0 and w % 32 == 0 for h, w in Wr.MS_BATCHES)
    # every case of the forms test appears once; the Cin = 256 list and the five multi-scale lists are among them
    cases = _all_forms_cases()
    assert sum(1 for c in cases if c[3] == 256) == 1 and sum(1 for c in cases if c[2] == 1) == len(Wr.MS_LISTS)
    for H0 in ROWS:
        g = Wr.gn_cases(H0)
        assert {(N, Cin) for _, N, Cin in g} == {(1, 64), (3, 64), (1, 256), (3, 256)}
    assert {(N, Cin) for _, N, Cin in Wr.GN_MS_CASES} >= {(1, 64), (3, 64), (1, 256)}
    assert len({tuple(s) for s, _, _ in Wr.GN_MS_CASES} & {tuple(s) for s in Wr.MS_LISTS[1:4]}) == 3


# ---------------------------------------------------------------------------------------------
# exactness
# ---------------------------------------------------------------------------------------------
def _check_limb_exact(x, w, sizes, Cin):
    U = Wr.wino_U(w)
    assert torch.equal(U, U.round()) and torch.equal(U.float().bfloat16().double(), U)
    vmax = 0.0
    for V in Wr.wino_V(x, sizes):
        assert torch.equal(V, V.round()) and torch.equal(V.float().bfloat16().double(), V)
        vmax = max(vmax, float(V.abs().max()))
    # the 16 GEMMs' partial sums, and the 3 x 3 of them the two output-transform stages add per pixel
    assert 9 * Cin * float(U.abs().max()) * vmax < R.F32_EXACT
    return float(U.abs().max()), vmax


@pytest.mark.parametrize("H0", ROWS)
def test_forms_cases_stay_exact(H0):
    """U and V are integers one bf16 limb holds, Cin * max|U| * max|V| < 2^24 (with the output transform's factor 9 to spare), the
    same for the input-gradient form (the transposed weights; dy in {-1, 0, 1}), per-column sums of |values| < 2^24, and the data do
    something: most outputs are non-zero"""
    for sizes, N, Cin in Wr.forms_cases(H0):
        case = Wr.conv_case(sizes, N, Cin, Wr.BNP)
        f = Wr.forms_refs(case)
        x, w, c = case["x"], case["w"], case["c"]
        assert set(x.unique().tolist()) <= {-1.0, 0.0, 1.0} and set(w.unique().tolist()) <= {-4.0, 0.0, 4.0}
        umax, vmax = _check_limb_exact(x, w, sizes, Cin)
        assert umax <= 9 and vmax <= 4
        _check_limb_exact(f["dy"], w.permute(3, 1, 2, 0).contiguous(), sizes, Wr.BNP)
        assert float(f["colsum_abs"].max()) < R.F32_EXACT
        assert float(c.abs().max()) + Wr.RES_MAX < 2 ** 8 and set(f["scale"].tolist()) == set(Wr.BN_SCALES)
        assert torch.equal(f["shift"], f["shift"].round()) and torch.equal(f["res"], f["res"].round())
        assert set(f["mask"].unique().tolist()) == {-1.0, 1.0}
        if case["A"] * N >= 64:
            assert float((c != 0).float().mean()) > 0.5 and float((f["out_b"] > 0).float().mean()) > 0.2
            assert float((f["dx"] != 0).float().mean()) > 0.5


def _check_gn_case(sizes, N, Cin):
    case = Wr.conv_case(sizes, N, Cin, Wr.GN_COUT)
    c = case["c"]
    _check_limb_exact(case["x"], case["w"], sizes, Cin)
    # an item holds 128 pixels x 8 channels per group; its partial sums (lanes, waves, the four transform rows) are sub-sums of that
    assert Wr.ITEM_PIXELS * 8 * float(c.abs().max()) ** 2 < R.F32_EXACT
    mean, var = Wr.group_moments(c, sizes)
    assert float(var.min()) > 0, (sizes, N, Cin, float(var.min()))
    mr = R.gn_stats_ref(c, sizes)
    assert bool(torch.isfinite(mr).all()) and float(mr[..., 1].max()) < 1.0 / R._eps32(R.GN_EPS) ** 0.5
    # gamma a power of two and beta = 0: both evaluation orders of the affine give the same bits
    gamma, zero = R.gn_pow2_gamma(), torch.zeros(Wr.GN_COUT)
    assert R.same_bits(*(R.gn_apply_f32(c, mr.float(), gamma, zero, sizes, fused=f) for f in (False, True)))


@pytest.mark.parametrize("H0", ROWS)
def test_groupnorm_cases_stay_exact(H0):
    for sizes, N, Cin in Wr.gn_cases(H0):
        _check_gn_case(sizes, N, Cin)


def test_groupnorm_multi_scale_cases_stay_exact():
    for sizes, N, Cin in Wr.GN_MS_CASES:
        _check_gn_case(sizes, N, Cin)
        _check_gn_case(Wr.GN_STALE_SMALL, N, Cin)
    assert Wr.list_blocks(Wr.GN_STALE_SMALL, 1) == 3


# ---------------------------------------------------------------------------------------------
# sensitivity: what the mutated kernels of the issue would compute differs from the reference
# ---------------------------------------------------------------------------------------------
def test_a_pixel_counted_twice_is_noticed():
    """the sums of a kernel that counts one pixel of a level twice (an item that does not mask a pixel of its neighbour's) are more
    than the allowed 1 ulp from the reference, on every level of a sweep list"""
    sizes, N, Cin = Wr.sweep_lists(6)[5], 3, 64
    c = Wr.conv_case(sizes, N, Cin, Wr.GN_COUT)["c"]
    mr = R.gn_stats_ref(c, sizes).float()
    for lvl, sl in enumerate(R.level_slices(sizes)):
        blk = c[:, sl].double().reshape(N, -1, R.GN_G, 8)
        last = c[:, sl.stop - 1].double().reshape(N, R.GN_G, 8)
        m = blk.shape[1] * 8.0
        s1, s2 = blk.sum((1, 3)) + last.sum(2), (blk * blk).sum((1, 3)) + (last * last).sum(2)
        mean = s1 / m
        rstd = 1.0 / torch.sqrt((s2 / m - mean * mean).clamp_min(0.0) + R._eps32(R.GN_EPS))
        got = torch.stack([mean, rstd], -1).float()
        assert int(R.ulp_distance(got, mr[:, lvl]).max()) > 1, (lvl, sizes)


# ---------------------------------------------------------------------------------------------
# the large mean-to-std case
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", Wr.RATIO_TARGETS)
def test_ratio_inputs_reach_their_targets(target):
    """a condition on the INPUTS: the median per-(image, level, group) r = |mean| / std of the fp64 convolution lies within a factor 2
    of the target (target 0: below 1), on every level"""
    x, w, gamma, beta = Wr.ratio_inputs(target)
    assert float(x.min()) >= 0.0
    mean, var = Wr.group_moments(Wr.conv_ref(x, w, Wr.RATIO_SIZES), Wr.RATIO_SIZES)
    r = mean.abs() / var.sqrt()
    med = [float(r.median())] + [float(r[:, i].median()) for i in range(len(Wr.RATIO_SIZES))]
    print(f"target {target}: median r {med[0]:.2f}, per level {[round(v, 2) for v in med[1:]]}, range {float(r.min()):.2f} .. {float(r.max()):.2f}")
    if target == 0:
        assert all(v < 1.0 for v in med)
    else:
        assert all(target / 2 <= v <= 2 * target for v in med), med
        assert bool((mean > 0).any()) and bool((mean < 0).any())             # both signs of the mean
