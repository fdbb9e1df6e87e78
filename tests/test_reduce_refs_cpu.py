"""CPU: the references, case tables and restated launch geometry of tests/reduce_refs.py, checked without a GPU -- against
torch.autograd in fp64, against the exactness bound (2^24) that the bit-equality tests of tests/test_gpu_reduce_exact.py lean on,
against the constants of elementwise.hip, and against four mutated references that the comparisons must tell from the right one."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import reduce_refs as R

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "erd_amd", "csrc", "elementwise.hip")


def _levels_nchw(t, sizes):
    """[N, A, C] -> per-level [N, C, h, w]"""
    return [t[:, sl].reshape(t.shape[0], h, w, t.shape[2]).permute(0, 3, 1, 2) for sl, (h, w) in zip(R.level_slices(sizes), sizes)]


def _flat(t):
    return t.permute(0, 2, 3, 1).reshape(t.shape[0], -1, t.shape[1])


# ---------------------------------------------------------------------------------------------
# the references against torch
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("li", range(len(R.GN_LEVEL_LISTS)))
def test_gn_refs_equal_autograd_fp64(li):
    """F.relu(F.group_norm(...)) per level in fp64 on random non-integer data: forward and all three gradients to 1e-12.
    (One-row levels have a variance of rounding-error size against eps = 1e-5: both formulas agree there to 1e-12 as well.)"""
    sizes, N, Cc = R.GN_LEVEL_LISTS[li], 2, 64
    A = R.total_rows(sizes)
    g = torch.Generator().manual_seed(100 + li)
    c = 0.3 + 2.0 * torch.randn(N, A, Cc, generator=g, dtype=torch.float64)
    gamma, beta = 0.5 + torch.rand(Cc, generator=g, dtype=torch.float64), 0.3 * torch.randn(Cc, generator=g, dtype=torch.float64)
    dy = torch.randn(N, A, Cc, generator=g, dtype=torch.float64)
    eps = R._eps32(R.GN_EPS)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    cls = [t.clone().requires_grad_(True) for t in _levels_nchw(c, sizes)]
    ys = [F.relu(F.group_norm(cl, 8, gr, br, eps)) for cl in cls]
    torch.autograd.backward(ys, _levels_nchw(dy, sizes))
    y_ref, pre = R.gn_fwd_ref(c, gamma, beta, sizes, 8)
    dc, dg, db = R.gn_bwd_ref(c, dy, gamma, pre > 0, sizes, 8)
    assert y_ref.dtype == dc.dtype == torch.float64
    for sl, yl, cl in zip(R.level_slices(sizes), ys, cls):
        assert R.relerr(y_ref[:, sl], _flat(yl.detach())) < 1e-12
        assert R.relerr(dc[:, sl], _flat(cl.grad)) < 1e-12
    assert R.relerr(dg, gr.grad) < 1e-12 and R.relerr(db, br.grad) < 1e-12
    mr = R.gn_stats_ref(c, sizes, 8)
    for i, cl in enumerate(cls):
        blk = cl.detach().reshape(N, 8, -1)
        assert R.relerr(mr[:, i, :, 0], blk.mean(2)) < 1e-12
        assert R.relerr(mr[:, i, :, 1], 1.0 / torch.sqrt(blk.var(2, unbiased=False) + eps)) < 1e-12


def test_relu_and_colsum_refs_equal_plain_torch():
    g = torch.Generator().manual_seed(7)
    y, dy = torch.randn(3, 5, 7, 12, generator=g), torch.randn(3, 5, 7, 12, generator=g)
    y[0, 0, 0, :4] = torch.tensor([0.0, -0.0, 1.0, -1.0])
    dz, cs = R.relu_bwd_colsum_ref(y, dy, True)
    assert torch.equal(dz, dy * (y > 0)) and dz.dtype == dy.dtype                     # equal as numbers (the product's zeros may be -0)
    assert not bool(torch.signbit(dz[~(y > 0)]).any())                                # the reference's are +0
    assert torch.allclose(cs, (dy.double() * (y > 0)).sum((0, 1, 2)), rtol=1e-13, atol=0) and cs.dtype == torch.float64
    dz, cs = R.relu_bwd_colsum_ref(None, dy, False)
    assert dz is dy and torch.allclose(cs, dy.double().sum((0, 1, 2)), rtol=1e-13, atol=0)
    x = torch.randn(4, 9, 70, generator=g)
    assert torch.allclose(R.colsum_ref(x), x.double().sum((0, 1)), rtol=1e-13, atol=0)
    yi = R.relu_y(3, 2, 9, 11, 8)
    zeros = yi.view(-1)[yi.view(-1) == 0]
    assert bool(torch.signbit(zeros).any()) and not bool(torch.signbit(zeros).all())  # both +0.0 and -0.0
    assert float(yi.abs().max()) == R.Y_MAX and torch.equal(yi, yi.round())


def test_level_row_index_is_the_level_view():
    for Cc, li, N in R.RELU_STRIDED:
        sizes = R.GN_LEVEL_LISTS[li]
        A = R.total_rows(sizes)
        buf = R.ints(50 + li, -R.DY_MAX, R.DY_MAX, N, A, 4)
        for sl in R.level_slices(sizes):
            idx = R.level_row_index(N, A, sl.start, sl.stop - sl.start)
            assert torch.equal(buf.view(N * A, 4)[idx], buf[:, sl].reshape(-1, 4))


# ---------------------------------------------------------------------------------------------
# exactness
# ---------------------------------------------------------------------------------------------
def test_exact_sum_cases_stay_exact():
    """the largest partial sum each bit-equality test can form: an integer below 2^24 is exact in fp32 whatever the order of the
    additions.  bf16 maps hold the INPUTS (and dz, a selection of them); every sum is accumulated and stored in fp32."""
    for Cc in R.RELU_DENSE_CS:
        for N, H, W in R.relu_dense_maps(Cc):
            assert R.relu_colsum_max_partial_sum(N * H * W) < R.F32_EXACT
    for Cc, li, N in R.RELU_STRIDED:
        assert R.relu_colsum_max_partial_sum(N * max(h * w for h, w in R.GN_LEVEL_LISTS[li])) < R.F32_EXACT
    assert R.relu_colsum_max_partial_sum(2 * 67 * 93) == 8 + 12462 * 3
    for rows in R.COLSUM_ROWS + (R.COLSUM_LONG[0],):
        assert R.colsum_max_partial_sum(rows) < R.F32_EXACT
    assert R.colsum_max_partial_sum(131073) == 393219
    for sizes in R.GN_LEVEL_LISTS:
        assert R.gn_stats_max_partial_sum(sizes) < R.F32_EXACT
        assert R.gn_dbeta_max_partial_sum(sizes, max(R.GN_NS)) < R.F32_EXACT
    assert R.gn_stats_max_partial_sum(R.GN_LEVEL_LISTS[0]) == 1050 * 8 * 16
    assert max(R.C_MAX, R.DY_MAX, R.Y_MAX, R.PRELOAD_MAX) <= R.BF16_EXACT
    for li in range(len(R.GN_LEVEL_LISTS)):
        c = R.gn_int_c(li, 3)
        assert torch.equal(c, c.round()) and float(c.abs().max()) == R.C_MAX and torch.equal(c, c.bfloat16().float())
    # gamma in {0.5, 1, 2, -1}, beta = 0: fused and unfused affine give the same bits, so the apply test can demand them
    c, gamma = R.gn_int_c(3, 3), R.gn_pow2_gamma()
    assert set(gamma.tolist()) == set(R.GN_POW2_GAMMAS)
    mr = R.gn_stats_ref(c, R.GN_LEVEL_LISTS[3]).float()
    a, b = (R.gn_apply_f32(c, mr, gamma, torch.zeros(R.GN_C), R.GN_LEVEL_LISTS[3], fused=f) for f in (False, True))
    assert R.same_bits(a, b) and 0.2 < float((a > 0).float().mean()) < 0.8


def test_one_row_levels_have_zero_variance_groups():
    eps = R._eps32(R.GN_EPS)
    for li in (4, 5):
        sizes = R.GN_LEVEL_LISTS[li]
        lvl = [h * w for h, w in sizes].index(1)
        mr = R.gn_stats_ref(R.gn_int_c(li, 3), sizes)
        assert torch.equal(mr[:, lvl, ::2, 1], torch.full((3, R.GN_G // 2), 1.0 / eps ** 0.5, dtype=torch.float64))
        assert bool((mr[:, lvl, 1::2, 1] < 10.0).any())                               # the odd groups have a variance
    # eps travels through the C ABI as a float and is widened there; that is the eps of the reference.  It matters: the fp32 rstd
    # of a zero variance is one ulp above what the double 1e-5 would give
    assert (float(torch.tensor(1.0 / eps ** 0.5).float()), float(torch.tensor(1.0 / 1e-5 ** 0.5).float())) == \
        (316.227783203125, 316.2277526855469)


# ---------------------------------------------------------------------------------------------
# the branch each case is there for
# ---------------------------------------------------------------------------------------------
def test_constants_match_the_source():
    src = open(SRC).read()
    for needle in ("GN_ROWS = 128", "GN_STAT_ROWS = 512", "rpb = 64"):
        assert needle in src, needle
    assert re.search(r"int want = [^;\n]*: 512;", src)                                   # (512 unless the tuning variable is set)
    assert (R.GN_ROWS, R.GN_STAT_ROWS, R.RELU_WANT, R.COLSUM_RPB) == (128, 512, 512, 64)
    assert re.search(r"rpb - 1\) / rpb > 2048\) rpb \*= 2", src) and R.COLSUM_MAX_WGS == 2048
    assert "r + 48 < r1; r += 64" in src and "r + 16 < r1; r += 32" in src and "r + 3 * lanes < r_end; r += 4 * lanes" in src
    assert "unit = 4 * lanes" in src and "C4 % 16 == 0 ? 16 : C4" in src
    assert re.search(r"#define ERD_MAX_SEG\s+5", open(os.path.join(os.path.dirname(SRC), "..", "..", "include", "erd_hip.h")).read())
    assert all(len(s) <= R.MAX_SEG for s in R.GN_LEVEL_LISTS)


def test_relu_cases_reach_their_branches():
    geo = {Cc: R.relu_geometry(1, Cc) for Cc in R.RELU_DENSE_CS}
    assert [(g["cw4"], g["gy"], g["lanes"], g["unit"]) for g in geo.values()] == \
        [(1, 1, 256, 1024), (2, 1, 128, 512), (8, 1, 32, 128), (16, 1, 16, 64), (16, 2, 16, 64), (16, 4, 16, 64), (16, 32, 16, 64)]
    for Cc in R.RELU_DENSE_CS:
        unit = geo[Cc]["unit"]
        maps = R.relu_dense_maps(Cc)
        npix = [N * H * W for N, H, W in maps]
        assert npix[:4] == [1, unit - 1, unit, unit + 1]
        assert all(N >= 2 for (N, H, W), n in zip(maps, npix) if n > 1 and any(n % p == 0 for p in (2, 3, 5, 7)))
        g = [R.relu_geometry(n, Cc) for n in npix]
        assert [(x["wgs"], x["last"]) for x in g[:4]] == [(1, 1), (1, unit - 1), (1, unit), (2, 1)]
        assert all(x["rpb"] == unit for x in g[:4])
        # one row: tail only.  unit - 1: every lane but the last has the four rows of one unrolled pass, the last one has three.
        # unit: the unrolled loop ends exactly at the boundary.  unit + 1: a second workgroup with one row and idle lanes
        assert R.relu_paths(1, Cc) == {"tail", "idle"} and R.relu_paths(unit - 1, Cc) == {"unrolled", "tail"}
        assert R.relu_paths(unit, Cc) == {"unrolled"} and R.relu_paths(unit + 1, Cc) == {"unrolled", "tail", "idle"}
        assert g[4]["wgs"] >= 3 and g[4]["last"] % g[4]["rpb"] != 0                    # several workgroups, ragged last one
    big = {Cc: R.relu_geometry(N * H * W, Cc) for Cc, (N, H, W) in R.RELU_BIG.items()}
    assert [(b["rpb"], b["wgs"], b["last"]) for b in big.values()] == \
        [(1024, 3, 952), (512, 3, 310), (128, 4, 58), (128, 260, 122), (64, 4, 6), (128, 98, 46), (64, 3, 26)]
    assert R.lane_rows(122, 16) == [8] * 10 + [7] * 6 and "unrolled+tail" in R.relu_paths(2 * 131 * 127, 64)
    assert R.lane_rows(952, 256) == [4] * 184 + [3] * 72                              # C = 4: unrolled and tail lanes in one workgroup
    # the `want / gy` row ranges: 512 / gy ranges of rows, so C = 256 and C = 2048 round rpb up from 98 and 10 rows
    assert [R.cdiv(n, R.RELU_WANT // gy) for n, gy in ((12462, 4), (154, 32))] == [98, 10]
    for Cc in R.RELU_REFUSED_CS:
        assert R.relu_geometry(100, Cc) is None
    # strided: every level view's image stride (A * C) differs from its own rows * C
    for Cc, li, N in R.RELU_STRIDED:
        sizes = R.GN_LEVEL_LISTS[li]
        assert len(sizes) > 1 and all(R.relu_geometry(N * h * w, Cc) is not None for h, w in sizes)
        assert all(R.total_rows(sizes) != h * w for h, w in sizes)
    g = [R.relu_geometry(3 * h * w, 256) for h, w in R.GN_LEVEL_LISTS[0]]
    assert [(x["rpb"], x["wgs"], x["last"]) for x in g] == [(64, 50, 14), (64, 13, 51), (64, 4, 39), (64, 2, 8), (64, 1, 18)]
    # workgroups of 64 rows cross image boundaries at other places than multiples of 64: the division is exercised inside a workgroup
    assert all((h * w) % 64 for h, w in R.GN_LEVEL_LISTS[0])


def test_colsum_cases_reach_their_branches():
    assert [R.colsum_geometry(r, 4)["wgs"] for r in R.COLSUM_ROWS] == [1, 1, 1, 2, 65]
    assert [R.colsum_geometry(r, 4)["last"] for r in R.COLSUM_ROWS] == [1, 63, 64, 1, 1]
    assert all(R.colsum_geometry(r, 4)["rpb"] == 64 for r in R.COLSUM_ROWS)
    assert [R.colsum_geometry(1, Cc)["column_passes"] for Cc in R.COLSUM_CS] == [1, 1, 1, 1, 2, 4]
    assert 70 % 4 == 2 and 1000 % 256 != 0 and 260 % 256 == 4
    rows, Cc = R.COLSUM_LONG
    assert R.cdiv(rows, 64) == 2049 > R.COLSUM_MAX_WGS
    g = R.colsum_geometry(rows, Cc)
    assert g["rpb"] == 128 and (g["wgs"], g["last"]) == (1025, 1)
    assert R.colsum_geometry(rows - 1, Cc)["rpb"] == 64


def test_groupnorm_cases_reach_their_branches():
    L = R.GN_LEVEL_LISTS
    assert [R.level_chunks(s, R.GN_STAT_ROWS) for s in L] == [
        [(3, 26), (1, 273), (1, 77), (1, 24), (1, 6)], [(1, 512)], [(2, 1)], [(1, 17), (1, 33), (1, 49), (1, 64), (1, 65)],
        [(1, 256), (1, 1)], [(1, 1), (1, 129)]]
    assert [R.level_chunks(s, R.GN_ROWS) for s in L] == [
        [(9, 26), (3, 17), (1, 77), (1, 24), (1, 6)], [(4, 128)], [(5, 1)], [(1, 17), (1, 33), (1, 49), (1, 64), (1, 65)],
        [(2, 128), (1, 1)], [(1, 1), (2, 1)]]
    # the fourth list: rows per row lane on both sides of each unroll boundary
    assert [R.lane_rows(h * w, 16)[:2] for h, w in L[3]] == [[2, 1], [3, 2], [4, 3], [4, 4], [5, 4]]
    assert R.gn_stat_paths(L[3], R.GN_STATS_UNROLL) == [
        {"tail"}, {"tail"}, {"unrolled", "tail"}, {"unrolled"}, {"unrolled+tail", "unrolled"}]
    assert R.gn_stat_paths(L[3], R.GN_BWD_STATS_UNROLL) == [
        {"unrolled", "tail"}, {"unrolled+tail", "unrolled"}, {"unrolled", "unrolled+tail"}, {"unrolled"}, {"unrolled+tail", "unrolled"}]
    assert R.gn_stat_paths(L[2], R.GN_STATS_UNROLL) == [{"unrolled", "tail", "idle"}]        # 513: a chunk of one row
    assert R.gn_stat_paths(L[4], R.GN_STATS_UNROLL)[1] == {"tail", "idle"}
    assert all(n % 2 for n in R.GN_NS) and 3 in R.GN_NS                                      # odd N


# ---------------------------------------------------------------------------------------------
# the adversarial beta
# ---------------------------------------------------------------------------------------------
def _adversarial(li, N=3):
    sizes = R.GN_LEVEL_LISTS[li]
    c, gamma, _ = R.gn_random_inputs(li, N)
    mr = R.gn_stats_ref(c, sizes).float()
    beta, targets = R.adversarial_beta(c, mr, gamma, sizes)
    return sizes, c, gamma, mr, beta, targets


@pytest.mark.parametrize("li", R.GN_MASK_LISTS)
def test_adversarial_beta_separates_the_two_evaluation_orders(li):
    """a condition on the INPUTS of the mask-agreement test: at the constructed elements the unfused affine is exactly 0 and the fused
    one (exact product + beta, rounded once) is positive for at least a quarter of them"""
    sizes, c, gamma, mr, beta, (n, row, ch) = _adversarial(li)
    assert torch.equal(ch, torch.arange(R.GN_C)) and len(set(zip(n.tolist(), row.tolist()))) == 3 * len(sizes)
    unfused = R.gn_pre_f32(c, mr, gamma, beta, sizes, fused=False)[n, row, ch]
    fused = R.gn_pre_f32(c, mr, gamma, beta, sizes, fused=True)[n, row, ch]
    assert torch.equal(unfused, torch.zeros(R.GN_C))
    share = float(((fused > 0) != (unfused > 0)).float().mean())
    print(f"list {li}: fused affine positive at {share:.3f} of the constructed elements")
    assert share >= 0.25
    dy = R.gn_mask_dy(1, c.shape, (n, row, ch))
    assert float(dy[n, row, ch].abs().min()) >= 1 and float(dy.abs().max()) == R.DY_MAX


# ---------------------------------------------------------------------------------------------
# sensitivity: each mutated reference makes the comparison of the GPU test fail
# ---------------------------------------------------------------------------------------------
def test_dropping_the_last_row_of_a_level_is_noticed():
    for li in range(len(R.GN_LEVEL_LISTS)):
        sizes, N = R.GN_LEVEL_LISTS[li], 3
        c = R.gn_int_c(li, N)
        dy = R.ints(60 + li, 1, R.DY_MAX, N, R.total_rows(sizes), R.GN_C)               # (no zeros: every row counts)
        mr = R.gn_stats_ref(c, sizes).float()
        for lvl, sl in enumerate(R.level_slices(sizes)):
            cut, dcut = c.clone(), dy.clone()
            cut[:, sl.stop - 1] = 0                                                    # the sums of a kernel that skips the row
            dcut[:, sl.stop - 1] = 0
            if float(c[:, sl.stop - 1].abs().sum()) > 0:
                assert int(R.ulp_distance(R.gn_stats_ref(cut, sizes).float(), mr).max()) > 1, (li, lvl)
            assert not torch.equal(R.colsum_ref(dcut).float(), R.colsum_ref(dy).float())
            view = dy[:, sl]                                                           # the strided ReLU-backward column sum
            assert not torch.equal(R.relu_bwd_colsum_ref(None, dcut[:, sl], False)[1], R.relu_bwd_colsum_ref(None, view, False)[1])
            mask = torch.ones(c.shape, dtype=torch.bool)
            assert not torch.equal(R.gn_bwd_ref(c, dcut, torch.ones(R.GN_C), mask, sizes)[2],
                                   R.gn_bwd_ref(c, dy, torch.ones(R.GN_C), mask, sizes)[2])      # dbeta


def test_the_next_groups_statistics_are_noticed():
    for li in (0, 3):
        sizes = R.GN_LEVEL_LISTS[li]
        c, gamma, zero = R.gn_int_c(li, 3), R.gn_pow2_gamma(), torch.zeros(R.GN_C)
        mr = R.gn_stats_ref(c, sizes).float()
        shifted = mr.roll(-1, dims=2)                                                  # group g reads group g + 1
        assert int(R.ulp_distance(shifted, mr).max()) > 1
        assert not R.same_bits(R.gn_apply_f32(c, shifted, gamma, zero, sizes), R.gn_apply_f32(c, mr, gamma, zero, sizes))


def test_a_2x_image_rule_in_the_strided_branch_is_noticed():
    """row r -> image r / (2 * rows) instead of r / rows: the rows of the images behind the first are read from the wrong place"""
    for Cc, li, N in R.RELU_STRIDED:
        if N == 1:
            continue                                                                   # one image: every rule says image 0
        sizes = R.GN_LEVEL_LISTS[li]
        A = R.total_rows(sizes)
        buf = R.ints(70 + li, -R.DY_MAX, R.DY_MAX, N, A, Cc).view(N * A, Cc)
        for sl in R.level_slices(sizes):
            rows = sl.stop - sl.start
            right = R.level_row_index(N, A, sl.start, rows)
            wrong = R.level_row_index(N, A, sl.start, rows, img_of=lambda r, n: r // (2 * n))
            assert not torch.equal(R.colsum_ref(buf[wrong]).float(), R.colsum_ref(buf[right]).float()), (Cc, li, sl)


@pytest.mark.parametrize("li", R.GN_MASK_LISTS)
def test_a_mask_from_the_other_evaluation_order_is_noticed(li):
    """forward with the fused affine, backward mask from the unfused one: dbeta is off by whole dy's and dc at the constructed
    elements by whole dy * gamma * rstd -- far past the 1e-4 of the level's largest |dc| that the GPU test allows"""
    sizes, c, gamma, mr, beta, (n, row, ch) = _adversarial(li)
    dy = R.gn_mask_dy(1, c.shape, (n, row, ch))
    y = R.gn_apply_f32(c, mr, gamma, beta, sizes, fused=True)
    other = R.gn_pre_f32(c, mr, gamma, beta, sizes, fused=False) > 0
    assert int(((y > 0) != other).sum()) >= R.GN_C // 4
    dc, _, db = R.gn_bwd_ref(c, dy, gamma, y > 0, sizes)
    dc_o, _, db_o = R.gn_bwd_ref(c, dy, gamma, other, sizes)
    assert not torch.equal(db.float(), db_o.float())
    flipped = ((y > 0) != other)[n, row, ch]
    level_max = torch.stack([dc[:, sl].abs().max() for sl in R.level_slices(sizes)])
    lvl = torch.tensor([next(i for i, sl in enumerate(R.level_slices(sizes)) if sl.start <= r < sl.stop) for r in row.tolist()])
    err = (dc - dc_o)[n, row, ch].abs() / level_max[lvl]
    assert bool((err[flipped] > 1e-4).all()) and int(flipped.sum()) >= R.GN_C // 4
