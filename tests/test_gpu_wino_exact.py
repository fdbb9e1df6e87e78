"""GPU: the three Winograd F(2x2,3x3) kernels of winograd.hip (wino_conv_kernel, wino_x3_kernel, wino_x3p_kernel) and the GroupNorm
statistics from wino_x3p_kernel's output stage (gn_part, wino_gn_finalize_kernel, kernels.conv3x3_gn_relu_forward) against the
plain CPU references of tests/wino_refs.py, EXACTLY: with x in {-1, 0, 1} and weights in {-4, 0, 4} every transform, limb, product
and fp32 sum is an integer far below 2^24 (tests/test_wino_refs_cpu.py asserts it on the references), so every output element, every
column sum and every per-item statistic has one right value, whatever the order of the additions.  One pixel stored twice, not at
all, or counted into the wrong sum fails.

The shapes are every (H, W) with 1 <= H <= 18, 1 <= W <= 34 -- every block shape of wino_plan's cover, with and without interior,
bottom strip and right strip, partial tiles in both directions --, five maps to a launch, and the level lists multi-scale training
produces.  The only tolerances in this file: 1 ulp on mean_rstd (one fp64 formula on equal sums, rounded to fp32 on both sides), and,
for the non-integer test at a large mean-to-std ratio, a bound derived from the fp32 roundings of the partial sums."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import reduce_refs as R
import wino_refs as Wr

NAN = float("nan")
ROWS = range(1, Wr.SWEEP_H + 1)


@pytest.fixture(scope="module")
def K():
    from erd_amd import kernels
    assert torch.cuda.is_available()
    return kernels


@pytest.fixture(scope="module")
def lib():
    from erd_amd import _lib
    return _lib.load()


@pytest.fixture()
def wino_p_mode():
    """ERD_WINO_P (read per launch by wino_plan): 0 = items of 64 output channels (wino_x3_kernel), 2 = items of 128 wherever
    Cout % 128 == 0 (wino_x3p_kernel), unset = the launch's own choice"""
    old = os.environ.get("ERD_WINO_P")

    def set_mode(m):
        if m is None:
            os.environ.pop("ERD_WINO_P", None)
        else:
            os.environ["ERD_WINO_P"] = str(m)
    yield set_mode
    set_mode(old)


@pytest.fixture()
def gn_fused(K):
    keep = K.GN_FUSED
    K.GN_FUSED = True
    yield
    K.GN_FUSED = keep


def nans(*shape):
    return torch.full(shape, NAN, device="cuda")


def where(row, sizes):
    for lvl, (sl, (h, w)) in enumerate(zip(R.level_slices(sizes), sizes)):
        if sl.start <= row < sl.stop:
            return f"level {lvl} ({h}x{w}) pixel ({(row - sl.start) // w}, {(row - sl.start) % w})"


def assert_exact(got, want, what, sizes=None):
    """every element equal, none NaN; the message names the first element that differs"""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    if not torch.equal(got, want):
        bad = ~(got == want)
        first = [int(v) for v in bad.nonzero()[0]]
        at = where(first[1], sizes) if sizes is not None and len(first) == 3 else ""
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ ({int(torch.isnan(got).sum())} NaN); first at "
                             f"{first} {at}: got {float(got[tuple(first)])}, want {float(want[tuple(first)])}")


def assert_same_bits(got, want, what):
    assert R.same_bits(got.cpu(), want.cpu()), what


def conv_segs(K, x, out, sizes):
    from erd_amd._lib import ConvSeg
    xs, outs = K.level_views(x, sizes), K.level_views(out, sizes)
    segs = (ConvSeg * len(xs))()
    for i, (a, b) in enumerate(zip(xs, outs)):
        K._fill_seg(segs[i], a, b, a.shape[1], a.shape[2], None, None, None)
    return segs, len(xs)


def couts_per_item(K, lib, x, sizes, Cout):
    out = torch.empty(x.shape[:2] + (Cout,), device="cuda")
    segs, n = conv_segs(K, x, out, sizes)
    return int(lib.erd_wino_x3_couts_per_item(segs, n, Cout))


def gn_ws_bytes(K, lib, x, sizes, Cout):
    out = torch.empty(x.shape[:2] + (Cout,), device="cuda")
    segs, n = conv_segs(K, x, out, sizes)
    return int(lib.erd_wino_x3_gn_ws_bytes(segs, n, Cout))


def launch(K, x, U, out, sizes, **kw):
    views = {k: K.level_views(kw.pop(k), sizes) for k in ("res", "mask") if k in kw}
    K.wino_conv3x3(K.level_views(x, sizes), U, K.level_views(out, sizes), out.shape[2], **views, **kw)


# ---------------------------------------------------------------------------------------------
# 1. all three kernels, all forms, over the sweep
# ---------------------------------------------------------------------------------------------
KERNELS = (("wino_conv_kernel", False, None), ("wino_x3_kernel", True, 0), ("wino_x3p_kernel", True, 2))


def check_forms(K, lib, wino_p_mode, sizes, N, Cin):
    case = Wr.conv_case(sizes, N, Cin, Wr.BNP)
    f = Wr.forms_refs(case)
    A, Cout = case["A"], Wr.BNP
    x, w, c, dy = (t.cuda() for t in (case["x"], case["w"], case["c"], f["dy"]))
    scale, shift, res, mask, out_b, out_c, cs_ref, dx_ref = (f[k].cuda() for k in ("scale", "shift", "res", "mask", "out_b", "out_c", "colsum", "dx"))
    out_r, csr_ref = f["out_r"].cuda(), f["colsum_r"].cuda()
    wt = K.weight_transpose(w)
    assert wt.shape == (Cin, 3, 3, Cout)
    for name, x3, mode in KERNELS:
        what = f"{name} {Cin}->{Cout} N={N} {sizes}"
        wino_p_mode(mode)
        if x3:
            assert couts_per_item(K, lib, x, sizes, Cout) == (128 if mode == 2 else 64), what
        U = K.wino_weights(w, x3=x3)
        runs = []
        for rep in range(2):
            out_a = nans(N, A, Cout)
            launch(K, x, U, out_a, sizes)
            assert_exact(out_a, c, what + ": plain", sizes)
            got_b = nans(N, A, Cout)
            launch(K, x, U, got_b, sizes, scale=scale, shift=shift, relu=True)
            assert_exact(got_b, out_b, what + ": scale, shift, ReLU", sizes)
            got_cs = []
            for copies in (1, 8):
                got_c = res.clone()                                        # the residual aliases the output
                cs = torch.zeros(Cout, device="cuda") if copies == 1 else torch.zeros(copies, Cout, device="cuda")
                launch(K, x, U, got_c, sizes, res=got_c, mask=mask, colsum=cs)
                assert_exact(got_c, out_c, what + f": residual + mask, {copies} column-sum copies", sizes)
                assert_exact(cs.view(copies, Cout).sum(0), cs_ref, what + f": column sums over {copies} copies")
                got_cs.append(cs)
                # ... and without the mask (which is also zero wherever a block reaches beyond the pixels it stores), the residual
                # a tensor of its own
                got_r = nans(N, A, Cout)
                cs = torch.zeros(copies, Cout, device="cuda")
                launch(K, x, U, got_r, sizes, res=res, colsum=cs)
                assert_exact(got_r, out_r, what + f": residual, {copies} column-sum copies", sizes)
                assert_exact(cs.sum(0), csr_ref, what + f": column sums without a mask over {copies} copies")
            runs.append([out_a, got_b, got_c] + got_cs[:1])                # (which copy a workgroup adds into is not fixed)
        for a, b in zip(*runs):
            assert_same_bits(a, b, what + ": second run")
        # the input gradient: the same kernel on dy with the transposed, flipped weights (Cin output channels)
        if mode == 2 and Cin % Wr.BNP:
            continue                                                       # (no items of 128 among Cin output channels)
        if x3:
            assert couts_per_item(K, lib, dy, sizes, Cin) == (128 if mode == 2 else 64), what
        Ut = K.wino_weights(wt, flip=True, x3=x3)
        dxs = []
        for rep in range(2):
            dx = nans(N, A, Cin)
            launch(K, dy, Ut, dx, sizes)
            assert_exact(dx, dx_ref, what + ": input gradient", sizes)
            dxs.append(dx)
        assert_same_bits(dxs[0], dxs[1], what + ": input gradient, second run")
    # output channel counts that are no multiple of 32 / of 4: the first Cout filters of the same weights
    for Cout in Wr.RAGGED_COUTS:
        wr, cr, br = w[:Cout].contiguous(), c[..., :Cout].contiguous(), out_b[..., :Cout].contiguous()
        sc, sh = scale[:Cout].contiguous(), shift[:Cout].contiguous()
        for name, x3, mode in KERNELS[:2]:
            what = f"{name} {Cin}->{Cout} N={N} {sizes}"
            wino_p_mode(mode)
            U = K.wino_weights(wr, x3=x3)
            for rep in range(2):
                out_a = nans(N, A, Cout)
                launch(K, x, U, out_a, sizes)
                assert_exact(out_a, cr, what + ": plain", sizes)
                got_b = nans(N, A, Cout)
                launch(K, x, U, got_b, sizes, scale=sc, shift=sh, relu=True)
                assert_exact(got_b, br, what + ": scale, shift, ReLU", sizes)


@pytest.mark.parametrize("H0", ROWS)
def test_every_kernel_and_form_is_the_integer_convolution(K, lib, wino_p_mode, H0):
    """Row H0 of the sweep (seven launches of five maps, N = 2, 64 -> 128; row 1 also a list at Cin = 256, rows 2-6 a multi-scale
    level list at N = 1), on the fp32 kernel, the three-limb kernel with items of 64 and the one with items of 128 output channels:
    (a) plain into NaN, (b) folded-BN scale / shift + ReLU, (c) a residual that aliases the output + mask + column sums into 1 and
    into 8 copies, and residual + column sums without a mask, (d) the input gradient (Cin output channels: on the kernel with items of 128 that is the Cin = 256 list); then Cout = 80, 68, 70 on the two kernels that serve them, forms (a) and (b).  Every run
    twice, every element equal to the integer reference."""
    for sizes, N, Cin in Wr.forms_cases(H0):
        check_forms(K, lib, wino_p_mode, sizes, N, Cin)


# ---------------------------------------------------------------------------------------------
# 2. fused GroupNorm statistics, exact
# ---------------------------------------------------------------------------------------------
def gn_part_fill(K, nbytes):
    """NaN into the whole gn_part workspace of the current stream (grown to nbytes first)"""
    K.workspace("gn_part", nbytes, torch.device("cuda", torch.cuda.current_device())).view(torch.float32).fill_(NAN)


def run_fused(K, lib, case, refill=True):
    """K.conv3x3_gn_relu_forward on a case's GPU tensors; asserts that the fused path is the one that runs and that the restated
    cover gives the item count the library sizes its workspace for"""
    sizes, N = case["sizes"], case["N"]
    ws = gn_ws_bytes(K, lib, case["xg"], sizes, Wr.GN_COUT)
    assert ws > 0, "the launch does not run on the 128-couts-per-item kernel: nothing fused"
    assert ws == Wr.list_blocks(sizes, N) * Wr.GN_PART_FLOATS * 4 * (Wr.GN_COUT // Wr.BNP)
    assert ws // (Wr.GN_PART_FLOATS * 4) == N * sum(Wr.items_per_image(h, w, Wr.GN_COUT, Wr.BNP) for h, w in sizes)
    if refill:
        gn_part_fill(K, ws)
    c, y, mr = K.conv3x3_gn_relu_forward(case["xg"], case["wg"], case["gamma"], case["beta"], sizes)
    if refill:                                                             # every item wrote its 32 slots
        part = K.workspace("gn_part", ws, c.device)[:ws].view(torch.float32)
        assert not bool(torch.isnan(part).any()), int(torch.isnan(part).sum())
    return c, y, mr


def gn_case(sizes, N, Cin):
    case = dict(Wr.conv_case(sizes, N, Cin, Wr.GN_COUT))
    case.update(xg=case["x"].cuda(), wg=case["w"].cuda(), gamma=R.gn_pow2_gamma().cuda(), beta=torch.zeros(Wr.GN_COUT, device="cuda"))
    return case


def check_fused_exact(K, lib, case):
    sizes, N, Cin, c_ref = (case[k] for k in ("sizes", "N", "Cin", "c"))
    what = f"fused GroupNorm statistics {Cin}->{Wr.GN_COUT} N={N} {sizes}"
    c, y, mr = run_fused(K, lib, case)
    assert_exact(c.cpu(), c_ref, what + ": c", sizes)
    assert mr.shape == (N, len(sizes), R.GN_G, 2) and not bool(torch.isnan(mr).any()), what
    want = R.gn_stats_ref(c_ref, sizes).float()
    d = R.ulp_distance(mr.cpu(), want)
    assert int(d.max()) <= 1, (what, int(d.max()), [int(v) for v in (d > 1).nonzero()[0]])     # at (n, level, group, mean / rstd)
    y_ref = R.gn_apply_f32(c_ref, mr.cpu(), R.gn_pow2_gamma(), torch.zeros(Wr.GN_COUT), sizes)
    assert_same_bits(y, y_ref, what + ": y from the kernel's own statistics")
    c2, y2, mr2 = run_fused(K, lib, case, refill=False)
    for a, b, name in ((c2, c, "c"), (y2, y, "y"), (mr2, mr, "mean_rstd")):
        assert_same_bits(a, b, what + f": {name} of a second call")
    return c, y, mr


def check_stale(K, lib, large, small, alone):
    """the large launch, then the small one on the workspace the large one left behind: the small list's results alone"""
    gn_part_fill(K, 1)
    run_fused(K, lib, large, refill=False)
    got = run_fused(K, lib, small, refill=False)
    for a, b, name in zip(got, alone, ("c", "y", "mean_rstd")):
        assert_same_bits(a, b, f"{small['sizes']} behind {large['sizes']}: {name}")


@pytest.mark.parametrize("H0", ROWS)
def test_fused_groupnorm_statistics_exact(K, lib, wino_p_mode, gn_fused, H0):
    """kernels.conv3x3_gn_relu_forward on the 128-couts-per-item kernel, row H0 of the sweep at Cout = 256: every list at (Cin 64,
    N 3) and (Cin 256, N 1), one at (64, 1) and (256, 3); the partial-sum workspace is full of NaN before the call.  c is the integer
    convolution, mean_rstd at most 1 ulp from the reference at every (image, level, group), y the apply formula on the kernel's own
    statistics bit for bit, a second call the same bits; then the row's largest launch followed by its smallest with no refill."""
    wino_p_mode(2)
    done = []
    for sizes, N, Cin in Wr.gn_cases(H0):
        case = gn_case(sizes, N, Cin)
        done.append((Wr.list_blocks(sizes, N), len(done), case, check_fused_exact(K, lib, case)))
    (_, _, small, alone), (_, _, large, _) = min(done)[:4], max(done)[:4]
    assert Wr.list_blocks(large["sizes"], large["N"]) > Wr.list_blocks(small["sizes"], small["N"])
    check_stale(K, lib, large, small, alone)


@pytest.mark.parametrize("i", range(len(Wr.GN_MS_CASES)))
def test_fused_groupnorm_statistics_exact_multi_scale(K, lib, wino_p_mode, gn_fused, i):
    """the same on level lists of multi-scale training; then a three-item list on the workspace the big launch filled"""
    wino_p_mode(2)
    case = gn_case(*Wr.GN_MS_CASES[i])
    check_fused_exact(K, lib, case)
    small = gn_case(Wr.GN_STALE_SMALL, case["N"], case["Cin"])
    alone = check_fused_exact(K, lib, small)
    check_stale(K, lib, case, small, alone)


# ---------------------------------------------------------------------------------------------
# 3. fused statistics at a large mean-to-std ratio
# ---------------------------------------------------------------------------------------------
GN_PARTIAL_ROUNDINGS = 12
RATIO_Y_BOUND = 1e-5              # the forward bound of test_groupnorm_numeric


@pytest.mark.parametrize("target", Wr.RATIO_TARGETS)
def test_fused_groupnorm_statistics_at_a_large_mean_to_std_ratio(K, lib, wino_p_mode, gn_fused, target):
    """Non-integer data (x = |randn|, He-scaled weights plus a per-output-channel constant on the centre tap; 256 -> 256,
    [(25,42),(13,21),(7,11),(4,6),(2,3)], N = 3) whose per-group r = |mean| / std has a median near `target`
    (tests/test_wino_refs_cpu.py asserts that).  The per-item sums of x and x^2 are fp32; only the fold is f64 and forms
    var = E[x^2] - mean^2, so their rounding errors are amplified by 1 + r^2.

    k = GN_PARTIAL_ROUNDINGS = 12 is the number of fp32 roundings on the longest path from a value to the item's sum of squares in
    wino_x3p_kernel's output stage: 1 (the square, where it is not contracted into an fma) + 2 (the lane's pairwise sum of four) + 4 (the
    DPP steps of wave_sum_dpp) + 2 (its pairwise sum of the four row sums) + 3 (the 32-thread combine of the four transform rows'
    shares).  Each partial sum so carries at most k u of its sum of magnitudes (u = 2^-24): |d E[x^2]| <= k u E[x^2],
    |d mean| <= k u E|x| <= k u sqrt(var + mean^2), hence |d var| <= 3 k u (var + mean^2) and
        |d rstd| / rstd <= 1.5 k u (1 + r^2) + 2^-23          |d mean| <= k u sqrt(var + mean^2) + u |mean|
    (the last terms: the results' own rounding to fp32).  Both are asserted at every (image, level, group) against an fp64
    evaluation of the kernel's own c.  For the targets 0 and 3, y per level is also held to the project's forward bound 1e-5; for 10
    and 30 the errors are printed (DESIGN.md section 2 records them)."""
    wino_p_mode(2)
    sizes, N = Wr.RATIO_SIZES, Wr.RATIO_N
    x, w, gamma, beta = Wr.ratio_inputs(target)
    case = dict(sizes=sizes, N=N, xg=x.cuda(), wg=w.cuda(), gamma=gamma.cuda(), beta=beta.cuda())
    c, y, mr = run_fused(K, lib, case)
    assert not bool(torch.isnan(mr).any() | torch.isnan(y).any() | torch.isnan(c).any())
    cc = c.cpu()
    mean, var = Wr.group_moments(cc, sizes)
    rstd = 1.0 / torch.sqrt(var + R._eps32(R.GN_EPS))
    r = mean.abs() / var.sqrt()
    u, k = 2.0 ** -24, GN_PARTIAL_ROUNDINGS
    got_mean, got_rstd = mr[..., 0].double().cpu(), mr[..., 1].double().cpu()
    e_rstd = (got_rstd - rstd).abs() / rstd
    e_mean = (got_mean - mean).abs()
    b_rstd = 1.5 * k * u * (1.0 + r * r) + 2.0 ** -23
    b_mean = k * u * torch.sqrt(var + mean * mean) + u * mean.abs()
    y_ref = R.gn_fwd_ref(cc, gamma, beta, sizes)[0]
    e_y = [R.relerr(y[:, sl].cpu().double(), y_ref[:, sl]) for sl in R.level_slices(sizes)]
    print(f"fused GroupNorm statistics, target r {target}: median r {float(r.median()):.2f} (max {float(r.max()):.1f}); rstd rel. error max "
          f"{float(e_rstd.max()):.3g} (largest share of its bound {float((e_rstd / b_rstd).max()):.3f}); mean error / std max "
          f"{float((e_mean / var.sqrt()).max()):.3g} (share {float((e_mean / b_mean).max()):.3f}); y relerr per level "
          f"{' '.join('%.3g' % e for e in e_y)}")
    assert bool((e_rstd <= b_rstd).all()), (target, float((e_rstd / b_rstd).max()))
    assert bool((e_mean <= b_mean).all()), (target, float((e_mean / b_mean).max()))
    if target <= 3:
        assert max(e_y) < RATIO_Y_BOUND, (target, e_y)
