"""GPU: the reduction-shaped kernels of elementwise.hip -- ReLU backward with column sums, column sums, the five GroupNorm kernels --
against the plain CPU references of tests/reduce_refs.py, at the shapes where their chunk tables, unrolled loops, LDS folds and
atomics change branch.

Inputs are small integers wherever a sum is checked, so every sum is exact in any order (tests/test_reduce_refs_cpu.py bounds every
partial sum) and is held to BIT equality: one lost or doubled row fails.  Outputs that a kernel stores (dz, y, dc, mean_rstd, the
zero-filled colsum) are pre-filled with NaN, and so is the statistics workspace that the GroupNorm launchers must zero themselves.
Which branch each case reaches is computed from the launchers' constants in reduce_refs.py and asserted in the CPU test."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import reduce_refs as R

NAN = float("nan")
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
G = R.GN_G


@pytest.fixture(scope="module")
def K():
    from erd_amd import kernels
    assert torch.cuda.is_available()
    return kernels


def nans(shape, dtype=F32):
    return torch.full(tuple(shape), NAN, dtype=dtype, device="cuda")


def dev(*ts):
    """GPU copies, to be bound to names that outlive the launch: a raw pointer does not keep a temporary's memory alive"""
    return tuple(None if t is None else t.cuda() for t in ts)


def assert_same(got, want, what=""):
    """bit equality (so -0 != +0), with a message that names the first element that differs"""
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not R.same_bits(got, want):
        bad = R.bits(got) != R.bits(want)
        first = [int(v) for v in bad.nonzero()[0]]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ ({int(torch.isnan(got).sum())} NaN); "
                             f"first at {first}: got {float(got[tuple(first)])}, want {float(want[tuple(first)])}")


def exact_f32(t64, what=""):
    """an fp64 reference sum as fp32, after checking that nothing is lost on the way"""
    t32 = t64.float()
    assert torch.equal(t32.double(), t64), what
    return t32


# ---------------------------------------------------------------------------------------------
# ReLU backward + column sums
# ---------------------------------------------------------------------------------------------
def run_relu(K, y, dy, colsum0):
    """raw erd_relu_bwd_colsum on a dense map, dz pre-filled with NaN; colsum0: what the accumulator holds before, or None"""
    N, H, W, Cc = dy.shape
    yg, dyg, cs = dev(y, dy, colsum0)
    dz = nans(dy.shape, dy.dtype)
    K.call("erd_relu_bwd_colsum", K._p(yg), K._p(dyg), K._p(dz), N * H * W, Cc, H * W * Cc, H * W, K._p(cs), 1, K._mt(dyg, yg),
           K._stream())
    return dz, cs


def check_relu_dense(K, N, H, W, Cc, dtype, seed):
    what = f"relu_bwd_colsum {N}x{H}x{W}x{Cc} {dtype}"
    y, dy = R.relu_y(seed, N, H, W, Cc).to(dtype), R.ints(seed + 1, -R.DY_MAX, R.DY_MAX, N, H, W, Cc).to(dtype)
    pre = R.ints(seed + 2, -R.PRELOAD_MAX, R.PRELOAD_MAX, Cc)
    dz_ref, cs64 = R.relu_bwd_colsum_ref(y, dy, True)
    assert torch.equal(dz_ref, dy * (y > 0))
    cs_ref, cs_pre_ref = exact_f32(cs64, what), exact_f32(cs64 + pre.double(), what)
    dz, cs = run_relu(K, y, dy, torch.zeros(Cc))
    assert_same(dz, dz_ref, what + ": dz")
    assert_same(cs, cs_ref, what + ": colsum")
    dz, cs = run_relu(K, y, dy, pre)                                          # the accumulator is added to
    assert_same(dz, dz_ref, what + ": dz (pre-loaded colsum)")
    assert_same(cs, cs_pre_ref, what + ": pre-loaded colsum")
    dz, cs = run_relu(K, y, dy, None)                                         # no column sum wanted
    assert_same(dz, dz_ref, what + ": dz (no colsum)")
    # the wrapper's three forms
    yg, dyg, pg = dev(y, dy, pre)
    dz, cs = K.relu_bwd_colsum(yg, dyg, True)
    assert_same(dz, dz_ref, what + ": K dz")
    assert_same(cs, cs_ref, what + ": K colsum")
    dz, cs = K.relu_bwd_colsum(yg, dyg, True, want_colsum=False)
    assert cs is None
    assert_same(dz, dz_ref, what + ": K dz (want_colsum=False)")
    dz, cs = K.relu_bwd_colsum(yg, dyg, True, colsum_into=pg)
    assert cs is pg
    assert_same(pg, cs_pre_ref, what + ": K colsum_into")
    assert_same(yg, y, what + ": y")                                          # the inputs stay as they were
    assert_same(dyg, dy, what + ": dy")


@pytest.mark.parametrize("Cc", R.RELU_DENSE_CS)
def test_relu_bwd_colsum_dense(K, Cc):
    """1, unit - 1, unit, unit + 1 rows and a map of several workgroups with a ragged last one, for every launch geometry: one
    float4 column x 256 row lanes (C = 4) ... 16 columns x 16 lanes x 32 column groups (C = 2048).  y holds +0.0 and -0.0."""
    for i, (N, H, W) in enumerate(R.relu_dense_maps(Cc)):
        check_relu_dense(K, N, H, W, Cc, F32, 3000 + 16 * Cc + 3 * i)


def test_relu_bwd_colsum_dense_bf16_maps(K):
    Cc = R.RELU_BF16_C
    for i, (N, H, W) in enumerate(R.relu_dense_maps(Cc)):
        check_relu_dense(K, N, H, W, Cc, BF16, 3500 + 3 * i)


@pytest.mark.parametrize("Cc,li,N", R.RELU_STRIDED)
def test_relu_bwd_colsum_strided_level_views(K, Cc, li, N):
    """use_relu = False on every level view of an [N, A, C] buffer (the FPN P6 / P7 bias gradients): row r belongs to image
    r / rows_per_img, and workgroups of 64 rows straddle the images.  The column sums are exact, dz is dy itself, and the whole buffer -- the other levels' rows included -- stays
    bit for bit what it was."""
    sizes = R.GN_LEVEL_LISTS[li]
    A = R.total_rows(sizes)
    buf = R.ints(3600 + 10 * li + N + Cc, -R.DY_MAX, R.DY_MAX, N, A, Cc)
    bg, = dev(buf)
    for lvl, (v, sl) in enumerate(zip(K.level_views(bg, sizes), R.level_slices(sizes))):
        what = f"strided relu_bwd_colsum C={Cc} N={N} level {lvl} of {sizes}"
        rows = sl.stop - sl.start
        assert A * Cc != rows * Cc and (N == 1 or v.stride(0) == A * Cc)
        cs_ref = exact_f32(R.relu_bwd_colsum_ref(None, buf[:, sl], False)[1], what)
        dz, cs = K.relu_bwd_colsum(None, v, False)
        assert dz is v
        assert_same(cs, cs_ref, what)
        # the entry point with the buffer's image stride spelled out: torch gives the view of ONE image the dense stride, so for N = 1
        # the wrapper reaches the dense branch, this call the strided one (every row is image 0 either way)
        cs = torch.zeros(Cc, device="cuda")
        K.call("erd_relu_bwd_colsum", K._p(None), K._p(v), K._p(None), N * rows, Cc, A * Cc, rows, K._p(cs), 0, 0, K._stream())
        assert_same(cs, cs_ref, what + ": raw")
        pre = R.ints(3700 + lvl, -R.PRELOAD_MAX, R.PRELOAD_MAX, Cc)
        pg, = dev(pre)
        K.relu_bwd_colsum(None, v, False, colsum_into=pg)
        assert_same(pg, exact_f32(cs_ref.double() + pre.double(), what), what + ": colsum_into")
        dz, cs = K.relu_bwd_colsum(None, v, False, want_colsum=False)
        assert dz is v and cs is None
    assert_same(bg, buf, f"the [N, A, C] buffer behind the level views, C={Cc} N={N} {sizes}")


@pytest.mark.parametrize("Cc", R.RELU_REFUSED_CS)
def test_relu_bwd_colsum_refuses_channel_counts_it_cannot_tile(K, Cc):
    """C / 4 = 17 and 20 fit neither geometry: an argument error that names C, before any launch -- dz and colsum keep their fill"""
    from erd_amd._lib import ErdHipError
    assert R.relu_geometry(1, Cc) is None
    N, H, W = 2, 3, 5
    yg, dyg = dev(R.relu_y(3800, N, H, W, Cc), R.ints(3801, -R.DY_MAX, R.DY_MAX, N, H, W, Cc))
    dz, cs = nans((N, H, W, Cc)), nans((Cc,))
    with pytest.raises(ErdHipError, match=f"C={Cc}"):
        K.call("erd_relu_bwd_colsum", K._p(yg), K._p(dyg), K._p(dz), N * H * W, Cc, H * W * Cc, H * W, K._p(cs), 1, 0, K._stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(dz).all()) and bool(torch.isnan(cs).all())
    with pytest.raises(ErdHipError, match=f"C={Cc}"):
        K.relu_bwd_colsum(yg, dyg, True)


# ---------------------------------------------------------------------------------------------
# column sums
# ---------------------------------------------------------------------------------------------
def check_colsum(K, rows, Cc, dtype, seed):
    what = f"colsum {rows}x{Cc} {dtype}"
    x = R.ints(seed, -R.DY_MAX, R.DY_MAX, rows, Cc).to(dtype)
    ref = exact_f32(R.colsum_ref(x), what)
    xg, = dev(x)
    out = nans((Cc,))                                                         # the launcher's zero fill must happen
    K.call("erd_colsum", K._p(xg), rows, Cc, K._p(out), 0, K._mt(xg), K._stream())
    assert_same(out, ref, what)
    assert_same(K.colsum(xg), ref, what + ": K.colsum")
    out = nans((Cc,))
    assert K.colsum(xg, out=out) is out
    assert_same(out, ref, what + ": K.colsum(out=)")
    pre = R.ints(seed + 1, -R.PRELOAD_MAX, R.PRELOAD_MAX, Cc)                  # accumulate = 1: added to, not filled
    pg, = dev(pre)
    K.call("erd_colsum", K._p(xg), rows, Cc, K._p(pg), 1, K._mt(xg), K._stream())
    assert_same(pg, exact_f32(ref.double() + pre.double(), what), what + ": accumulate")


@pytest.mark.parametrize("Cc", R.COLSUM_CS)
def test_colsum_exact(K, Cc):
    """1 / 63 / 64 / 65 / 4097 rows (one workgroup, one full, one row into the second, 65 workgroups adding to the same addresses) at
    C = 4, the 68- and 70-channel heads (scalar loads, rows not 16-byte aligned), 256, and past it: 260 and 1000 columns take a
    second and a fourth pass of the `c += 256` loop"""
    for i, rows in enumerate(R.COLSUM_ROWS):
        check_colsum(K, rows, Cc, F32, 4000 + 8 * Cc + 2 * i)


def test_colsum_past_2048_workgroups(K):
    rows, Cc = R.COLSUM_LONG
    assert R.colsum_geometry(rows, Cc)["rpb"] == 128
    check_colsum(K, rows, Cc, F32, 4500)


@pytest.mark.parametrize("Cc", R.COLSUM_BF16_CS)
def test_colsum_exact_bf16_maps(K, Cc):
    for i, rows in enumerate(R.COLSUM_ROWS):
        check_colsum(K, rows, Cc, BF16, 4600 + 8 * Cc + 2 * i)


def test_colsum_of_a_level_concatenated_buffer(K):
    """K.colsum on a 3-D [N, A, C] input: N * A rows"""
    N, A, Cc = 3, R.total_rows(R.GN_LEVEL_LISTS[0]), 68
    x = R.ints(4700, -R.DY_MAX, R.DY_MAX, N, A, Cc)
    xg, = dev(x)
    out = nans((Cc,))
    K.colsum(xg, out=out)
    assert_same(out, exact_f32(R.colsum_ref(x)), "K.colsum [N, A, C]")


# ---------------------------------------------------------------------------------------------
# GroupNorm + ReLU
# ---------------------------------------------------------------------------------------------
def gn_fwd(K, c, gamma, beta, sizes):
    """raw erd_gn_relu_fwd on GPU tensors -> (y, mean_rstd); both, and the statistics workspace, pre-filled with NaN"""
    N, A, Cc = c.shape
    lv = K.make_levels(sizes)
    y, mr = nans(c.shape, c.dtype), nans((N, len(sizes), G, 2))
    ws = nans((N * len(sizes) * G * 2,), F64)
    K.call("erd_gn_relu_fwd", K._p(c), K._p(y), K._p(gamma), K._p(beta), K._p(ws), K._p(mr), N, A, Cc, G, C.byref(lv), R.GN_EPS,
           K._mt(c), K._stream())
    torch.cuda.synchronize()
    return y, mr


def gn_bwd(K, c, dy, gamma, beta, mr, sizes, dgamma0=None, dbeta0=None):
    """raw erd_gn_relu_bwd on GPU tensors -> (dc, dgamma, dbeta); dc and the workspace pre-filled with NaN, the two accumulators with
    zeros or with what the caller hands in (CPU tensors)"""
    N, A, Cc = c.shape
    lv = K.make_levels(sizes)
    dc = nans(c.shape, c.dtype)
    ws = nans((N * len(sizes) * G * 2,), F64)
    dg, db = dev(torch.zeros(Cc) if dgamma0 is None else dgamma0, torch.zeros(Cc) if dbeta0 is None else dbeta0)
    K.call("erd_gn_relu_bwd", K._p(c), K._p(dy), K._p(gamma), K._p(beta), K._p(mr), K._p(ws), K._p(dc), K._p(dg), K._p(db), N, A, Cc,
           G, C.byref(lv), K._mt(c, dy), K._stream())
    torch.cuda.synchronize()
    return dc, dg, db


GN_CASES = [(li, N) for li in range(len(R.GN_LEVEL_LISTS)) for N in R.GN_NS]
GN_BF16_CASES = [(li, 3) for li in R.GN_MASK_LISTS]


def check_gn_integer_forward(K, li, N, dtype):
    """integer c, gamma in {0.5, 1, 2, -1}, beta = 0"""
    sizes = R.GN_LEVEL_LISTS[li]
    what = f"groupnorm {sizes} N={N} {dtype}"
    c, gamma, beta = R.gn_int_c(li, N), R.gn_pow2_gamma(), torch.zeros(R.GN_C)
    cg, gg, bg = dev(c.to(dtype), gamma, beta)
    y, mr = gn_fwd(K, cg, gg, bg, sizes)
    # statistics: sum and sum of squares are exact, so both sides evaluate one fp64 formula on the same numbers and can differ only
    # where its result sits on an fp32 rounding boundary
    want = R.gn_stats_ref(c, sizes).float()
    d = R.ulp_distance(mr.cpu(), want)
    print(f"{what}: mean_rstd at most {int(d.max())} ulp from the reference, {int((d > 0).sum())} of {d.numel()} differ")
    assert int(d.max()) <= 1, (what, int(d.max()), [int(v) for v in (d > 1).nonzero()[0]])
    for lvl, (h, w) in enumerate(sizes):
        if h * w == 1:                                                        # the even groups hold one value eight times
            rstd0 = torch.tensor(1.0 / R._eps32(R.GN_EPS) ** 0.5, dtype=F64).float()
            assert_same(mr[:, lvl, ::2, 1], rstd0.expand(N, G // 2).contiguous(), what + ": rstd of a zero variance")
            assert_same(mr[:, lvl, ::2, 0], c[:, R.level_slices(sizes)[lvl].start, ::16].contiguous(), what + ": mean of a constant")
    # apply, bit for bit, from the kernel's OWN statistics: a wrong level / group index, chunk start or end, a row written twice with
    # different statistics or not at all shows as a differing element
    y_ref = R.gn_apply_f32(c, mr.cpu(), gamma, beta, sizes).to(dtype)
    assert_same(y, y_ref, what + ": y")
    y2, mr2 = gn_fwd(K, cg, gg, bg, sizes)                                    # the workspace is zeroed again
    assert_same(mr2, mr.cpu(), what + ": mean_rstd of a second call")
    assert_same(y2, y_ref, what + ": y of a second call")
    y3, mr3 = K.gn_relu_forward(cg, gg, bg, sizes)                            # the wrapper (its own, reused workspace), twice
    y4, mr4 = K.gn_relu_forward(cg, gg, bg, sizes)
    for yy, mm in ((y3, mr3), (y4, mr4)):
        assert_same(mm, mr.cpu(), what + ": K.gn_relu_forward mean_rstd")
        assert_same(yy, y_ref, what + ": K.gn_relu_forward y")
    assert_same(cg, c.to(dtype), what + ": c")


@pytest.mark.parametrize("li,N", GN_CASES)
def test_groupnorm_statistics_and_apply_exact(K, li, N):
    check_gn_integer_forward(K, li, N, F32)


@pytest.mark.parametrize("li,N", GN_BF16_CASES)
def test_groupnorm_statistics_and_apply_exact_bf16_maps(K, li, N):
    """integers up to 4 are exact in bf16: the same statistics; y is the fp32 result rounded once"""
    check_gn_integer_forward(K, li, N, BF16)


@pytest.mark.parametrize("li,N", GN_CASES)
def test_groupnorm_backward_dbeta_exact(K, li, N):
    """integer dy, random c / gamma / beta: dbeta[ch] = sum of dy over the elements the FORWARD let through is an integer sum -- a row
    that gn_bwd_stats_kernel's chunking loses or doubles, or an element whose mask it decides differently, changes it.  Then the
    same into accumulators pre-loaded with integers: dbeta exactly, dgamma to the project's bound."""
    sizes = R.GN_LEVEL_LISTS[li]
    what = f"groupnorm backward {sizes} N={N}"
    c, gamma, beta = R.gn_random_inputs(li, N)
    dy = R.ints(5000 + 10 * li + N, -R.DY_MAX, R.DY_MAX, *c.shape)
    cg, gg, bg, dyg = dev(c, gamma, beta, dy)
    y, mr = gn_fwd(K, cg, gg, bg, sizes)
    mask = y.cpu() > 0
    assert not bool(torch.isnan(y).any()) and 0.2 < float(mask.float().mean()) < 0.8
    db_ref = exact_f32((dy.double() * mask).sum((0, 1)), what)
    dc, dg, db = gn_bwd(K, cg, dyg, gg, bg, mr, sizes)
    assert_same(db, db_ref, what + ": dbeta")
    assert not bool(torch.isnan(dc).any())
    dg0, db0 = (R.ints(5001 + k, -R.PRELOAD_MAX, R.PRELOAD_MAX, R.GN_C) for k in (0, 1))
    dc, dg, db = gn_bwd(K, cg, dyg, gg, bg, mr, sizes, dg0, db0)
    assert_same(db, exact_f32(db_ref.double() + db0.double(), what), what + ": pre-loaded dbeta")
    dg_ref = R.gn_bwd_ref(c, dy, gamma, mask, sizes)[1]
    err = R.relerr(dg.cpu().double(), dg_ref + dg0.double())
    print(f"{what}: pre-loaded dgamma relerr {err:.3g}")
    assert err < 1e-4, (what, err)
    dc, dg, db = K.gn_relu_backward(cg, dyg, gg, bg, mr, sizes)               # the wrapper, fresh accumulators
    assert_same(db, db_ref, what + ": K.gn_relu_backward dbeta")
    pg, = dev(db0)
    dc, dg, db = K.gn_relu_backward(cg, dyg, gg, bg, mr, sizes, dbeta=pg)
    assert db is pg
    assert_same(pg, exact_f32(db_ref.double() + db0.double(), what), what + ": K.gn_relu_backward dbeta=")


@pytest.mark.parametrize("li", R.GN_MASK_LISTS)
def test_groupnorm_relu_mask_is_one_decision(K, li):
    """The backward kernels do not read y: gn_bwd_stats and gn_bwd_apply each recompute the ReLU mask as xh * gamma + beta > 0, and the
    forward clamps the same expression.  With beta[ch] = -fl(xh * gamma[ch]) at one element per channel, the unfused affine is
    exactly 0 there and the fused one is the product's rounding residual (positive at about half of them: the CPU test asserts the
    share), so kernels that evaluate the expression differently disagree -- by a whole dy in dbeta, by a whole dy * gamma * rstd in dc.
    Whichever order the compiler picked, all three must have picked the same."""
    sizes, N = R.GN_LEVEL_LISTS[li], 3
    what = f"groupnorm mask agreement {sizes}"
    c, gamma, _ = R.gn_random_inputs(li, N)
    cg, gg, zg = dev(c, gamma, torch.zeros(R.GN_C))
    _, mr = gn_fwd(K, cg, gg, zg, sizes)                                      # the statistics do not depend on beta
    beta, (n, row, ch) = R.adversarial_beta(c, mr.cpu(), gamma, sizes)
    dy = R.gn_mask_dy(5100 + li, c.shape, (n, row, ch))
    bg, dyg = dev(beta, dy)
    y, mr2 = gn_fwd(K, cg, gg, bg, sizes)
    assert_same(mr2, mr.cpu(), what + ": mean_rstd")
    dc, dg, db = gn_bwd(K, cg, dyg, gg, bg, mr, sizes)
    mask = y.cpu() > 0
    on = mask[n, row, ch]
    print(f"{what}: the forward lets {int(on.sum())} of {on.numel()} constructed elements through")
    # (a) gn_bwd_stats against the forward
    assert_same(db, exact_f32((dy.double() * mask).sum((0, 1)), what), what + ": dbeta against the forward's mask")
    # (b) gn_bwd_apply against the forward, at the constructed elements
    dc_ref = R.gn_bwd_ref(c, dy, gamma, mask, sizes)[0]
    lvl_of_row = torch.cat([torch.full((sl.stop - sl.start,), i) for i, sl in enumerate(R.level_slices(sizes))])
    level_max = torch.stack([dc_ref[:, sl].abs().max() for sl in R.level_slices(sizes)])
    err = (dc.cpu().double() - dc_ref)[n, row, ch].abs() / level_max[lvl_of_row[row]]
    print(f"{what}: dc at the constructed elements, largest error {float(err.max()):.3g} of the level's largest |dc|")
    assert float(err.max()) < 1e-4, (what, float(err.max()), int(err.argmax()))
    for i, sl in enumerate(R.level_slices(sizes)):                            # ... and everywhere else
        e = R.relerr(dc[:, sl].cpu().double(), dc_ref[:, sl])
        assert e < 1e-4, (what, i, e)
    # (c) two runs agree bit for bit.  (dgamma is left out: float atomics of non-integers round by arrival order.  So, in principle,
    # do the double atomics behind dc's group sums where a level has several statistics chunks -- by 1e-16, which reaches the fp32 that
    # gn_bwd_apply rounds them to about once in 1e8 sums.)
    y_b, _ = gn_fwd(K, cg, gg, bg, sizes)
    dc_b, _, db_b = gn_bwd(K, cg, dyg, gg, bg, mr, sizes)
    assert_same(y_b, y.cpu(), what + ": y of a second run")
    assert_same(db_b, db.cpu(), what + ": dbeta of a second run")
    assert_same(dc_b, dc.cpu(), what + ": dc of a second run")


GN_NUMERIC_MARGIN = 1e-5


@pytest.mark.parametrize("li", range(len(R.GN_LEVEL_LISTS)))
def test_groupnorm_numeric(K, li):
    """random data at the scale of test_groupnorm_relu_fwd_bwd against the fp64 references, its bounds (1e-5 forward, 1e-4 backward),
    y and dc PER LEVEL (a small level's error is not hidden behind a large level's values).  The mask is the reference's own.  Where
    the reference's pre-activation is within 1e-5 of zero -- ten times the fp32 rounding error of (c - mean) * rstd * gamma + beta at
    |xh| < 6 -- fp32 arithmetic does not determine the mask, so dy is zero there (a handful of elements per list); the mask decision at
    zero itself is the subject of test_groupnorm_relu_mask_is_one_decision."""
    sizes, N = R.GN_LEVEL_LISTS[li], 3
    what = f"groupnorm numeric {sizes}"
    c, gamma, beta = R.gn_random_inputs(li, N)
    dy = R.randn(5200 + li, *c.shape)
    y_ref, pre = R.gn_fwd_ref(c, gamma, beta, sizes)
    near = pre.abs() < GN_NUMERIC_MARGIN
    assert int(near.sum()) <= 1e-4 * near.numel()
    dy[near] = 0.0
    dc_ref, dg_ref, db_ref = R.gn_bwd_ref(c, dy, gamma, pre > 0, sizes)
    cg, gg, bg, dyg = dev(c, gamma, beta, dy)
    y, mr = gn_fwd(K, cg, gg, bg, sizes)
    dc, dg, db = gn_bwd(K, cg, dyg, gg, bg, mr, sizes)
    errs = {}
    for i, sl in enumerate(R.level_slices(sizes)):
        errs[f"y level {i}"] = R.relerr(y[:, sl].cpu().double(), y_ref[:, sl]), 1e-5
        errs[f"dc level {i}"] = R.relerr(dc[:, sl].cpu().double(), dc_ref[:, sl]), 1e-4
    errs["dgamma"] = R.relerr(dg.cpu().double(), dg_ref), 1e-4
    errs["dbeta"] = R.relerr(db.cpu().double(), db_ref), 1e-4
    print(what, {k: f"{e:.3g}" for k, (e, _) in errs.items()}, f"({int(near.sum())} elements near zero)")
    assert not bool(torch.isnan(y).any() | torch.isnan(dc).any() | torch.isnan(mr).any())
    for k, (e, bound) in errs.items():
        assert e < bound, (what, k, e)
