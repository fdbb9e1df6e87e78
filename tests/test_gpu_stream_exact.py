"""GPU: the streaming loops of elementwise.hip that keep four 16-byte rows in flight per thread -- GroupNorm apply, GroupNorm backward
(statistics and apply), the float4 column sum and the per-level scale's backward -- at the row counts where an unrolled pass, its one-row tail,
a chunk and a level end, against the host references of tests/reduce_refs.py (tests/glue_refs.py for the level scale).

Every sum is over integers, or over products of small integers with powers of two, so it is exact in any order and held to BIT
equality; stored outputs are compared bit for bit and are pre-filled with NaN.  GroupNorm runs from a GIVEN mean_rstd (integer means,
power-of-two rstd, different for every image, level and group) with power-of-two gamma and beta = 0, so (c - mean) * rstd * gamma is
exact whatever the compiler fuses, and a row normalised with another row's statistics differs.  Where a kernel keeps a 16-byte and a
4-byte path, data of a wide exponent range makes the SUM depend on the order of its additions, and the result must carry the bits
of the expected path's order (tests/test_csrc_stream_build.py holds the constants restated here to the source)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import glue_refs as GR
import reduce_refs as R

NAN = float("nan")
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
G, CH = R.GN_G, R.GN_C

# restated from elementwise.hip: rows in flight per thread, row lanes of the apply / statistics kernels, rows per chunk
FLIGHT = 4
APPLY_U, APPLY_R = FLIGHT * 4, R.GN_ROWS                      # 16 rows per unrolled pass, 128 per workgroup
STAT_U, STAT_R = FLIGHT * R.GN_STAT_LANES, R.GN_STAT_ROWS     # 64, 512
COLSUM_WGS = 128


def ragged(U, Rr):
    return [1, U - 1, U, U + 1, Rr - 1, Rr, Rr + 1, 2 * Rr + 3]


_a, _s = ragged(APPLY_U, APPLY_R), ragged(STAT_U, STAT_R)
# two- and five-level tables over the row counts of both kernels' (U, R): levels shorter than one pass (1, 15), ending inside a pass
# (17, 65, 129), ending on a pass (16, 64, 128, 512) and with a chunk boundary inside (129, 259, 513, 1027)
LEVEL_ROWS = [[_a[0], _a[1], _a[2], _a[3], _a[4]],            # 1 15 16 17 127
              [_a[5], _a[6], _a[7], _a[0], _a[3]],            # 128 129 259 1 17
              [_a[7], _a[1]],                                 # 259 15
              [_s[1], _s[2], _s[3], _s[0], _s[4]],            # 63 64 65 1 511
              [_s[5], _s[6]],                                 # 512 513
              [_s[7], _s[3]]]                                 # 1027 65
assert {r for t in LEVEL_ROWS for r in t} == set(_a) | set(_s) and sorted({len(t) for t in LEVEL_ROWS}) == [2, 5]
TABLES = [[(1, r) for r in t] for t in LEVEL_ROWS]
N_IMG = 2


@pytest.fixture(scope="module")
def K():
    from erd_amd import kernels
    assert torch.cuda.is_available()
    return kernels


def nans(shape, dtype=F32):
    return torch.full(tuple(shape), NAN, dtype=dtype, device="cuda")


def dev(*ts):
    return tuple(None if t is None else t.cuda() for t in ts)


def assert_same(got, want, what="", zero_sign=True):
    """bit equality; zero_sign=False: a zero may carry either sign (a product with a negative gamma)"""
    got = got.cpu()
    if not zero_sign:
        got, want = got + 0.0, want + 0.0
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not R.same_bits(got, want):
        bad = R.bits(got) != R.bits(want)
        first = [int(v) for v in bad.nonzero()[0]]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ ({int(torch.isnan(got).sum())} NaN); "
                             f"first at {first}: got {float(got[tuple(first)])}, want {float(want[tuple(first)])}")


def exact_f32(t64, what=""):
    t32 = t64.float()
    assert torch.equal(t32.double(), t64), what
    return t32


def one_level(off, cnt):
    from erd_amd._lib import Levels
    lv = Levels()
    lv.nseg, lv.off[0], lv.cnt[0] = 1, off, cnt
    return lv


# ---------------------------------------------------------------------------------------------
# GroupNorm apply and backward from a given mean_rstd
# ---------------------------------------------------------------------------------------------
_GN = {}


def gn_case(ti):
    """inputs and references of one level table, computed once.  Channels k and k + 4 of a group hold the same c and gamma and
    opposite dy, so the group sums s1 and s2 are exactly zero and dc = rstd * dy * mask * gamma with no rounding at all"""
    if ti in _GN:
        return _GN[ti]
    sizes = TABLES[ti]
    A, nseg = R.total_rows(sizes), len(sizes)
    pair = lambda t: t.view(*t.shape[:-1], G, 2, 4)
    c = R.ints(7000 + ti, -R.C_MAX, R.C_MAX, N_IMG, A, CH)
    pair(c)[..., 1, :] = pair(c)[..., 0, :]
    gamma = R.gn_pow2_gamma().clone()
    pair(gamma)[..., 1, :] = pair(gamma)[..., 0, :]
    dy = R.ints(7100 + ti, -R.DY_MAX, R.DY_MAX, N_IMG, A, CH)
    pair(dy)[..., 1, :] = -pair(dy)[..., 0, :]
    mr = torch.stack([R.ints(7200 + ti, -2, 2, N_IMG, nseg, G), 2.0 ** R.ints(7300 + ti, -1, 1, N_IMG, nseg, G)], -1).contiguous()
    beta = torch.zeros(CH)
    xh = R.gn_xhat_f32(c, mr, sizes)
    y = R.gn_apply_f32(c, mr, gamma, beta, sizes)
    assert torch.equal(y, R.gn_apply_f32(c, mr, gamma, beta, sizes, fused=True))          # exact: the evaluation order cannot matter
    mask = xh * gamma > 0
    assert 0.2 < float(mask.float().mean()) < 0.8
    dm = dy * mask
    dc = torch.empty_like(c)
    for i, sl in enumerate(R.level_slices(sizes)):
        dc[:, sl] = R._per_channel(mr[:, i], CH)[1] * (dm[:, sl] * gamma)
    rows64 = lambda t: [t[:, sl].double().sum((0, 1)) for sl in R.level_slices(sizes)]      # per level: [C]
    _GN[ti] = dict(sizes=sizes, A=A, c=c, gamma=gamma, beta=beta, dy=dy, mr=mr, y=y, dc=dc, mask=mask, xh=xh,
                   db=rows64(dm), dg=rows64(dm * xh), s1=dm * gamma, s2=dm * gamma * xh)
    return _GN[ti]


def gn_apply(K, c, gamma, beta, mr, N, A, lv, y):
    K.call("erd_gn_relu_apply", K._p(c), K._p(y), K._p(gamma), K._p(beta), K._p(mr), N, A, CH, G, C.byref(lv), K._mt(c), K._stream())
    torch.cuda.synchronize()


def gn_bwd(K, c, dy, gamma, beta, mr, N, A, lv, nseg, dc, dg, db):
    ws = nans((N * nseg * G * 2,), F64)
    K.call("erd_gn_relu_bwd", K._p(c), K._p(dy), K._p(gamma), K._p(beta), K._p(mr), K._p(ws), K._p(dc), K._p(dg), K._p(db), N, A, CH,
           G, C.byref(lv), K._mt(c, dy), K._stream())
    torch.cuda.synchronize()
    return ws


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("ti", range(len(TABLES)))
def test_groupnorm_apply_and_backward_at_ragged_levels(K, ti, dtype):
    d = gn_case(ti)
    sizes, A = d["sizes"], d["A"]
    what = f"groupnorm {LEVEL_ROWS[ti]} {dtype}"
    cg, dyg, gg, bg, mrg = dev(d["c"].to(dtype), d["dy"].to(dtype), d["gamma"], d["beta"], d["mr"])
    lv = K.make_levels(sizes)
    # forward apply, all levels and images
    y = nans(cg.shape, dtype)
    gn_apply(K, cg, gg, bg, mrg, N_IMG, A, lv, y)
    assert_same(y, d["y"].to(dtype), what + ": y")
    # backward into accumulators that already hold integers
    dg0, db0 = (R.ints(7400 + ti + k, -R.PRELOAD_MAX, R.PRELOAD_MAX, CH) for k in (0, 1))
    dc = nans(cg.shape, dtype)
    dgg, dbg = dev(dg0, db0)
    ws = gn_bwd(K, cg, dyg, gg, bg, mrg, N_IMG, A, lv, len(sizes), dc, dgg, dbg)
    assert_same(dbg, exact_f32(sum(d["db"]) + db0.double(), what), what + ": dbeta")
    assert_same(dgg, exact_f32(sum(d["dg"]) + dg0.double(), what), what + ": dgamma")
    assert_same(ws, torch.zeros(ws.numel(), dtype=F64), what + ": group sums", zero_sign=False)
    assert_same(dc, d["dc"].to(dtype), what + ": dc", zero_sign=False)
    assert_same(cg, d["c"].to(dtype), what + ": c")
    assert_same(dyg, d["dy"].to(dtype), what + ": dy")
    # one level of image 0 alone: the rows of its neighbours and of the other image keep their fill
    for j, sl in enumerate(R.level_slices(sizes)):
        if j not in (0, len(sizes) // 2, len(sizes) - 1):
            continue
        lv1 = one_level(sl.start, sl.stop - sl.start)
        mr1, = dev(d["mr"][:1, j:j + 1].contiguous())
        y, dc = nans(cg.shape, dtype), nans(cg.shape, dtype)
        dgg, dbg = dev(torch.zeros(CH), torch.zeros(CH))
        gn_apply(K, cg, gg, bg, mr1, 1, A, lv1, y)
        gn_bwd(K, cg, dyg, gg, bg, mr1, 1, A, lv1, 1, dc, dgg, dbg)
        y_ref, dc_ref = torch.full(d["y"].shape, NAN).to(dtype), torch.full(d["y"].shape, NAN).to(dtype)
        y_ref[0, sl], dc_ref[0, sl] = d["y"][0, sl].to(dtype), d["dc"][0, sl].to(dtype)
        inside = torch.zeros(d["y"].shape, dtype=torch.bool)
        inside[0, sl] = True
        assert bool((torch.isnan(y.cpu()) == ~inside).all()) and bool((torch.isnan(dc.cpu()) == ~inside).all()), (what, j)
        assert_same(torch.nan_to_num(y), torch.nan_to_num(y_ref), f"{what}: y of level {j}, image 0")
        assert_same(torch.nan_to_num(dc), torch.nan_to_num(dc_ref), f"{what}: dc of level {j}, image 0", zero_sign=False)
        dm0 = (d["dy"] * d["mask"])[0, sl].double()
        assert_same(dbg, exact_f32(dm0.sum(0)), f"{what}: dbeta of level {j}, image 0")
        assert_same(dgg, exact_f32((dm0 * d["xh"][0, sl].double()).sum(0)), f"{what}: dgamma of level {j}, image 0")


@pytest.mark.parametrize("ti", range(len(TABLES)))
def test_groupnorm_backward_group_sums_exact(K, ti):
    """dy without the pairing: s1 = sum dy * mask * gamma and s2 = sum dy * mask * gamma * xhat per (image, level, group) are sums of
    multiples of 1/4 -- exact in the workspace's doubles whatever chunk and lane they arrive from -- and dc follows them to the
    project's bound (1e-4 of the level's largest value, tests/test_gpu_reduce_exact.py)"""
    d = gn_case(ti)
    sizes, A = d["sizes"], d["A"]
    what = f"groupnorm group sums {LEVEL_ROWS[ti]}"
    dy = R.ints(7500 + ti, -R.DY_MAX, R.DY_MAX, N_IMG, A, CH)
    cg, dyg, gg, bg, mrg = dev(d["c"], dy, d["gamma"], d["beta"], d["mr"])
    dc = nans(cg.shape)
    dgg, dbg = dev(torch.zeros(CH), torch.zeros(CH))
    ws = gn_bwd(K, cg, dyg, gg, bg, mrg, N_IMG, A, K.make_levels(sizes), len(sizes), dc, dgg, dbg)
    dh = (dy * d["mask"] * d["gamma"]).double()
    ref = torch.empty((N_IMG, len(sizes), G, 2), dtype=F64)
    dc_ref = torch.empty(dc.shape, dtype=F64)
    for i, sl in enumerate(R.level_slices(sizes)):
        grp = lambda t: t[:, sl].reshape(N_IMG, -1, G, CH // G).sum((1, 3))
        ref[:, i, :, 0], ref[:, i, :, 1] = grp(dh), grp(dh * d["xh"].double())
        m = float((sl.stop - sl.start) * (CH // G))
        per_ch = lambda t: t.repeat_interleave(CH // G, dim=1).unsqueeze(1)
        rstd = R._per_channel(d["mr"][:, i].double(), CH)[1]
        dc_ref[:, sl] = rstd * (dh[:, sl] - per_ch(ref[:, i, :, 0]) / m - d["xh"][:, sl].double() * per_ch(ref[:, i, :, 1]) / m)
    assert_same(ws.view(N_IMG, len(sizes), G, 2), ref, what, zero_sign=False)
    assert_same(dbg, exact_f32((dy * d["mask"]).double().sum((0, 1))), what + ": dbeta")
    for i, sl in enumerate(R.level_slices(sizes)):
        e = R.relerr(dc[:, sl].cpu().double(), dc_ref[:, sl])
        assert e < 1e-4, (what, i, e)


# ---------------------------------------------------------------------------------------------
# column sums
# ---------------------------------------------------------------------------------------------
def colsum_geometry(rows, Cc, aligned=True):
    """erd_colsum's choices: (path, row lanes, rows per unrolled pass, rows per workgroup)"""
    if Cc % 4 or not aligned:
        g = R.colsum_geometry(rows, Cc)
        return "scalar", 1, g["rpb"], g["rpb"]
    C4 = Cc // 4
    cw4 = min(C4, 64)
    gy, lanes = R.cdiv(C4, cw4), 256 // cw4
    unit = 4 * lanes
    rpb = R.cdiv(R.cdiv(rows, max(COLSUM_WGS // gy, 1)), unit) * unit
    return "vector", lanes, unit, rpb


COLSUM_CS = (4, 68, 70, 80, 256)


def colsum_rows(Cc):
    _, _, U, Rr = colsum_geometry(1, Cc)
    return [1, 3, U - 1, U + 1, 2 * Rr + 1]


def check_colsum(K, rows, Cc, dtype, seed):
    what = f"colsum {rows}x{Cc} {dtype}"
    x = R.ints(seed, -R.DY_MAX, R.DY_MAX, rows, Cc).to(dtype)
    ref = exact_f32(R.colsum_ref(x), what)
    xg, = dev(x)
    out = nans((Cc,))                                                         # accumulate off: the launcher's zero fill
    K.call("erd_colsum", K._p(xg), rows, Cc, K._p(out), 0, K._mt(xg), K._stream())
    assert_same(out, ref, what)
    assert_same(K.colsum(xg), ref, what + ": K.colsum")
    pre = R.ints(seed + 1, -R.PRELOAD_MAX, R.PRELOAD_MAX, Cc)                  # accumulate on: added to
    pg, = dev(pre)
    K.call("erd_colsum", K._p(xg), rows, Cc, K._p(pg), 1, K._mt(xg), K._stream())
    assert_same(pg, exact_f32(ref.double() + pre.double(), what), what + ": accumulate")
    assert_same(xg, x, what + ": x")


@pytest.mark.parametrize("Cc", COLSUM_CS)
def test_colsum_exact_at_pass_and_workgroup_edges(K, Cc):
    """1 and 3 rows (tail only, idle lanes), one row short of and one row past an unrolled pass, and three workgroups of which the
    last holds one row; C = 4 (one column, 256 row lanes) ... 256 (64 columns, 4 lanes); 17 and 20 columns leave threads idle;
    70 columns take the 4-byte path"""
    path, lanes, U, Rr = colsum_geometry(1, Cc)
    assert path == ("scalar" if Cc == 70 else "vector") and Rr == U
    for i, rows in enumerate(colsum_rows(Cc)):
        assert colsum_geometry(rows, Cc)[3] == U and R.cdiv(rows, U) == (3 if i == 4 else 2 if i == 3 else 1)
        check_colsum(K, rows, Cc, F32, 8000 + 16 * Cc + 2 * i)


def test_colsum_exact_bf16_maps(K):
    for i, rows in enumerate(colsum_rows(80)):
        check_colsum(K, rows, 80, BF16, 8500 + 2 * i)


@pytest.mark.parametrize("Cc", (4, 68))
def test_colsum_workgroups_of_two_passes(K, Cc):
    """enough rows that a workgroup's range is two unrolled passes, the last workgroup ragged"""
    _, _, U, _ = colsum_geometry(1, Cc)
    rows = COLSUM_WGS * U + 1
    assert colsum_geometry(rows, Cc)[3] == 2 * U and rows * R.DY_MAX < R.F32_EXACT
    check_colsum(K, rows, Cc, F32, 8600 + Cc)


def wide(seed, *shape):
    """small integers times powers of two up to 2^30: a sum of them depends on the order of its additions"""
    return R.ints(seed, -3, 3, *shape) * 2.0 ** R.ints(seed + 1, 0, 30, *shape)


def colsum_in_order(x, lanes):
    """one workgroup's column sums in fp32 in the order the kernel adds: each of `lanes` row lanes its rows l, l + lanes, ... in turn,
    then the lanes in turn (lanes = 1: the 4-byte path's one chain)"""
    parts = []
    for l in range(lanes):
        s = torch.zeros(x.shape[1])
        for r in range(l, x.shape[0], lanes):
            s = s + x[r]
        parts.append(s)
    t = parts[0]
    for p in parts[1:]:
        t = t + p
    return torch.zeros(x.shape[1]) + t


def test_colsum_routing(K):
    """59 rows -- one workgroup on either path -- of order-sensitive data: 68 columns carry the bits of the 15-lane order, 70 columns
    and a 68-column matrix that starts 4 bytes off a 16-byte boundary those of the single chain"""
    rows = 59
    for Cc, offset, path in ((68, 0, "vector"), (70, 0, "scalar"), (68, 1, "scalar")):
        got_path, lanes, U, _ = colsum_geometry(rows, Cc, aligned=offset == 0)
        assert got_path == path and rows < U
        x = wide(8700 + Cc + offset, rows, Cc)
        buf, = dev(torch.cat([torch.zeros(offset), x.reshape(-1)]))
        xg = buf[offset:].view(rows, Cc)
        assert xg.data_ptr() % 16 == 4 * offset
        out = nans((Cc,))
        K.call("erd_colsum", K._p(xg), rows, Cc, K._p(out), 0, 0, K._stream())
        want, other = colsum_in_order(x, lanes), colsum_in_order(x, 1 if lanes > 1 else 15)
        assert not torch.equal(want, other)                                   # the data tells the two orders apart
        assert_same(out, want, f"colsum {rows}x{Cc} offset {offset}: the {path} path's order")


# ---------------------------------------------------------------------------------------------
# per-level scale
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cc", (68, 6))
@pytest.mark.parametrize("ti", range(len(TABLES)))
def test_level_scale_at_ragged_levels(K, ti, Cc):
    """68 channels: the backward reads and writes float4s, four of each tensor in flight (a 128-row chunk is 2 176 float4s: two unrolled
    passes and a tail); 6 channels: its 4-byte form; the forward has one form.  Integers and power-of-two alphas: y, dx and the
    per-level sums are exact"""
    sizes = TABLES[ti]
    A, nseg = R.total_rows(sizes), len(sizes)
    what = f"level_scale {LEVEL_ROWS[ti]} C={Cc}"
    lv = K.make_levels(sizes)
    al = torch.tensor([GR.LEVEL_ALPHAS[i % 4] for i in range(nseg)])
    x, dy = R.ints(9000 + ti + Cc, -3, 3, N_IMG, A, Cc), R.ints(9100 + ti + Cc, -3, 3, N_IMG, A, Cc)
    assert N_IMG * max(h * w for h, w in sizes) * Cc * 9 < R.F32_EXACT
    xg, dyg, ag = dev(x, dy, al)
    y = nans(x.shape)
    K.call("erd_level_scale", K._p(xg), K._p(ag), K._p(y), N_IMG, A, Cc, C.byref(lv), K._stream())
    assert_same(y, GR.level_scale_ref(x, al, sizes), what + ": y")
    dx, dal = nans(x.shape), nans((nseg,))
    K.call("erd_level_scale_bwd", K._p(xg), K._p(dyg), K._p(ag), K._p(dx), K._p(dal), N_IMG, A, Cc, C.byref(lv), K._stream())
    dx_ref, dal_ref = GR.level_scale_bwd_ref(x, dy, al, sizes)
    assert_same(dx, dx_ref, what + ": dx")
    assert_same(dal, exact_f32(dal_ref, what), what + ": dalphas")
    assert_same(xg, x, what + ": x")
    # the middle level of image 0 alone
    j = nseg // 2
    sl = R.level_slices(sizes)[j]
    lv1 = one_level(sl.start, sl.stop - sl.start)
    a1, = dev(al[j:j + 1].contiguous())
    y, dx, dal = nans(x.shape), nans(x.shape), nans((1,))
    K.call("erd_level_scale", K._p(xg), K._p(a1), K._p(y), 1, A, Cc, C.byref(lv1), K._stream())
    K.call("erd_level_scale_bwd", K._p(xg), K._p(dyg), K._p(a1), K._p(dx), K._p(dal), 1, A, Cc, C.byref(lv1), K._stream())
    inside = torch.zeros(x.shape, dtype=torch.bool)
    inside[0, sl] = True
    for got, ref, name in ((y, GR.level_scale_ref(x, al, sizes), "y"), (dx, dx_ref, "dx")):
        assert bool((torch.isnan(got.cpu()) == ~inside).all()), (what, name)
        assert_same(got[0, sl], ref[0, sl].contiguous(), f"{what}: {name} of level {j}, image 0")
    assert_same(dal, exact_f32((dy[0, sl].double() * x[0, sl].double()).sum().reshape(1)), f"{what}: dalphas of level {j}, image 0")


def level_sum_in_order(x, dy, vec):
    """one workgroup's sum of dy * x (exact products) in the kernel's order: thread t of 256 adds its elements t, t + 256, ... (vec: its
    float4s, component by component) in turn, each wave folds its 64 lanes by xor 32, 16, ... 1, and the four waves are added in turn"""
    p = (dy.double() * x.double()).float().reshape(-1)
    assert torch.equal(p.double(), dy.double().reshape(-1) * x.double().reshape(-1))
    w = 4 if vec else 1
    n = R.cdiv(p.numel(), 256 * w) * 256 * w
    p = torch.cat([p, torch.zeros(n - p.numel())]).view(-1, 256, w)          # [pass, thread, component]; + 0.0 changes nothing
    acc = torch.zeros(256)
    for i in range(p.shape[0]):
        for k in range(w):
            acc = acc + p[i, :, k]
    acc = acc.view(4, 64)
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lane ^ o]
    return (torch.zeros(1) + (((acc[0, 0] + acc[1, 0]) + acc[2, 0]) + acc[3, 0])).reshape(1)


def test_level_scale_routing(K):
    """five levels of one chunk each, one image -- one workgroup per sum -- with order-sensitive dy: at 68 channels dalphas carries the
    bits of the float4 order, at 6 channels and for 68-channel buffers 4 bytes off a 16-byte boundary those of the 4-byte order"""
    sizes = [(1, 100), (1, 77), (1, 128), (1, 50), (1, 31)]
    A = R.total_rows(sizes)
    lv = K.make_levels(sizes)
    for Cc, offset, vec in ((68, 0, True), (6, 0, False), (68, 1, False)):
        x, dy = R.ints(9200 + Cc + offset, -3, 3, 1, A, Cc), wide(9300 + Cc + offset, 1, A, Cc)
        bx, bdy, bdx, ag = dev(torch.cat([torch.zeros(offset), x.reshape(-1)]), torch.cat([torch.zeros(offset), dy.reshape(-1)]),
                               torch.full((offset + x.numel(),), NAN), torch.full((len(sizes),), 2.0))
        xg, dyg, dx = (b[offset:].view(1, A, Cc) for b in (bx, bdy, bdx))
        assert xg.data_ptr() % 16 == 4 * offset
        dal = nans((len(sizes),))
        K.call("erd_level_scale_bwd", K._p(xg), K._p(dyg), K._p(ag), K._p(dx), K._p(dal), 1, A, Cc, C.byref(lv), K._stream())
        want, other = (torch.cat([level_sum_in_order(x[:, sl], dy[:, sl], v) for sl in R.level_slices(sizes)]) for v in (vec, not vec))
        assert not torch.equal(want, other)                                   # the data tells the two orders apart
        assert_same(dal, want, f"level_scale_bwd C={Cc} offset {offset}: the {'float4' if vec else '4-byte'} order")
        assert_same(dx.contiguous(), dy * 2.0, f"level_scale_bwd C={Cc} offset {offset}: dx")
        y = torch.full_like(bdx, NAN)[offset:].view(1, A, Cc)
        K.call("erd_level_scale", K._p(xg), K._p(ag), K._p(y), 1, A, Cc, C.byref(lv), K._stream())
        assert_same(y.contiguous(), x * 2.0, f"level_scale C={Cc} offset {offset}: y")
