"""GPU: the deformable-convolution kernels (erd_amd/csrc/conv_deform.hip) and their kernels.py wrappers against the fp64 restatement
(tests/deform_refs.py), EXACTLY.  x in {-1, 0, 1}; offsets are multiples of 0.5 in [-2.5, 2.5], 5 % of them multiples of 0.5 in
[-40, 40] and a handful +-3e9; dcol, dz in {-1, 0, 1}; weights in {-2 .. 2}.  Every bilinear weight is then in {0, 1/4, 1/2, 1}, every
col element a multiple of 1/4 with |.| <= 1, dx a multiple of 1/4, doffset a multiple of 1/2 with |.| <= 2 C and layer outputs
|.| <= 9 * C * 2 -- all far below 2^24 (each test asserts the sum of magnitudes it relies on), so every element has ONE right value
whatever the order of the additions or of the atomics: a wrong tap, corner, boundary rule, channel or a missed accumulation fails.
Outputs start as NaN (they must be written in full), dx starts from an integer base (it accumulates), and everything is repeated with
all but 8 CUs reserved."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import deform_refs as R

NAN = float("nan")
MAPS = [(1, 1, 1), (2, 2, 3), (1, 5, 7), (1, 8, 6), (3, 18, 34)]      # (N, H, W) of the layer's INPUT
PARAMS = [(c, s) for c in (64, 128, 512) for s in (1, 2)]
EXACT_BELOW = float(2 ** 22)      # sums of multiples of 1/4 whose magnitudes add up to less are exact in fp32 in any order


@pytest.fixture()
def K():
    from erd_amd import kernels as K
    reserve = K.set_cu_reserve(0)
    yield K
    K.set_cu_reserve(reserve)
    K.set_compute(K.DEFAULT_COMPUTE)


def assert_exact(got, want, what):
    """every element equal, none NaN; the message names the first element that differs"""
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not torch.equal(got, want):
        bad = ~(got == want)
        first = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ ({int(torch.isnan(got).sum())} NaN); first at "
                             f"{first}: got {float(got[first])}, want {float(want[first])}")


def ints(seed, lo, hi, *shape):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def make_offsets(seed, N, OH, OW):
    g = torch.Generator().manual_seed(seed)
    off = torch.randint(-5, 6, (N, OH, OW, 18), generator=g).float() * 0.5
    far = torch.randint(-80, 81, (N, OH, OW, 18), generator=g).float() * 0.5
    off = torch.where(torch.rand((N, OH, OW, 18), generator=g) < 0.05, far, off)
    flat = off.view(-1)
    where = torch.randperm(flat.numel(), generator=g)[:4]
    flat[where] = torch.tensor([3e9, -3e9, 3e9, -3e9])[:where.numel()]
    return off


def few_cus(K):
    from erd_amd import _lib
    lib = _lib.load()
    K.set_cu_reserve(0)
    K.set_cu_reserve(int(lib.erd_usable_cus()) - 8)
    assert int(lib.erd_usable_cus()) == 8


@functools.lru_cache(maxsize=None)
def fixture(Cc, s, mi):
    """inputs and fp64 references of one case, computed once and shared by the tests (never modified)"""
    N, H, W = MAPS[mi]
    OH, OW = R.out_hw(H, W, s)
    seed = 100 * Cc + 10 * mi + s
    x, off = ints(seed, -1, 1, N, H, W, Cc), make_offsets(seed + 1, N, OH, OW)
    dcol, base = ints(seed + 2, -1, 1, N, OH, OW, 9 * Cc), ints(seed + 3, -3, 3, N, H, W, Cc)
    col = R.deform_cols(x, off, s)
    assert torch.equal(R.deform_cols(x, off, s, torch.float32).double(), col), "the fixture is not exact in fp32"
    assert float(col.abs().max()) <= 1 and torch.equal(col * 4, torch.round(col * 4))
    dx, doff = R.deform_cols_bwd(dcol, x, off, s)
    dx_abs, _ = R.deform_cols_bwd(dcol.abs(), x.abs(), off, s)
    assert float(dx_abs.max()) + 3 < EXACT_BELOW and float(R.deform_doffset_abs(dcol, x, off, s).max()) < EXACT_BELOW
    assert float(doff.abs().max()) <= 2 * Cc          # (every term: |g| <= 1, |x10 - x00| <= 2)
    return dict(N=N, H=H, W=W, OH=OH, OW=OW, x=x, off=off, dcol=dcol, base=base, col=col.reshape(N, OH, OW, 9 * Cc).float(),
                dx=(dx + base.double()).float(), doff=doff.float())


def test_the_fixture_is_not_degenerate():
    f = fixture(64, 1, 4)
    assert float((f["col"] != 0).float().mean()) > 0.4 and float((f["doff"] != 0).float().mean()) > 0.4
    assert float((f["off"].abs() > 1e9).sum()) == 4 and float((f["off"].abs() > 2.5).float().mean()) > 0.02


@pytest.mark.parametrize("Cc,s", PARAMS)
def test_sampling_kernel_is_the_exact_result(K, Cc, s):
    from erd_amd import _lib
    lib = _lib.load()
    for mi in range(len(MAPS)):
        f = fixture(Cc, s, mi)
        what = f"col C {Cc} stride {s} map {MAPS[mi]}"
        x, off = f["x"].cuda(), f["off"].cuda()
        col = torch.full(f["col"].shape, NAN, device="cuda")
        assert lib.erd_deform_cols(x.data_ptr(), off.data_ptr(), col.data_ptr(), f["N"], f["H"], f["W"], Cc, s, K._stream()) == 0
        assert_exact(col, f["col"], what + " (C ABI)")
        out = torch.full(f["col"].shape, NAN, device="cuda")
        assert K.deform_cols(x, off, s, out=out) is out
        assert_exact(out, f["col"], what + " (wrapper)")
        assert_exact(K.deform_cols(x, off, s), f["col"], what + " (workspace)")
        few_cus(K)
        out = torch.full(f["col"].shape, NAN, device="cuda")
        K.deform_cols(x, off, s, out=out)
        assert_exact(out, f["col"], what + " on 8 CUs")
        K.set_cu_reserve(0)


@pytest.mark.parametrize("Cc,s", PARAMS)
def test_backward_kernel_is_the_exact_result_and_accumulates(K, Cc, s):
    from erd_amd import _lib
    lib = _lib.load()
    for mi in range(len(MAPS)):
        f = fixture(Cc, s, mi)
        what = f"C {Cc} stride {s} map {MAPS[mi]}"
        x, off, dcol = f["x"].cuda(), f["off"].cuda(), f["dcol"].cuda()
        dx, doff = f["base"].cuda(), torch.full(f["off"].shape, NAN, device="cuda")
        assert lib.erd_deform_cols_bwd(dcol.data_ptr(), x.data_ptr(), off.data_ptr(), dx.data_ptr(), doff.data_ptr(), f["N"], f["H"], f["W"],
                                       Cc, s, K._stream()) == 0
        assert_exact(dx, f["dx"], "dx " + what + " (C ABI)")
        assert_exact(doff, f["doff"], "doffset " + what + " (C ABI)")
        for reserve in (False, True):
            if reserve:
                few_cus(K)
            dx, doff = f["base"].cuda(), torch.full(f["off"].shape, NAN, device="cuda")
            assert K.deform_cols_bwd(dcol, x, off, s, dx, doff) is doff
            assert_exact(dx, f["dx"], "dx " + what + (" on 8 CUs" if reserve else " (wrapper)"))
            assert_exact(doff, f["doff"], "doffset " + what + (" on 8 CUs" if reserve else " (wrapper)"))
        K.set_cu_reserve(0)


@pytest.mark.parametrize("Cc,s", PARAMS)
def test_layer_trio_is_the_exact_result(K, Cc, s):
    """deform_conv3x3_forward / _dgrad / _wgrad_partials + wgrad_reduce: the sampling kernels composed with the 1x1 launch forms"""
    Cout = Cc
    for mi in range(len(MAPS)):
        f = fixture(Cc, s, mi)
        N, H, W, OH, OW = f["N"], f["H"], f["W"], f["OH"], f["OW"]
        what = f"C {Cc} stride {s} map {MAPS[mi]}"
        seed = 7 * Cc + mi + s
        w = ints(seed, -2, 2, Cout, 3, 3, Cc)                  # OHWI
        scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (Cout,), generator=torch.Generator().manual_seed(seed + 1))]
        shift, dz = ints(seed + 2, -3, 3, Cout), ints(seed + 3, -1, 1, N, OH, OW, Cout)
        x, off = f["x"].cuda(), f["off"].cuda()
        w2 = w.view(Cout, 9 * Cc).double()
        y = f["col"].double() @ w2.t()
        assert float(y.abs().max()) <= 9 * Cc * 2
        out = torch.full((N, OH, OW, Cout), NAN, device="cuda")
        K.deform_conv3x3_forward(x, off, w.cuda(), out, s, scale=scale.cuda(), shift=shift.cuda(), relu=True)
        assert_exact(out, (y * scale.double() + shift.double()).clamp(min=0).float(), "forward " + what)
        # input and offset gradients: dcol = dz . W (integers, |.| <= 2 Cout), then the scatter onto an integer base
        dcol = dz.double() @ w2
        dx_ref, doff_ref = R.deform_cols_bwd(dcol, f["x"], f["off"], s)
        dx_abs, _ = R.deform_cols_bwd(dcol.abs(), f["x"].abs(), f["off"], s)
        assert float(dx_abs.max()) + 3 < 2 ** 22 and float(R.deform_doffset_abs(dcol, f["x"], f["off"], s).max()) < 2 ** 22
        dx = f["base"].cuda()
        doff = K.deform_conv3x3_dgrad(dz.cuda(), w.cuda(), None, x, off, s, dx)
        assert_exact(dx, (dx_ref + f["base"].double()).float(), "dx " + what)
        assert_exact(doff, doff_ref.float(), "doffset " + what)
        # weight gradient: partial slabs over the re-gathered columns, folded against the parameter's own view
        G = (dz.double().reshape(-1, Cout).t() @ f["col"].double().reshape(-1, 9 * Cc)).view(Cout, 3, 3, Cc)
        part, S = K.deform_conv3x3_wgrad_partials(x, off, dz.cuda(), s)
        dW = torch.full((Cout, 3, 3, Cc), NAN, device="cuda")
        dots = torch.full((Cout,), NAN, device="cuda")
        K.wgrad_reduce(part, S, w.cuda(), scale.cuda(), dW, False, dots)
        assert_exact(dW, (G * scale.double().view(Cout, 1, 1, 1)).float(), f"weight gradient {what} (S = {S})")
        assert_exact(dots, (G * w.double()).sum((1, 2, 3)).float(), f"<W, G> dots {what} (S = {S})")


def test_entry_points_refuse_what_is_out_of_scope(K):
    from erd_amd import _lib
    lib = _lib.load()
    st = K._stream()
    buf = torch.zeros(1 << 16, device="cuda")
    p = buf.data_ptr()
    cases = [((1, 4, 4, 6, 1), "multiple of 4"), ((1, 4, 4, 64, 3), "stride"), ((0, 4, 4, 64, 1), "empty"),
             ((64, 1024, 1024, 64, 1), "too large"), ((1, 1 << 12, 1 << 12, 64, 1), "too large")]      # x, and col alone, past 2^31
    for (N, H, W, Cc, s), word in cases:
        assert lib.erd_deform_cols(p, p, p, N, H, W, Cc, s, st) < 0
        assert word in lib.erd_last_error().decode(), (word, lib.erd_last_error())
        assert lib.erd_deform_cols_bwd(p, p, p, p + 256, p, N, H, W, Cc, s, st) < 0
        assert word in lib.erd_last_error().decode(), (word, lib.erd_last_error())
    assert lib.erd_deform_cols(p, 0, p, 1, 4, 4, 64, 1, st) < 0 and "null" in lib.erd_last_error().decode()
    assert lib.erd_deform_cols_bwd(p, p, p, p, p, 1, 4, 4, 64, 1, st) < 0 and "alias" in lib.erd_last_error().decode()
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0, "a refused launch wrote"
    x, off = torch.zeros(1, 4, 4, 6, device="cuda"), torch.zeros(1, 4, 4, 18, device="cuda")
    with pytest.raises(_lib.ErdHipError, match="multiple of 4"):
        K.deform_cols(x, off, 1)


def test_bf16_mode_is_refused(K):
    x, off = torch.zeros(1, 4, 4, 64, device="cuda"), torch.zeros(1, 4, 4, 18, device="cuda")
    w, out = torch.zeros(64, 3, 3, 64, device="cuda"), torch.zeros(1, 4, 4, 64, device="cuda")
    K.set_compute("bf16")
    with pytest.raises(NotImplementedError, match="bf16"):
        K.deform_cols(x, off, 1)
    with pytest.raises(NotImplementedError, match="bf16"):
        K.deform_cols_bwd(torch.zeros(1, 4, 4, 576, device="cuda"), x, off, 1, torch.zeros_like(x))
    with pytest.raises(NotImplementedError, match="bf16"):
        K.deform_conv3x3_forward(x, off, w, out, 1)
    with pytest.raises(NotImplementedError, match="bf16"):
        K.deform_conv3x3_dgrad(out, w, None, x, off, 1, torch.zeros_like(x))
    with pytest.raises(NotImplementedError, match="bf16"):
        K.deform_conv3x3_wgrad_partials(x, off, out, 1)
