"""GPU: the grouped 3x3 convolution kernels (erd_amd/csrc/conv_grouped.hip; ResNeXt conv2) against torch's grouped convolution,
EXACTLY.  Activations in {-1, 0, 1}, weights in {-2 .. 2}, scales in {0.5, 1, 2}, integer shifts / residuals, masks in {-1, 0, 1}:
every partial sum is a small multiple of 1/2 far below 2^24 (|y| <= 9 * 32 * 2 * 2 at cg = 32 with a row scale of 2; weight-gradient
sums <= 1 836 pixels; <W, G> dots <= 288 * 2 * 1 836), so each element has ONE right value whatever the order of the additions -- a tap
or channel decoded wrongly, a group boundary crossed, a pixel of a stride-2 input gradient left unwritten (outputs start as NaN), an
epilogue step out of order or a split counted twice fails.  Column sums are compared as the sum over the replicated rows.
The launches go through kernels.conv_forward / conv_dgrad / conv_wgrad_partials + wgrad_reduce, and straight through the C ABI."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import grouped_refs as R

NAN = float("nan")
CASES = [(32, 4), (32, 8), (32, 16), (32, 32), (64, 4), (2, 4), (3, 8)]           # (cardinality, cg)
MAPS = [(1, 1, 1), (2, 2, 3), (1, 5, 7), (1, 8, 6), (3, 18, 34)]                  # (N, H, W) of the layer's INPUT: odd and even extents
PARAMS = [(card, cg, s) for card, cg in CASES for s in (1, 2)]


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


def pick(seed, values, *shape):
    g = torch.Generator().manual_seed(seed)
    return torch.tensor(values)[torch.randint(0, len(values), shape, generator=g)].float()


def out_hw(H, W, s):
    return (H - 1) // s + 1, (W - 1) // s + 1


def few_cus(K):
    """reserve all but 8 CUs; returns the usable count"""
    from erd_amd import _lib
    lib = _lib.load()
    K.set_cu_reserve(0)
    K.set_cu_reserve(int(lib.erd_usable_cus()) - 8)
    assert int(lib.erd_usable_cus()) == 8
    return 8


@pytest.mark.parametrize("card,cg,s", PARAMS)
def test_forward_is_the_integer_result(K, card, cg, s):
    Cc = card * cg
    for mi, (N, H, W) in enumerate(MAPS):
        seed = 1000 * cg + 10 * card + mi
        x, w = ints(seed, -1, 1, N, H, W, Cc), ints(seed + 1, -2, 2, Cc, 3, 3, cg)
        OH, OW = out_hw(H, W, s)
        scale, shift, res = pick(seed + 2, [0.5, 1.0, 2.0], Cc), ints(seed + 3, -3, 3, Cc), ints(seed + 4, -3, 3, N, OH, OW, Cc)
        y = R.conv_g(x, w, s, card)
        assert float(y.abs().max()) <= 9 * cg * 2
        xd, wd, sc, sh, rs = x.cuda(), w.cuda(), scale.cuda(), shift.cuda(), res.cuda()
        variants = {"plain": (None, None, None, False), "scale+shift+res+relu": (sc, sh, rs, True), "shift+relu": (None, sh, None, True),
                    "scale+res": (sc, None, rs, False)}
        got = {}
        for name, (a, b, r, relu) in variants.items():
            want = y.clone()
            if a is not None:
                want = want * scale.double()
            if b is not None:
                want = want + shift.double()
            if r is not None:
                want = want + res.double()
            if relu:
                want = want.clamp(min=0)
            out = torch.full((N, OH, OW, Cc), NAN, device="cuda")
            K.conv_forward([xd], wd, [out], 3, s, 1, scale=a, shift=b, res=None if r is None else [r], relu=relu)
            assert_exact(out, want.float(), f"forward {card}x{cg} stride {s} map {(N, H, W)} {name}")
            got[name] = out
        few_cus(K)      # the same bits on 8 CUs: nothing depends on the grid
        out = torch.full((N, OH, OW, Cc), NAN, device="cuda")
        K.conv_forward([xd], wd, [out], 3, s, 1, scale=sc, shift=sh, res=[rs], relu=True)
        assert_exact(out, got["scale+shift+res+relu"], f"forward {card}x{cg} stride {s} map {(N, H, W)} on 8 CUs")
        K.set_cu_reserve(0)


@pytest.mark.parametrize("card,cg,s", PARAMS)
def test_input_gradient_is_the_integer_result(K, card, cg, s):
    Cc = card * cg
    for mi, (N, H, W) in enumerate(MAPS):
        seed = 2000 * cg + 10 * card + mi
        OH, OW = out_hw(H, W, s)
        dz, w = ints(seed, -1, 1, N, OH, OW, Cc), ints(seed + 1, -2, 2, Cc, 3, 3, cg)
        rowscale = pick(seed + 2, [0.5, 1.0, 2.0], Cc)
        res, base, mask = ints(seed + 3, -3, 3, N, H, W, Cc), ints(seed + 4, -3, 3, N, H, W, Cc), ints(seed + 5, -1, 1, N, H, W, Cc)
        g_plain = R.conv_g_dgrad(dz, w, (H, W), s, card)
        g_scaled = R.conv_g_dgrad(dz, w * rowscale.view(Cc, 1, 1, 1), (H, W), s, card)
        dzd, wd, rsd = dz.cuda(), w.cuda(), rowscale.cuda()
        what = f"input gradient {card}x{cg} stride {s} map {(N, H, W)}"

        dx = torch.full((N, H, W, Cc), NAN, device="cuda")
        K.conv_dgrad([dzd], wd, [dx], 3, s, 1, cardinality=card)
        assert_exact(dx, g_plain.float(), what + " plain")

        dx = base.cuda()
        K.conv_dgrad([dzd], wd, [dx], 3, s, 1, accumulate=True, cardinality=card, rowscale=rsd)
        assert_exact(dx, (g_scaled + base.double()).float(), what + " accumulate")

        dx = torch.full((N, H, W, Cc), NAN, device="cuda")
        K.conv_dgrad([dzd], wd, [dx], 3, s, 1, res=[res.cuda()], cardinality=card, rowscale=rsd)
        assert_exact(dx, (g_scaled + res.double()).float(), what + " res")

        want = ((g_scaled + res.double()) * (mask > 0).double()).float()
        got = {}
        for copies in (1, 8):
            dx = torch.full((N, H, W, Cc), NAN, device="cuda")
            cs = torch.zeros(copies, Cc, device="cuda")
            K.conv_dgrad([dzd], wd, [dx], 3, s, 1, res=[res.cuda()], relu_mask=[mask.cuda()], colsum=cs, cardinality=card, rowscale=rsd)
            assert_exact(dx, want, what + f" res + mask + colsum ({copies} rows)")
            assert_exact(cs.sum(0), want.double().sum((0, 1, 2)).float(), what + f" column sums ({copies} rows)")
            got[copies] = dx
        few_cus(K)
        dx = torch.full((N, H, W, Cc), NAN, device="cuda")
        cs = torch.zeros(8, Cc, device="cuda")
        K.conv_dgrad([dzd], wd, [dx], 3, s, 1, res=[res.cuda()], relu_mask=[mask.cuda()], colsum=cs, cardinality=card, rowscale=rsd)
        assert_exact(dx, got[8], what + " on 8 CUs")
        assert_exact(cs.sum(0), want.double().sum((0, 1, 2)).float(), what + " column sums on 8 CUs")
        K.set_cu_reserve(0)


@pytest.mark.parametrize("card,cg,s", PARAMS)
def test_weight_gradient_is_the_integer_result(K, card, cg, s):
    Cc = card * cg
    for mi, (N, H, W) in enumerate(MAPS):
        seed = 3000 * cg + 10 * card + mi
        OH, OW = out_hw(H, W, s)
        x, dz, w = ints(seed, -1, 1, N, H, W, Cc), ints(seed + 1, -1, 1, N, OH, OW, Cc), ints(seed + 2, -2, 2, Cc, 3, 3, cg)
        rowscale, slot = pick(seed + 3, [0.5, 1.0, 2.0], Cc), ints(seed + 4, -3, 3, Cc, 3, 3, cg)
        G = R.conv_g_wgrad(x, dz, s, card)
        assert float(G.abs().max()) <= N * OH * OW
        what = f"weight gradient {card}x{cg} stride {s} map {(N, H, W)}"
        xd, dzd, wd = x.cuda(), dz.cuda(), w.cuda()
        for reserve in (False, True):
            if reserve:
                few_cus(K)
            part, S = K.conv_wgrad_partials([xd], [dzd], 3, s, 1, cardinality=card)
            assert part.numel() >= S * Cc * 9 * cg and 1 <= S <= max(1, N * OH * OW // 16)
            dW = torch.full((Cc, 3, 3, cg), NAN, device="cuda")
            K.wgrad_reduce(part, S, wd, None, dW, False, None)
            assert_exact(dW, G.float(), what + f" fresh (S = {S})")
            dW = slot.cuda()
            dots = torch.full((Cc,), NAN, device="cuda")
            K.wgrad_reduce(part, S, wd, rowscale.cuda(), dW, True, dots)
            assert_exact(dW, (slot.double() + G * rowscale.double().view(Cc, 1, 1, 1)).float(), what + f" row scale, accumulated (S = {S})")
            assert_exact(dots, (G * w.double()).sum((1, 2, 3)).float(), what + f" <W, G> dots (S = {S})")
        K.set_cu_reserve(0)


def _desc(inp, out, w, N, H, W, Cc, cg, s):
    from erd_amd import _lib
    d = _lib.ConvGroupedDesc()
    OH, OW = out_hw(H, W, max(s, 1))
    d.inp, d.out, d.w = inp.data_ptr(), out.data_ptr(), w.data_ptr()
    d.N, d.IH, d.IW, d.OH, d.OW, d.C, d.cg, d.stride = N, H, W, OH, OW, Cc, cg, s
    return d


def test_c_abi_launches_and_rejects_what_is_out_of_scope(K):
    from erd_amd import _lib
    lib = _lib.load()
    N, H, W, card, cg = 2, 5, 6, 3, 8
    Cc = card * cg
    x, w = ints(1, -1, 1, N, H, W, Cc).cuda(), ints(2, -2, 2, Cc, 3, 3, cg).cuda()
    st = K._stream()
    for s in (1, 2):
        OH, OW = out_hw(H, W, s)
        out = torch.full((N, OH, OW, Cc), NAN, device="cuda")
        assert lib.erd_conv_grouped_fwd(C.byref(_desc(x, out, w, N, H, W, Cc, cg, s)), st) == 0
        assert_exact(out, R.conv_g(x.cpu(), w.cpu(), s, card).float(), f"C ABI forward stride {s}")
        dx = torch.full((N, H, W, Cc), NAN, device="cuda")
        assert lib.erd_conv_grouped_dgrad(C.byref(_desc(out, dx, w, N, H, W, Cc, cg, s)), st) == 0
        assert_exact(dx, R.conv_g_dgrad(out.cpu(), w.cpu(), (H, W), s, card).float(), f"C ABI input gradient stride {s}")
        part = torch.full((3, Cc, 9 * cg), NAN, device="cuda")
        assert lib.erd_conv_grouped_wgrad(x.data_ptr(), out.data_ptr(), part.data_ptr(), N, H, W, Cc, cg, s, 3, st) == 0
        assert_exact(part.sum(0).view(Cc, 3, 3, cg), R.conv_g_wgrad(x.cpu(), out.cpu(), s, card).float(), f"C ABI weight gradient stride {s}")
    out = torch.zeros((N, H, W, Cc), device="cuda")
    bad = [(_desc(x, out, w, N, H, W, Cc, 6, 1), "channels per group"),        # cg outside {4, 8, 16, 32}
           (_desc(x, out, w, N, H, W, 64, 64, 1), "channels per group"),       # cg = 64 (32x8d)
           (_desc(x, out, w, N, H, W, 8, 8, 1), "cardinality"),                # a dense convolution
           (_desc(x, out, w, N, H, W, Cc, cg, 3), "stride"),
           (_desc(x, out, w, 0, H, W, Cc, cg, 1), "empty")]
    for d, word in bad:
        for fn in (lib.erd_conv_grouped_fwd, lib.erd_conv_grouped_dgrad):
            assert fn(C.byref(d), st) < 0
            assert word in lib.erd_last_error().decode(), (word, lib.erd_last_error())
    d = _desc(x, out, w, N, H, W, Cc, cg, 1)
    d.OH += 1
    assert lib.erd_conv_grouped_fwd(C.byref(d), st) == -1 and "does not belong" in lib.erd_last_error().decode()      # ERD_EINVAL
    d = _desc(x, out, w, N, H, W, Cc, cg, 1)
    d.w = 0
    assert lib.erd_conv_grouped_dgrad(C.byref(d), st) < 0 and "null" in lib.erd_last_error().decode()
    assert lib.erd_conv_grouped_wgrad(x.data_ptr(), out.data_ptr(), 0, N, H, W, Cc, cg, 1, 4, st) < 0
    assert lib.erd_conv_grouped_wgrad(x.data_ptr(), out.data_ptr(), out.data_ptr(), N, H, W, Cc, cg, 1, 0, st) < 0
    assert lib.erd_conv_grouped_wgrad(x.data_ptr(), out.data_ptr(), out.data_ptr(), N, H, W, Cc, 64, 1, 4, st) < 0
    torch.cuda.synchronize()


def test_f32_and_f32x3_modes_share_the_launch_and_bf16_is_refused(K):
    N, H, W, card, cg = 2, 9, 11, 32, 4
    Cc = card * cg
    g = torch.Generator().manual_seed(3)
    x, w = torch.randn(N, H, W, Cc, generator=g).cuda(), (0.2 * torch.randn(Cc, 3, 3, cg, generator=g)).cuda()
    outs = {}
    for mode in ("f32", "f32x3"):
        K.set_compute(mode)
        outs[mode] = torch.full((N, H, W, Cc), NAN, device="cuda")
        K.conv_forward([x], w, [outs[mode]], 3, 1, 1, relu=True)
    assert_exact(outs["f32"], outs["f32x3"], "conv2 in the modes f32 / f32x3")
    K.set_compute("bf16")
    out = torch.empty((N, H, W, Cc), device="cuda")
    with pytest.raises(NotImplementedError, match="bf16"):
        K.conv_forward([x], w, [out], 3, 1, 1)
    with pytest.raises(NotImplementedError, match="bf16"):
        K.conv_dgrad([out], w, [x.clone()], 3, 1, 1, cardinality=card)
    with pytest.raises(NotImplementedError, match="bf16"):
        K.conv_wgrad_partials([x], [out], 3, 1, 1, cardinality=card)
