"""GPU: the Winograd-domain weight gradient F(3x3, 2x2) of the BN-free 3x3 / stride-1 / pad-1 layers (erd_conv_wgrad_wino,
erd_wgrad_wino_reduce; erd_amd/csrc/wgrad_wino.hip).

Exact level.  With x in {-1, 0, 1} and dz in {-2 .. 2} every transformed value is a small multiple of 1/4 (|V| <= 4, |M| <= 2): one bf16
limb each, the other two zero, every product a multiple of 1/16 and every fp32 sum over the tiles of a case far below 2^24 / 16 -- exact
in any order.  The reduced dW must therefore EQUAL the integer weight gradient, from NaN-filled slabs into a NaN-filled output, at every
split count.  Shapes are the smallest that reach each path of the tile table: one K-step of 16 tiles and several, tiles half outside an
odd map, a map narrower than a K-step, K-steps that straddle tile rows, images and segments, a ragged last step, empty splits.

Real-valued level.  max |err| / max |dW| against the fp64 correlation, bound 4 x the direct three-tap kernel's figure on the same inputs
(floor 1e-6): the fp32 emulation of the transform gave 2.6 x, the rest is margin for the three-limb rounding of the transformed values.

Then a head-tower layer (HeadConvGN) and two trainer steps with the route on against off."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import golden_inputs as G
import wgrad_refs as R


@pytest.fixture()
def K():
    from erd_amd import kernels as K
    K.set_compute("f32x3")
    yield K
    K.set_compute(K.DEFAULT_COMPUTE)
    K.set_cu_reserve(0)


def _ntiles(N, sizes):
    return N * sum(((h + 1) // 2) * ((w + 1) // 2) for h, w in sizes)


def _correlation64(x, dz, N, sizes, Cin, Cout):
    """[Cout, 3, 3, Cin] fp64 on the CPU: sum over maps and pixels of dz[p, co] * x[p + tap, ci], pad 1"""
    ref = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64)
    o = 0
    for h, w in sizes:
        xl = x[:, o:o + h * w].reshape(N, h, w, Cin).permute(0, 3, 1, 2).double()
        dl = dz[:, o:o + h * w].reshape(N, h, w, Cout).permute(0, 3, 1, 2).double()
        ref += torch.nn.grad.conv2d_weight(xl, (Cout, Cin, 3, 3), dl, stride=1, padding=1)
        o += h * w
    return ref.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def _int_case(N, sizes, Cin, Cout):
    """integer operands on the GPU and the integer dW (computed once per shape, left unchanged)"""
    A = sum(h * w for h, w in sizes)
    g = torch.Generator().manual_seed(4000 + 7 * N + A + Cin + 3 * Cout)
    x = torch.randint(-1, 2, (N, A, Cin), generator=g).float()
    dz = torch.randint(-2, 3, (N, A, Cout), generator=g).float()
    ref = _correlation64(x, dz, N, sizes, Cin, Cout)
    assert float(ref.abs().max()) < 2 ** 20 and torch.equal(ref, ref.round())
    return x.cuda(), dz.cuda(), ref.float()


def _desc(K, xg, dg, sizes):
    xs, dzs = K.level_views(xg, sizes), K.level_views(dg, sizes)
    xoff = tuple((t.data_ptr() - xg.data_ptr()) // 4 for t in xs)
    zoff = tuple((t.data_ptr() - dg.data_ptr()) // 4 for t in dzs)
    d, _, _, _, _, Cout, Cin, row3 = K._wgrad_desc(xs, dzs, 3, 1, 1, xoff, zoff)
    assert row3 and d.limbs3 == 1
    d.x, d.dz = xg.data_ptr(), dg.data_ptr()
    return d, Cout, Cin


def _wino(K, xg, dg, sizes, nsplit, base=None):
    """erd_conv_wgrad_wino at a split count of our choosing into NaN-filled slabs, erd_wgrad_wino_reduce into a NaN-filled dW (or onto `base`)"""
    d, Cout, Cin = _desc(K, xg, dg, sizes)
    assert K._lib.load().erd_conv_wgrad_wino_ok(C.byref(d)) == 1
    d.nsplit = nsplit
    part = torch.full((nsplit, 16, Cout, Cin), float("nan"), device="cuda")
    d.part = part.data_ptr()
    K.call("erd_conv_wgrad_wino", C.byref(d), K._stream())
    dW = torch.full((Cout, 3, 3, Cin), float("nan"), device="cuda") if base is None else base.clone().cuda()
    K.wgrad_wino_reduce(part, nsplit, dW, base is not None)
    torch.cuda.synchronize()
    assert not torch.isnan(part).any()
    return dW.cpu()


SEG5 = ((13, 21), (7, 11), (4, 6), (5, 3), (2, 2))
EXACT = [
    # N, sizes, Cin, Cout, nsplit
    (1, ((8, 16),), 128, 128, 1),                # two whole K-steps of one map
    (1, ((8, 16),), 128, 256, 1),                # two tiles on the output side
    (1, ((8, 16),), 256, 128, 2),                # ... on the input side
    (1, ((7, 11),), 128, 128, 1),                # odd both ways: last tile row and column half outside
    (1, ((13, 21),), 128, 128, 2),
    (1, ((5, 3),), 128, 128, 1),                 # narrower than a K-step: 2 tiles per row, 6 in all
    (2, ((7, 11), (5, 3)), 128, 128, 2),         # K-steps straddle tile rows, images and the segment boundary
    (2, SEG5, 128, 128, 3),                      # five segments
    (1, ((8, 16),), 128, 128, 5),                # more splits than K-steps: three empty slabs
]


@pytest.mark.parametrize("N,sizes,Cin,Cout,nsplit", EXACT)
def test_integer_weight_gradient_is_exact(K, N, sizes, Cin, Cout, nsplit):
    xg, dg, ref = _int_case(N, sizes, Cin, Cout)
    steps = -(-_ntiles(N, sizes) // 16)
    print(f"N {N} sizes {sizes}: {_ntiles(N, sizes)} tiles, {steps} K-steps, nsplit {nsplit}")
    got = _wino(K, xg, dg, sizes, nsplit)
    assert torch.equal(got, ref), float((got - ref).abs().max())


def test_the_cases_are_what_they_claim():
    assert _ntiles(2, SEG5) % 16 != 0 and _ntiles(2, ((7, 11), (5, 3))) % 16 != 0 and _ntiles(1, ((5, 3),)) < 16
    assert -(-_ntiles(1, ((8, 16),)) // 16) < 5
    assert _ntiles(2, R.ROW3_SIZES) % 16 != 0


def test_integer_case_of_the_direct_kernels_suite(K):
    """tests/wgrad_refs.py's three-tap case (N = 2, maps 13x21, 7x11, 20x36) against ITS integer reference, and onto an integer base"""
    Cin = Cout = 128
    x, dz = R.inputs(R.ROW3_CASE, Cin, Cout)
    ref = R.wgrad_of(R.ROW3_CASE, Cin, Cout, range(R.pixels(R.ROW3_SIZES))).reshape(Cout, 3, 3, Cin)
    xg, dg = x.cuda(), dz.cuda()
    assert torch.equal(_wino(K, xg, dg, R.ROW3_SIZES, 4), ref)
    base = torch.randint(-50, 51, ref.shape, generator=torch.Generator().manual_seed(5)).float()
    assert torch.equal(_wino(K, xg, dg, R.ROW3_SIZES, 4, base=base), base + ref)


def test_split_counts_and_cu_reserve_give_the_identical_gradient(K):
    N, sizes = 2, SEG5
    xg, dg, ref = _int_case(N, sizes, 128, 128)
    for nsplit in (1, 3, 16):
        assert torch.equal(_wino(K, xg, dg, sizes, nsplit), ref), nsplit
    # the host path (its own split count, sized for the CUs in use) with and without a reserve
    xs, dzs = K.level_views(xg, sizes), K.level_views(dg, sizes)
    got = []
    for reserve in (0, 8):
        K.set_cu_reserve(reserve)
        assert K.conv_wgrad_wino_ok(xs, dzs)
        part, S = K.conv_wgrad_wino(xs, dzs)
        dW = torch.full((128, 3, 3, 128), float("nan"), device="cuda")
        K.wgrad_wino_reduce(part, S, dW, False)
        got.append((S, dW.cpu()))
    K.set_cu_reserve(0)
    print(f"host split counts: reserve 0 -> {got[0][0]}, reserve 8 -> {got[1][0]}")
    assert got[1][0] <= got[0][0] and got[0][0] * 4 <= 256
    assert torch.equal(got[0][1], ref) and torch.equal(got[1][1], ref)


def test_refusals_come_before_any_launch(K):
    xg, dg, _ = _int_case(1, ((8, 16),), 128, 128)
    lib = K._lib.load()
    part = torch.full((1, 16, 128, 128), float("nan"), device="cuda")

    def rc(**kw):
        d, _, _ = _desc(K, xg, dg, ((8, 16),))
        d.nsplit, d.part = 1, part.data_ptr()
        for k, v in kw.items():
            setattr(d, k, v)
        ok = lib.erd_conv_wgrad_wino_ok(C.byref(d))
        return ok, lib.erd_conv_wgrad_wino(C.byref(d), K._stream())

    for kw in (dict(x_bf16=1), dict(dz_bf16=1), dict(bf16_multiplicands=1), dict(Cin=64), dict(Cout=192), dict(in_stride=2), dict(ntaps=1),
               dict(ngroups=2), dict(part=None), dict(nsplit=0)):
        ok, code = rc(**kw)
        assert code != 0, kw
        assert ok == 0 or set(kw) <= {"part", "nsplit"}, kw
    torch.cuda.synchronize()
    assert torch.isnan(part).all()
    assert rc() == (1, 0)


# ---------------------------------------------------------------------------------------------------------------------
# real-valued data
# ---------------------------------------------------------------------------------------------------------------------
REAL_SIZES = ((25, 42), (13, 21))


@functools.lru_cache(maxsize=None)
def _real_case(C_):
    """x = ReLU of a normal, dz normal with half the entries zero and a nonzero mean in every fourth channel; fp64 dW on the CPU"""
    N, A = 2, sum(h * w for h, w in REAL_SIZES)
    x = G.randn(61, N, A, C_).clamp_min(0)
    dz = G.randn(62, N, A, C_)
    dz[..., ::4] += 0.5
    dz = dz * (G.randn(63, N, A, C_) > 0).float()
    return x.cuda(), dz.cuda(), _correlation64(x, dz, N, REAL_SIZES, C_, C_)


def _maxerr(a, ref):
    return float((a.double() - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("C_", [128, 256])
def test_real_valued_gradient_against_fp64(K, C_):
    xg, dg, ref = _real_case(C_)
    xs, dzs = K.level_views(xg, REAL_SIZES), K.level_views(dg, REAL_SIZES)
    part, S = K.conv_wgrad_partials(xs, dzs, 3, 1, 1)
    direct = torch.empty((C_, 3, 3, C_), device="cuda")
    K.wgrad_reduce(part, S, direct, None, direct, False, None)
    e_direct = _maxerr(direct.cpu(), ref)
    part, Sw = K.conv_wgrad_wino(xs, dzs)
    wino = torch.full((C_, 3, 3, C_), float("nan"), device="cuda")
    K.wgrad_wino_reduce(part, Sw, wino, False)
    again = torch.full((C_, 3, 3, C_), float("nan"), device="cuda")
    K.wgrad_wino_reduce(K.conv_wgrad_wino(xs, dzs)[0], Sw, again, False)
    e_wino = _maxerr(wino.cpu(), ref)
    print(f"{C_} -> {C_}, 2 x (25x42 + 13x21): max |err| / max |dW| against fp64: direct three-tap {e_direct:.3e} (S {S}) | "
          f"Winograd {e_wino:.3e} (S {Sw}) | ratio {e_wino / e_direct:.2f}")
    assert e_wino <= max(4 * e_direct, 1e-6), (e_wino, e_direct)
    assert torch.equal(wino, again)


# ---------------------------------------------------------------------------------------------------------------------
# a head-tower layer
# ---------------------------------------------------------------------------------------------------------------------
HEAD_SIZES = ((8, 12), (4, 6), (2, 3))


def _head_layer(K, Fn, on, monkeypatch):
    monkeypatch.setattr(Fn, "WGRAD_WINO", on)
    calls, seen = [], {}
    real, real_direct, real_wino = K.call, K.conv_wgrad_partials, K.conv_wgrad_wino

    def recording(name, *args):
        calls.append(name)
        return real(name, *args)

    def keep(fn):      # the weight gradient's operands (the layer's input and the gradient behind its GroupNorm), for the fp64 reference
        def wrapped(xs, dzs, *a, **kw):
            seen["x"], seen["dz"] = xs[0]._base.detach().cpu().clone(), dzs[0]._base.detach().cpu().clone()
            return fn(xs, dzs, *a, **kw)
        return wrapped

    monkeypatch.setattr(K, "call", recording)
    monkeypatch.setattr(K, "conv_wgrad_partials", keep(real_direct))
    monkeypatch.setattr(K, "conv_wgrad_wino", keep(real_wino))
    Cc, N, A = 256, 2, sum(h * w for h, w in HEAD_SIZES)
    x = G.randn(71, N, A, Cc).abs().cuda().requires_grad_(True)
    w = torch.nn.Parameter((G.randn(72, Cc, Cc, 3, 3) * (2.0 / (9 * Cc)) ** 0.5).cuda())
    gamma = torch.nn.Parameter((1.0 + 0.1 * G.randn(73, Cc)).cuda())
    beta = torch.nn.Parameter((0.1 * G.randn(74, Cc)).cuda())
    y = Fn.HeadConvGN.apply(x, w, gamma, beta, HEAD_SIZES, 1e-5)
    y.backward(G.randn(75, N, A, Cc).cuda())
    Fn.trail_join()
    torch.cuda.synchronize()
    for name, fn in (("call", real), ("conv_wgrad_partials", real_direct), ("conv_wgrad_wino", real_wino)):
        monkeypatch.setattr(K, name, fn)
    return [t.grad.detach().cpu().clone() for t in (x, w, gamma, beta)], calls, seen


def test_head_tower_layer_on_against_off(K, monkeypatch):
    """dx does not pass through the weight gradient: bit-equal, and so are the operands the layer hands to its weight gradient (the
    gradient behind the GroupNorm among them).  d gamma and d beta do not pass through it either, but gn_bwd_stats_kernel forms them with
    float atomics: two runs of the SAME path differ by a reordering of fp32 additions, so bit equality is not a
    property they have with the route off both times either (four runs of the direct path on one GPU: dx and dW bit-equal, d gamma and
    d beta differing from the first run by up to 7.7e-8 of the largest value).  They are held to the reordering bound tests/test_gpu_wgrad_grouped.py
    derives for its atomically summed 1-d gradients, 2 (n - 1) 2^-24 of the sum of magnitudes with n = 2 x 126 terms per channel here:
    3e-5, held to that test's 1e-4 of the largest value.
    dW: against the fp64 correlation of those operands, with the bound of the real-valued test."""
    from erd_amd import functional as Fn
    off, calls_off, seen_off = _head_layer(K, Fn, False, monkeypatch)
    on, calls_on, seen_on = _head_layer(K, Fn, True, monkeypatch)
    assert "erd_conv_wgrad" in calls_off and "erd_conv_wgrad_wino" not in calls_off
    assert "erd_conv_wgrad_wino" in calls_on and "erd_wgrad_wino_reduce" in calls_on and "erd_conv_wgrad" not in calls_on
    assert torch.equal(on[0], off[0]), "dx"
    for i, name in ((2, "dgamma"), (3, "dbeta")):
        d = float((on[i].double() - off[i].double()).abs().max() / off[i].double().abs().max())
        print(f"{name}: on against off {d:.3e} of the largest value")
        assert d < 1e-4, (name, d)
    assert torch.equal(seen_on["x"], seen_off["x"]) and torch.equal(seen_on["dz"], seen_off["dz"])
    ref = _correlation64(seen_on["x"], seen_on["dz"], 2, HEAD_SIZES, 256, 256)
    e_direct, e_wino = (_maxerr(g[1].permute(0, 2, 3, 1), ref) for g in (off, on))
    print(f"HeadConvGN 256 -> 256 at {HEAD_SIZES}, N = 2: dW max |err| / max |dW| against fp64: direct {e_direct:.3e} | Winograd {e_wino:.3e}")
    assert not torch.isnan(on[1]).any()
    assert e_wino <= max(4 * e_direct, 1e-6), (e_wino, e_direct)


# ---------------------------------------------------------------------------------------------------------------------
# trainer
# ---------------------------------------------------------------------------------------------------------------------
def test_trainer_steps_on_against_off(K, monkeypatch):
    """Two ERDTrainer steps on the small model, route on against off, in the manner of tests/test_gpu_wgrad_grouped.py: the gradient sync's
    diagnostics stay clean, and the second step's loss and the updated parameters agree to that test's 1e-6."""
    from e2e_util import build_erd, f7_state_dicts, make_samples
    from erd_amd import functional as Fn
    from erd_amd.engine import ERDTrainer
    from oracle import erd_oracle as O
    tsd, ssd = f7_state_dicts()
    batches = []
    for seed in (0, 1):
        imgs, boxes, labels = O.synthetic_batch(2, 123, 153, 40, seed=seed)
        x, metas = O.preprocess(imgs)
        batches.append((x.cuda(), make_samples(boxes, labels, metas)))
    got, losses, routed = [], [], []
    real = K.call
    for on in (False, True):
        monkeypatch.setattr(Fn, "WGRAD_WINO", on)
        n = [0]

        def recording(name, *args):
            n[0] += name == "erd_conv_wgrad_wino"
            return real(name, *args)

        monkeypatch.setattr(K, "call", recording)
        model = build_erd(tsd, ssd)
        tr = ERDTrainer(model, lr=0.02, batch_size_per_gpu=2, auto_scale_lr=False, warmup_iters=0, bucket_mb=1)
        per_step = []
        for b in batches:
            log = tr.train_step(*b)
            tr.flush()
            torch.cuda.synchronize()
            assert tr.sync.late_buckets == 0 and not tr.sync.missing and not tr.sync.repeats
            per_step.append(float(log["loss"]))
        monkeypatch.setattr(K, "call", real)
        losses.append(per_step)
        routed.append(n[0])
        got.append({k: p.detach().cpu().clone() for k, p in model.named_parameters() if p.requires_grad})
    print(f"losses off {losses[0]}, on {losses[1]}; Winograd-domain launches per two steps: off {routed[0]}, on {routed[1]}")
    assert routed[0] == 0 and routed[1] >= 2 * 8      # the eight head-tower layers of each step at least
    for step in (0, 1):      # (the first step's loss does not depend on the route at all)
        assert abs(losses[1][step] - losses[0][step]) <= 1e-6 * abs(losses[0][step]), losses
    errs = {k: float((got[1][k] - got[0][k]).abs().max() / (got[0][k].abs().max() + 1e-12)) for k in got[0]}
    worst = max(errs, key=errs.get)
    print(f"updated parameters on against off after two steps: worst {errs[worst]:.3e} ({worst})")
    assert all(torch.isfinite(p).all() for p in got[1].values())
    assert errs[worst] < 1e-6
