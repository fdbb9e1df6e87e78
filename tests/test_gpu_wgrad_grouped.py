"""GPU: grouped launches of the three-limb weight-gradient kernels (erd_wgrad_desc::ngroups, erd_wgrad_reduce_grouped) and the
stage-level collector that feeds them (functional._WgradGroups).

Native level: ONE grouped launch into NaN-filled slabs plus ONE grouped reduce against G separate erd_conv_wgrad + erd_wgrad_reduce
calls at the same nsplit -- nothing inside a split changes, so dW (and the row dots: K <= 1024 is one block per row, no atomics between
blocks) must be BIT-equal and no NaN may be left.  The groups' tensors are separate allocations and their base pointers are handed over
in descending address order.  Shapes as in test_gpu_wgrad_tables.py: chosen to break the tables (ragged last slice, ragged channel
tiles, an empty last split, a map narrower than 16 pixels, two row chunks with a ragged second one), not to load the chip.

Stage level: a ResLayerFn backward with Fn.WGRAD_GROUPED on against off.  Trainer level: two ERDTrainer steps with the per-bucket
update, where a parameter must not report before the launches of its gradient are queued (BucketedGradSync)."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import golden_inputs as G

NAN = float("nan")


@pytest.fixture()
def K():
    from erd_amd import kernels as K
    yield K
    K.set_compute(K.DEFAULT_COMPUTE)


# name: (N, H, W, Cin, Cout, k, pad, row3)
CASES = {
    "one_tap_9x13": (2, 9, 13, 132, 68, 1, 0, False),      # 234 pixels = 15 slices, the last one ragged; ragged channel tiles
    "one_tap_9x9": (1, 9, 9, 132, 68, 1, 0, False),        # 81 pixels = 6 slices: nsplit 4 leaves the last split empty
    "one_tap_7x5": (3, 7, 5, 132, 68, 1, 0, False),        # narrower than 16 pixels: the per-lane decode
    "row3_co36": (2, 10, 21, 68, 36, 3, 1, True),          # two row chunks, the second ragged; the 64-row form
    "row3_co132": (2, 10, 21, 68, 132, 3, 1, True),        # ... the 128-row form
}
RUNS = ([("one_tap_9x13", g, s) for g in (1, 2, 3, 5) for s in (1, 2, 4)] + [("one_tap_9x9", 3, 4), ("one_tap_7x5", 2, 2)]
        + [(c, g, s) for c in ("row3_co36", "row3_co132") for g in (2, 3) for s in (1, 3)])


def test_the_cases_are_what_they_claim():
    N, H, W = CASES["one_tap_9x13"][:3]
    assert (N * H * W + 15) // 16 == 15 and N * H * W % 16 != 0
    N, H, W = CASES["one_tap_9x9"][:3]
    ns = (N * H * W + 15) // 16
    per = -(-ns // 4)
    assert ns == 6 and 3 * per >= ns > 2 * per                  # nsplit 4: exactly the last split is empty
    assert CASES["one_tap_7x5"][2] < 16
    assert -(-CASES["row3_co36"][2] // 16) == 2 and CASES["row3_co36"][2] % 16 != 0
    assert CASES["row3_co36"][4] <= 64 < CASES["row3_co132"][4]
    for c in CASES.values():
        assert c[5] * c[5] * c[3] <= 1024                       # one reduce block per row: rowdot is deterministic


@functools.lru_cache(maxsize=None)
def _inputs(case, Gn):
    """Gn separately allocated (x, dz) pairs in DESCENDING address order, one w / rowscale for the reduce options"""
    N, H, W, Cin, Cout, k, pad, _ = CASES[case]
    xs = [G.randn(61 + 2 * g, N, H, W, Cin).cuda() for g in range(Gn)]
    zs = [G.randn(62 + 2 * g, N, H, W, Cout).cuda() for g in range(Gn)]
    xs.sort(key=lambda t: -t.data_ptr())
    zs.sort(key=lambda t: -t.data_ptr())
    w = [G.randn(91 + g, Cout, k, k, Cin).cuda() for g in range(Gn)]
    rs = [(G.randn(95 + g, Cout).abs() + 0.5).cuda() for g in range(Gn)]
    pre = [G.randn(99 + g, Cout, k, k, Cin).cuda() for g in range(Gn)]
    return xs, zs, w, rs, pre


def _desc(K, case, x, dz, nsplit):
    N, H, W, Cin, Cout, k, pad, row3 = CASES[case]
    K.set_compute("f32x3")
    d, _, _, _, _, _, _, is_row3 = K._wgrad_desc([x], [dz], k, 1, pad, (0,), (0,))
    assert d.limbs3 == 1 and is_row3 == row3 and d.ngroups == 1
    d.x, d.dz, d.nsplit = x.data_ptr(), dz.data_ptr(), nsplit
    return d


def _separate(K, case, Gn, nsplit, rowscale, accumulate, rowdot):
    N, H, W, Cin, Cout, k, pad, _ = CASES[case]
    xs, zs, w, rs, pre = _inputs(case, Gn)
    out = []
    for g in range(Gn):
        d = _desc(K, case, xs[g], zs[g], nsplit)
        part = torch.full((nsplit, Cout, k * k, Cin), NAN, device="cuda")
        d.part = part.data_ptr()
        K.call("erd_conv_wgrad", C.byref(d), K._stream())
        dW = pre[g].clone() if accumulate else torch.full((Cout, k, k, Cin), NAN, device="cuda")
        rd = torch.full((Cout,), NAN, device="cuda") if rowdot else None
        K.wgrad_reduce(part, nsplit, w[g], rs[g] if rowscale else None, dW, accumulate, rd)
        torch.cuda.synchronize()
        out.append((dW.cpu(), None if rd is None else rd.cpu()))
    return out


def _grouped(K, case, Gn, nsplit, rowscale, accumulate, rowdot):
    N, H, W, Cin, Cout, k, pad, _ = CASES[case]
    xs, zs, w, rs, pre = _inputs(case, Gn)
    d = _desc(K, case, xs[0], zs[0], nsplit)
    d.x = d.dz = 0                      # a grouped launch reads the per-group pointers only
    d.ngroups = Gn
    if Gn == 1:
        d.x, d.dz = xs[0].data_ptr(), zs[0].data_ptr()
    for g in range(Gn):
        d.gx[g], d.gdz[g] = xs[g].data_ptr(), zs[g].data_ptr()
    assert Gn == 1 or all(d.gx[g] > d.gx[g + 1] and d.gdz[g] > d.gdz[g + 1] for g in range(Gn - 1))
    part = torch.full((Gn * nsplit, Cout, k * k, Cin), NAN, device="cuda")
    d.part = part.data_ptr()
    K.call("erd_conv_wgrad", C.byref(d), K._stream())
    dWs = [pre[g].clone() if accumulate else torch.full((Cout, k, k, Cin), NAN, device="cuda") for g in range(Gn)]
    rds = [torch.full((Cout,), NAN, device="cuda") if rowdot else None for g in range(Gn)]
    K.wgrad_reduce_grouped(part, nsplit, w[:Gn], [rs[g] if rowscale else None for g in range(Gn)], dWs, accumulate, rds)
    torch.cuda.synchronize()
    assert not torch.isnan(part).any(), "a slab of the grouped launch was not written"
    return [(dWs[g].cpu(), None if rds[g] is None else rds[g].cpu()) for g in range(Gn)]


def _compare(K, case, Gn, nsplit, rowscale, accumulate, rowdot):
    want = _separate(K, case, Gn, nsplit, rowscale, accumulate, rowdot)
    got = _grouped(K, case, Gn, nsplit, rowscale, accumulate, rowdot)
    for g in range(Gn):
        what = (case, Gn, nsplit, rowscale, accumulate, rowdot, g)
        assert not torch.isnan(got[g][0]).any(), what
        assert torch.equal(got[g][0], want[g][0]), (what, float((got[g][0] - want[g][0]).abs().max()))
        if rowdot:
            assert not torch.isnan(got[g][1]).any(), what
            assert torch.equal(got[g][1], want[g][1]), (what, float((got[g][1] - want[g][1]).abs().max()))
    if Gn > 1:        # different groups give different results: a launch that read one group's maps for all of them fails above, and here
        assert not torch.equal(got[0][0], got[1][0])


@pytest.mark.parametrize("case,Gn,nsplit", RUNS)
def test_grouped_launch_is_bit_equal_to_separate_launches(K, case, Gn, nsplit):
    _compare(K, case, Gn, nsplit, False, False, False)
    _compare(K, case, Gn, nsplit, True, True, True)


@pytest.mark.parametrize("rowscale", [False, True])
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("rowdot", [False, True])
def test_grouped_reduce_options(K, rowscale, accumulate, rowdot):
    _compare(K, "one_tap_9x13", 3, 2, rowscale, accumulate, rowdot)
    _compare(K, "row3_co132", 2, 3, rowscale, accumulate, rowdot)


def test_refusals_launch_nothing(K):
    from erd_amd import _lib
    lib = _lib.load()
    case = "one_tap_9x13"
    N, H, W, Cin, Cout, k, pad, _ = CASES[case]
    xs, zs, _, _, _ = _inputs(case, 2)

    def attempt(**fields):
        d = _desc(K, case, xs[0], zs[0], 1)
        for g in range(2):
            d.gx[g], d.gdz[g] = xs[g].data_ptr(), zs[g].data_ptr()
        for name, v in fields.items():
            setattr(d, name, v)
        part = torch.full((_lib.ERD_MAX_GROUPS + 1, Cout, k * k, Cin), NAN, device="cuda")
        d.part = part.data_ptr()
        rc = lib.erd_conv_wgrad(C.byref(d), K._stream())
        torch.cuda.synchronize()
        assert rc != 0 and lib.erd_last_error(), fields
        assert bool(torch.isnan(part).all()), (fields, "a refused call launched")

    attempt(ngroups=0)
    attempt(ngroups=_lib.ERD_MAX_GROUPS + 1)
    attempt(ngroups=2, bf16_multiplicands=1)
    attempt(ngroups=2, limbs3=0)
    d = _desc(K, case, xs[0], zs[0], 1)          # a group without pointers
    d.ngroups = 2
    d.gx[0], d.gdz[0] = xs[0].data_ptr(), zs[0].data_ptr()
    part = torch.full((2, Cout, k * k, Cin), NAN, device="cuda")
    d.part = part.data_ptr()
    assert lib.erd_conv_wgrad(C.byref(d), K._stream()) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(part).all())
    t = _lib.WgradReduceGroups()
    for n in (0, _lib.ERD_MAX_GROUPS + 1):
        t.ngroups = n
        assert lib.erd_wgrad_reduce_grouped(part.data_ptr(), 1, Cout, k * k * Cin, C.byref(t), 0, K._stream()) != 0
    with pytest.raises(RuntimeError):            # the wrapper outside the three-limb mode
        K.set_compute("f32")
        K.conv_wgrad_partials_grouped([[xs[0]], [xs[1]]], [[zs[0]], [zs[1]]], k, 1, pad)


# ---------------------------------------------------------------------------------------------------------------------
# stage level
# ---------------------------------------------------------------------------------------------------------------------
def _stage_params(n_identity, cin=32, mid=8, seed=300):
    """(w, gamma, beta, mean, var) x {conv1, conv2, conv3[, downsample]} per block, every trainable one with a zeroed gradient slot
    marked as a sink (what engine.FlatParams does), so that the weight gradients take the trailing stream"""
    def conv(i, cout, ci, k):
        w = torch.empty(cout, k, k, ci).permute(0, 3, 1, 2)
        w.copy_((G.randn(seed + i, cout, ci, k, k) * (2.0 / (ci * k * k)) ** 0.5))
        ps = [torch.nn.Parameter(w.cuda()), torch.nn.Parameter((1.0 + 0.1 * G.randn(seed + i + 1, cout)).cuda()),
              torch.nn.Parameter((0.1 * G.randn(seed + i + 2, cout)).cuda())]
        for p in ps:
            p.grad = torch.zeros_like(p)
            p._erd_sink = True
        assert ps[0].permute(0, 2, 3, 1).is_contiguous() and ps[0].grad.permute(0, 2, 3, 1).is_contiguous()
        return ps + [(0.1 * G.randn(seed + i + 3, cout)).cuda(), (1.0 + 0.2 * G.randn(seed + i + 4, cout).abs()).cuda()]

    blocks, i = [], 0
    for b in range(1 + n_identity):
        shapes = [(mid, cin, 1), (mid, mid, 3), (cin, mid, 1)] + ([(cin, cin, 1)] if b == 0 else [])
        prm = []
        for cout, ci, k in shapes:
            prm += conv(i, cout, ci, k)
            i += 5
        blocks.append(prm)
    return blocks


def _run_stage(K, Fn, n_identity, grouped, monkeypatch):
    K.set_compute("f32x3")
    monkeypatch.setattr(Fn, "WGRAD_GROUPED", grouped)
    calls = []
    real = K.call

    def recording(name, *args):
        if name == "erd_conv_wgrad":
            d = args[0]._obj
            calls.append((d.ngroups, d.nsplit, d.Cin, d.Cout, d.ntaps, d.seg[0].GH, d.seg[0].GW, d.in_stride))
        return real(name, *args)

    monkeypatch.setattr(K, "call", recording)
    blocks = _stage_params(n_identity)
    x = G.randn(7, 2, 12, 20, 32).abs().cuda().requires_grad_(True)
    dy = G.randn(8, 2, 6, 10, 32).cuda()
    params = [p for b in blocks for p in b]
    y = Fn.ResLayerFn.apply(x, (2,) + (1,) * n_identity, 1e-5, tuple(len(b) for b in blocks), *params)
    y.backward(dy)
    Fn.trail_join()
    torch.cuda.synchronize()
    monkeypatch.setattr(K, "call", real)
    grads = [p.grad.detach().cpu().clone() for p in params if isinstance(p, torch.nn.Parameter)]
    return grads, x.grad.detach().cpu().clone(), calls, list(getattr(Fn.ResLayerFn, "last_group_launches", []))


def _relerr(a, b):      # (tests/reduce_refs.py / test_gpu_kernels.py: largest difference over largest value)
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-300))


@pytest.mark.parametrize("n_identity", [3, 10])
def test_stage_gradients_grouped_against_ungrouped(K, n_identity, monkeypatch):
    """One projection block + identity blocks, channels 32 -> 8 -> 32, input 12x20, stride 2, N = 2.  Every grouped key runs at ONE
    split both ways at these sizes (asserted), so the weight gradients see the same sums in the same order: parameters with two or more
    dimensions are bit-equal.  The 1-d gradients come out of float-atomic column sums of at most n = 2 x 12 x 20
    = 480 terms per channel, whose two runs differ by a reordering of fp32 additions: at most 2 (n - 1) 2^-24 = 5.7e-5 of the sum of
    magnitudes; held to 1e-4, the bound tests/test_gpu_reduce_exact.py holds the one column-sum-derived result to that is not an
    integer sum (d gamma).  10 identity blocks exercise the cap of 8 members per launch and a remainder."""
    from erd_amd import functional as Fn
    g_off, dx_off, calls_off, _ = _run_stage(K, Fn, n_identity, False, monkeypatch)
    g_on, dx_on, calls_on, launches = _run_stage(K, Fn, n_identity, True, monkeypatch)
    assert all(c[0] == 1 for c in calls_off) and len(calls_off) == 4 + 3 * n_identity
    grouped = [c for c in calls_on if c[0] > 1]
    print(f"stage with {n_identity} identity blocks: grouped launches {grouped}; members per launch {launches}")
    # conv3 has 1 + n_identity members, conv1 and conv2 n_identity; cap 8
    want = sorted([8, n_identity - 7, 8, n_identity - 8, 8, n_identity - 8] if n_identity == 10 else [n_identity + 1, n_identity, n_identity])
    assert sorted(c[0] for c in grouped) == want
    assert sorted(launches) == sorted(want + [1, 1, 1])         # conv1, conv2 and the shortcut of the projection block: on their own
    assert sum(c[0] for c in calls_on) == len(calls_off)
    # one split both ways for every shape that is grouped
    shapes = {c[2:] for c in grouped}
    assert all(c[1] == 1 for c in calls_on + calls_off if c[2:] in shapes)
    assert torch.equal(dx_on, dx_off)
    worst = 0.0
    for a, b in zip(g_on, g_off):
        assert not torch.isnan(a).any() and float(b.abs().max()) > 0
        if a.dim() >= 2:
            assert torch.equal(a, b), (a.shape, _relerr(a, b))
        else:
            worst = max(worst, _relerr(a, b))
    print(f"stage with {n_identity} identity blocks: worst 1-d gradient difference grouped against ungrouped {worst:.3e}")
    assert worst < 1e-4


# ---------------------------------------------------------------------------------------------------------------------
# trainer level
# ---------------------------------------------------------------------------------------------------------------------
def test_trainer_steps_with_per_bucket_update(K, monkeypatch):
    """Two ERDTrainer steps on the small model with ERD_BUCKET_UPDATE=1 and 1 MB buckets, grouped against ungrouped: the sync's
    diagnostics stay clean (every parameter reports once, no bucket is late), and the updated parameters agree to 1e-6 per parameter
    in test_gpu_optim_cfg.py's measure (its bound for a trainer's update against a second evaluation of the same step)."""
    from e2e_util import build_erd, f7_state_dicts, make_samples
    from erd_amd import functional as Fn
    from erd_amd.engine import ERDTrainer
    from oracle import erd_oracle as O
    monkeypatch.setenv("ERD_BUCKET_UPDATE", "1")
    K.set_compute("f32x3")
    tsd, ssd = f7_state_dicts()
    batches = []
    for seed in (0, 1):
        imgs, boxes, labels = O.synthetic_batch(2, 123, 153, 40, seed=seed)
        x, metas = O.preprocess(imgs)
        batches.append((x.cuda(), make_samples(boxes, labels, metas)))
    got, issued = [], []
    for grouped in (False, True):
        monkeypatch.setattr(Fn, "WGRAD_GROUPED", grouped)
        Fn.ResLayerFn.last_group_launches = []
        model = build_erd(tsd, ssd)
        tr = ERDTrainer(model, lr=0.02, batch_size_per_gpu=2, auto_scale_lr=False, warmup_iters=0, bucket_mb=1)
        per_step = []
        for b in batches:
            tr.train_step(*b)
            tr.flush()
            torch.cuda.synchronize()
            assert tr.sync.late_buckets == 0 and not tr.sync.missing and not tr.sync.repeats
            per_step.append(tr.sync.issued_in_backward)
        issued.append(per_step)
        assert (max(Fn.ResLayerFn.last_group_launches, default=0) >= 2) == grouped
        got.append({n: p.detach().cpu().clone() for n, p in model.named_parameters() if p.requires_grad})
    print(f"buckets issued in backward per step: ungrouped {issued[0]}, grouped {issued[1]}")
    errs = {n: float((got[1][n] - got[0][n]).abs().max() / (got[0][n].abs().max() + 1e-12)) for n in got[0]}
    worst = max(errs, key=errs.get)
    print(f"updated parameters grouped against ungrouped after two steps: worst {errs[worst]:.3e} ({worst})")
    assert all(torch.isfinite(p).all() for p in got[1].values())
    assert errs[worst] < 1e-6
    assert not torch.equal(got[1]["bbox_head.gfl_cls.weight"], ssd["bbox_head.gfl_cls.weight"])
