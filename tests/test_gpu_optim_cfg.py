"""GPU: the optim_wrapper options in the update -- erd_sgd_momentum_groups, erd_grad_sqnorm + erd_clip_coef,
erd_grad_accumulate, and ERDTrainer / Runner with paramwise_cfg, clip_grad and accumulative_counts.  The reference of every
update is torch.optim.SGD with explicit parameter groups and torch.nn.utils.clip_grad_norm_ on the host."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import golden_inputs as G
from e2e_util import CFG_FIRST, ROOT, build_erd, f7_state_dicts, make_samples
from oracle import erd_oracle as O

CFG_OPTIM = os.path.join(ROOT, "configs", "gfl_increment", "gfl_r50_fpn_1x_coco_first_40_incre_last_40_cats_optim.py")
TABLE_CFG = dict(norm_decay_mult=0., bias_lr_mult=2., bias_decay_mult=0.,
                 custom_keys={'backbone': dict(lr_mult=0.1), 'backbone.layer4': dict(lr_mult=0.5, decay_mult=2.)})
ALIGN = 64


@pytest.fixture(scope="module")
def K():
    from erd_amd import kernels
    assert torch.cuda.is_available()
    return kernels


def relerr(a, b):      # (tests/test_gpu_kernels.py)
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def table_expect(name):
    """(lr multiplier, decay multiplier) of TABLE_CFG for a parameter of the GFL-R50 student, written out by hand (not the
    resolver under test): backbone.layer4 -> (.5, 2), the rest of the backbone -> (.1, 1); elsewhere biases outside
    normalisation layers train at twice the rate, and normalisation parameters and biases are not decayed"""
    if "backbone.layer4" in name:
        return 0.5, 2.0
    if "backbone" in name:
        return 0.1, 1.0
    norm = ".gn." in name
    bias = name.endswith(".bias")
    return (2.0 if bias and not norm else 1.0), (0.0 if norm or bias else 1.0)


def host_update(ps, gs, bufs, lrs, wds, momentum, scale, max_norm=None, coef=None):
    """one torch.optim.SGD step with one parameter group per tensor on the host; gradients are g * scale, clipped by
    clip_grad_norm_(max_norm) or multiplied by a given coefficient.  bufs None: the first step.  -> params, momenta, norm.
    With max_norm the host side runs in fp64: clip_grad_norm_ over fp32 tensors on the CPU returns a norm that is itself 2e-5
    off the fp64 norm of the same gradients (measured on tensors of this model's sizes), twenty times the bound it would be the
    reference for; in fp64 the reference's error is nil and the whole 1e-6 is the device's."""
    dt = torch.float64 if max_norm is not None else torch.float32
    params = [torch.nn.Parameter(p.detach().cpu().to(dt)) for p in ps]
    opt = torch.optim.SGD([dict(params=[p], lr=lr, weight_decay=wd) for p, lr, wd in zip(params, lrs, wds)], lr=1.0, momentum=momentum)
    if bufs is not None:
        for p, b in zip(params, bufs):
            opt.state[p]["momentum_buffer"] = b.detach().cpu().to(dt).clone()
    for p, g in zip(params, gs):
        p.grad = g.detach().cpu().to(dt) * scale
        if coef is not None:
            p.grad.mul_(coef)
    norm = torch.nn.utils.clip_grad_norm_(params, max_norm) if max_norm is not None else None
    opt.step()
    return [p.detach().float() for p in params], [opt.state[p]["momentum_buffer"].float() for p in params], norm


def _layout(sizes):
    offs, total = [], 0
    for n in sizes:
        offs.append(total)
        total += (n + ALIGN - 1) // ALIGN * ALIGN
    return offs, total


SIZES = [1, 4, 68, 256 * 3 * 3 * 256, 64, 80, 256, 2048, 512 * 128, 3, 65, 128, 5, 1024 * 256, 17, 256, 256, 63, 64 * 3 * 3 * 64,
         1, 1, 1, 1, 1, 640, 12, 2048 * 512, 7, 255, 257, 4096, 4100, 9, 80 * 256 * 9, 68, 68, 2, 31, 333, 100000]


@pytest.mark.parametrize("with_coef", [False, True])
def test_sgd_momentum_groups_follows_torch_sgd_with_parameter_groups(K, with_coef):
    """3 steps over a flat buffer of 40 segments of mixed sizes with random multipliers and decays, each parameter starting on a
    multiple of 64 floats as in engine.FlatParams: relative error below 1e-6 (the bound test_gpu_kernels.py::
    test_level_scale_colsum_sgd holds erd_sgd_momentum to).  One launch over the whole buffer and one launch per "bucket" of
    segments give the same bits."""
    offs, total = _layout(SIZES)
    rng = torch.Generator().manual_seed(5)
    lrm = (torch.rand(len(SIZES), generator=rng) * 2).tolist()
    wds = (torch.rand(len(SIZES), generator=rng) * 2e-4).tolist()
    lrm[3], wds[4], wds[0] = 1.0, 0.0, 0.0
    lr, mom, gs, coef = 0.02, 0.9, 0.5, 0.37
    p0 = [G.randn(900 + i, n) for i, n in enumerate(SIZES)]
    flat = torch.zeros(total)
    for o, t in zip(offs, p0):
        flat[o:o + t.numel()] = t
    table = K.SgdSegTable(offs + [total], lrm, wds, "cuda")
    coef_dev = torch.tensor([coef], device="cuda") if with_coef else None
    pa, ba = flat.cuda(), torch.zeros(total, device="cuda")
    pb, bb = flat.cuda(), torch.zeros(total, device="cuda")
    cuts = [0, offs[3], offs[4], offs[20], offs[33], total]          # "buckets": runs of whole segments
    ps, bufs = p0, None
    for it in range(3):
        g = [G.randn(1000 + 50 * it + i, n) for i, n in enumerate(SIZES)]
        gflat = torch.zeros(total)
        for o, t in zip(offs, g):
            gflat[o:o + t.numel()] = t
        gd = gflat.cuda()
        K.sgd_momentum_groups_(pa, gd, ba, 0, table, lr, mom, gs, it == 0, coef_dev)
        for s, e in zip(cuts[:-1], cuts[1:]):
            K.sgd_momentum_groups_(pb[s:e], gd[s:e], bb[s:e], s, table, lr, mom, gs, it == 0, coef_dev)
        ps, bufs, _ = host_update(ps, g, bufs, [lr * m for m in lrm], wds, mom, gs, coef=coef if with_coef else None)
    torch.cuda.synchronize()
    assert torch.equal(pa, pb) and torch.equal(ba, bb)
    ref_p, ref_b = torch.zeros(total), torch.zeros(total)
    for o, t, b in zip(offs, ps, bufs):
        ref_p[o:o + t.numel()] = t
        ref_b[o:o + t.numel()] = b
    ep, eb = relerr(pa.cpu(), ref_p), relerr(ba.cpu(), ref_b)
    worst = max(relerr(pa[o:o + n].cpu(), t) for o, n, t in zip(offs, SIZES, ps))
    print(f"sgd_groups coef={with_coef}: relerr params {ep:.3e} momenta {eb:.3e} worst segment {worst:.3e}")
    assert ep < 1e-6 and eb < 1e-6 and worst < 1e-6
    assert float(pa.cpu()[offs[0] + 1:offs[1]].abs().max()) == 0.0          # the padding stays zero


def test_sgd_momentum_groups_with_unit_multipliers_is_bit_equal_to_sgd_momentum(K):
    offs, total = _layout(SIZES)
    table = K.SgdSegTable(offs + [total], [1.0] * len(SIZES), [1e-4] * len(SIZES), "cuda")
    p = G.randn(77, total)
    pa, ba = p.cuda(), torch.zeros(total, device="cuda")
    pb, bb = p.cuda(), torch.zeros(total, device="cuda")
    for it in range(3):
        g = G.randn(78 + it, total).cuda()
        K.sgd_momentum_(pa, g, ba, 0.02 * (it + 1), 0.9, 1e-4, 0.5, it == 0)
        K.sgd_momentum_groups_(pb, g, bb, 0, table, 0.02 * (it + 1), 0.9, 0.5, it == 0)
    torch.cuda.synchronize()
    assert torch.equal(pa, pb) and torch.equal(ba, bb)
    from erd_amd._lib import ErdHipError
    with pytest.raises(ErdHipError, match="multiple of 4"):          # a float4 must not straddle two segments
        K.SgdSegTable([0, 6, 64], [1.0, 1.0], [0.0, 0.0], "cuda")


@pytest.mark.parametrize("n", [4, 4 * 257, 4 * (4096 * 256 + 257)])
def test_sgd_momentum_at_the_tile_edges(K, n):
    """the shapes at which a kernel that walks tiles of 256 float4 can go wrong: one lane; one full tile plus one lane (the guard
    of the ragged tile); one full sweep of the 4096-block grid cap, then a second sweep with a ragged last tile.  3 steps of
    sgd_momentum_ stay within 1e-6 of the host update (the bound test_gpu_kernels.py::test_level_scale_colsum_sgd holds this
    entry to) and are bit-equal to sgd_momentum_groups_ with a unit table of 64-aligned segments of mixed sizes."""
    offs = [0]
    while offs[-1] < n:
        offs.append(offs[-1] + ALIGN * (1, 3, 16, 1, 33, 4097, 2)[(len(offs) - 1) % 7])
    lr, mom, wd, gs = 0.02, 0.9, 1e-4, 0.5
    table = K.SgdSegTable(offs, [1.0] * (len(offs) - 1), [wd] * (len(offs) - 1), "cuda")
    p = G.randn(87, n)
    pa, ba = p.cuda(), torch.zeros(n, device="cuda")
    pb, bb = p.cuda(), torch.zeros(n, device="cuda")
    ps, bufs = [p], None
    for it in range(3):
        g = G.randn(88 + it, n)
        gd = g.cuda()
        K.sgd_momentum_(pa, gd, ba, lr * (it + 1), mom, wd, gs, it == 0)
        K.sgd_momentum_groups_(pb, gd, bb, 0, table, lr * (it + 1), mom, gs, it == 0)
        ps, bufs, _ = host_update(ps, [g], bufs, [lr * (it + 1)], [wd], mom, gs)
    torch.cuda.synchronize()
    ep, eb = relerr(pa.cpu(), ps[0]), relerr(ba.cpu(), bufs[0])
    print(f"sgd n={n}: relerr params {ep:.3e} momenta {eb:.3e}")
    assert ep < 1e-6 and eb < 1e-6
    assert torch.equal(pa, pb) and torch.equal(ba, bb)


@pytest.mark.parametrize("n", [4, 1000004, 32 << 20])
@pytest.mark.parametrize("nb", [1, 7])
def test_grad_sqnorm_and_clip_coef_follow_the_fp64_norm(K, n, nb):
    """fp64 accumulation of exact fp32 squares leaves the final rounding to fp32 (6e-8); 1e-6 is the margin.  Two runs give the
    same bits; the coefficient is exactly 1 when max_norm is above the norm."""
    from erd_amd._lib import ERD_SQNORM_PARTS as P
    gen = torch.Generator(device="cuda").manual_seed(n + nb)
    g = torch.randn(n, device="cuda", generator=gen) * 3.0
    ref = float(g.cpu().double().norm())
    cuts = [min(n, (n // 4 * b // nb) * 4) for b in range(nb)] + [n]
    gs = 0.25                                     # 1 / (world * window): the norm is that of the MEAN gradient

    def run(max_norm):
        ws = torch.full((nb * P,), float("nan"), dtype=torch.float64, device="cuda")
        out = torch.empty(2, device="cuda")
        for b in range(nb):
            K.grad_sqnorm_into(g[cuts[b]:cuts[b + 1]], ws[b * P:(b + 1) * P])
        K.clip_coef_(ws, gs, max_norm, out)
        torch.cuda.synchronize()
        return ws.cpu(), out.cpu()

    ws1, out1 = run(2.0 * gs * ref)
    ws2, out2 = run(2.0 * gs * ref)
    assert torch.equal(ws1, ws2) and torch.equal(out1, out2)
    err = abs(float(out1[0]) - gs * ref) / (gs * ref)
    print(f"grad_sqnorm n={n} buckets={nb}: total_norm {float(out1[0]):.9g} host {gs * ref:.9g} relerr {err:.3e}")
    assert err < 1e-6
    assert float(out1[1]) == 1.0
    _, out3 = run(0.5 * gs * ref)
    want = 0.5 * gs * ref / (gs * ref + 1e-6)
    assert abs(float(out3[1]) - want) / want < 1e-6 and float(out3[0]) == float(out1[0])


def test_grad_accumulate_is_the_plain_fp32_sum(K):
    n = 1000004
    a, b, c = G.randn(1, n), G.randn(2, n), G.randn(3, n)
    acc = torch.full((n,), float("nan"), device="cuda")
    K.grad_accumulate_(acc, a.cuda(), True)
    K.grad_accumulate_(acc, b.cuda(), False)
    K.grad_accumulate_(acc[4:], c.cuda()[4:], False)
    assert torch.equal(acc.cpu()[4:], (a + b + c)[4:]) and torch.equal(acc.cpu()[:4], (a + b)[:4])


# ---------------------------------------------------------------------------------------------------------------------
# trainer
# ---------------------------------------------------------------------------------------------------------------------
def _batches(seeds=(0, 1)):
    out = []
    for seed in seeds:
        imgs, boxes, labels = O.synthetic_batch(2, 123, 153, 40, seed=seed)
        x, metas = O.preprocess(imgs)
        out.append((x.cuda(), make_samples(boxes, labels, metas)))
    return out


def _slices(tr, t):
    return [t[o:o + p.numel()] for o, p in zip(tr.flat.offsets, tr.flat.params)]


def _check_update(tr, d0, m0, first, g, lr, scale, max_norm, what):
    """flat.data / flat.momentum of `tr` against the host update of (d0, m0, g) under TABLE_CFG: below 1e-6 over the whole buffers
    (test_gpu_kernels.py::relerr, the measure test_level_scale_colsum_sgd uses) and, stricter, per parameter"""
    mult = [table_expect(n) for n in tr.flat.names]
    ps, bufs, norm = host_update(_slices(tr, d0), _slices(tr, g), None if first else _slices(tr, m0),
                                 [lr * a for a, _ in mult], [tr.weight_decay * b for _, b in mult], tr.momentum, scale, max_norm)
    ref_p, ref_b = tr.flat.data.cpu().clone(), tr.flat.momentum.cpu().clone()
    for o, t, b in zip(tr.flat.offsets, ps, bufs):
        ref_p[o:o + t.numel()] = t
        ref_b[o:o + t.numel()] = b
    wp, wb = relerr(tr.flat.data.cpu(), ref_p), relerr(tr.flat.momentum.cpu(), ref_b)
    ep = [relerr(a.cpu(), b) for a, b in zip(_slices(tr, tr.flat.data), ps)]
    eb = [relerr(a.cpu(), b) for a, b in zip(_slices(tr, tr.flat.momentum), bufs)]
    i, j = ep.index(max(ep)), eb.index(max(eb))
    print(f"{what}: whole buffers weights {wp:.3e} momenta {wb:.3e}; worst parameter weights {ep[i]:.3e} ({tr.flat.names[i]}) "
          f"momenta {eb[j]:.3e} ({tr.flat.names[j]})")
    assert wp < 1e-6 and wb < 1e-6, what
    assert max(ep) < 1e-6 and max(eb) < 1e-6, what
    return norm


@pytest.mark.parametrize("bucket_update", ["1", "0"])
def test_trainer_update_with_paramwise_cfg_and_active_clipping(bucket_update, monkeypatch):
    """one train_step + flush(): the update does not write flat.grad, so it still holds the step's summed gradient; the new
    weights and momenta equal the host update of (old weights, old momenta, that gradient) with the table's parameter groups
    and clip_grad_norm_ at half the gradient's own norm (clipping active) to 1e-6 per parameter; the logged grad_norm equals
    the host norm to 1e-6.  A first trainer with an unreachable max_norm measures that norm (and is checked the same way)."""
    from erd_amd.engine import ERDTrainer
    monkeypatch.setenv("ERD_BUCKET_UPDATE", bucket_update)
    tsd, ssd = f7_state_dicts()
    batches = _batches()
    norm0 = None
    for rnd in range(2):
        model = build_erd(tsd, ssd)
        max_norm = 1e9 if rnd == 0 else 0.5 * norm0
        tr = ERDTrainer(model, lr=0.02, batch_size_per_gpu=2, auto_scale_lr=False, warmup_iters=0, bucket_mb=1,
                        paramwise_cfg=TABLE_CFG, clip_grad=dict(max_norm=max_norm, norm_type=2))
        assert tr.bucket_update == (bucket_update == "1") and len(tr.flat.buckets) >= 4
        for step in range(2):
            d0, m0, first = tr.flat.data.clone(), tr.flat.momentum.clone(), tr._first
            log = tr.train_step(*batches[step])
            tr.flush()
            torch.cuda.synchronize()
            if bucket_update == "1":
                assert tr.sync.late_buckets == 0
            g = tr.flat.grad.clone()
            host_norm = float(g.cpu().double().norm())
            got = float(log["grad_norm"])
            print(f"bucket_update={bucket_update} max_norm={max_norm:.6g} step {step}: grad_norm {got:.9g} host {host_norm:.9g}")
            assert abs(got - host_norm) / host_norm < 1e-6
            assert (host_norm > max_norm) == (rnd == 1)            # clipping is active in the second round only
            _check_update(tr, d0, m0, first, g, tr.last_lr, 1.0, max_norm, f"bucket_update={bucket_update} round {rnd} step {step}")
            if norm0 is None:
                norm0 = host_norm
        assert not tr._first


@pytest.mark.parametrize("bucket_update", ["1", "0"])
def test_trainer_accumulates_two_micro_steps_per_update(bucket_update, monkeypatch):
    from erd_amd.engine import ERDTrainer
    monkeypatch.setenv("ERD_BUCKET_UPDATE", bucket_update)
    tsd, ssd = f7_state_dicts()
    batches = _batches((0, 1, 2))
    model = build_erd(tsd, ssd)
    tr = ERDTrainer(model, lr=0.02, batch_size_per_gpu=2, auto_scale_lr=False, warmup_iters=0, bucket_mb=1,
                    paramwise_cfg=TABLE_CFG, accumulative_counts=2)
    with pytest.raises(NotImplementedError):
        ERDTrainer(model, step_graph=True, accumulative_counts=2)

    def derived():
        # prepared weights that vouch for the parameters (ParamPrep.lookup: a recipe registered since the last preparation holds
        # no data yet)
        outs = {k: r.out.clone() for k, r in tr.prep.recipes.items() if tr.prep.lookup(k) is r} if tr.prep is not None else {}
        if tr.prefold is not None and tr.prefold.bns:
            outs["bn folds"] = tr.prefold.buf.clone()
        return outs

    # first call: no update -- weights and momenta are bit-equal to before, the accumulator holds the gradient
    d0, m0 = tr.flat.data.clone(), tr.flat.momentum.clone()
    tr.train_step(*batches[0])
    tr.flush(close_window=False)
    torch.cuda.synchronize()
    g1 = tr.flat.grad.clone()
    assert torch.equal(tr.flat.data, d0) and torch.equal(tr.flat.momentum, m0) and tr._first
    assert torch.equal(tr._acc, g1) and float(g1.abs().max()) > 0
    # second call: the window closes -- accumulator = fp32 sum in order, update with scale 1/2
    tr.train_step(*batches[1])
    tr.flush(close_window=False)
    torch.cuda.synchronize()
    g2 = tr.flat.grad.clone()
    assert torch.equal(tr._acc.cpu(), g1.cpu() + g2.cpu())
    _check_update(tr, d0, m0, True, tr._acc, tr.last_lr, 0.5, None, f"bucket_update={bucket_update} window of 2")
    assert not tr._first
    # third call: no update again -- weights, momenta, BN folds and prepared weights are bit-equal to before
    d1, m1, x1 = tr.flat.data.clone(), tr.flat.momentum.clone(), derived()
    assert len(x1) > 1
    tr.train_step(*batches[2])
    tr.flush(close_window=False)
    torch.cuda.synchronize()
    g3 = tr.flat.grad.clone()
    assert torch.equal(tr.flat.data, d1) and torch.equal(tr.flat.momentum, m1)
    x2 = derived()          # (later passes register further prepared buffers: those of before must all be there, unchanged)
    assert not [k for k in x1 if k not in x2 or not torch.equal(x1[k], x2[k])]
    assert torch.equal(tr._acc, g3)
    # ... and flush() closes the partial window: one micro-step, scale 1
    tr.flush()
    torch.cuda.synchronize()
    _check_update(tr, d1, m1, False, g3, tr.last_lr, 1.0, None, f"bucket_update={bucket_update} window of 1")
    state = tr.optimizer_state_dict()
    assert len(state["param_groups"]) == len(list(model.parameters()))


def test_unit_custom_key_leaves_the_weights_of_a_plain_trainer(monkeypatch):
    """custom_keys={'backbone': dict(lr_mult=1.0)} and nothing else: after ONE step the >= 2-D parameters are bit-equal to a plain
    trainer's from the same weights (1-D gradients carry float-atomic column sums and differ in their last bits between any two
    runs, DESIGN.md section 5: the 1e-6 tests cover them)"""
    from erd_amd.engine import ERDTrainer
    tsd, ssd = f7_state_dicts()
    batch = _batches((0,))[0]
    got = []
    for pw in (None, dict(custom_keys={'backbone': dict(lr_mult=1.0)})):
        model = build_erd(tsd, ssd)
        tr = ERDTrainer(model, lr=0.02, batch_size_per_gpu=2, auto_scale_lr=False, warmup_iters=0, paramwise_cfg=pw)
        assert (tr._table is not None) == (pw is not None)
        tr.train_step(*batch)
        tr.flush()
        torch.cuda.synchronize()
        got.append({n: p.detach().cpu().clone() for n, p in model.named_parameters() if p.requires_grad})
    names = [n for n, p in got[0].items() if p.dim() >= 2]
    assert len(names) > 50
    assert not [n for n in names if not torch.equal(got[0][n], got[1][n])]
    assert not torch.equal(got[0]["bbox_head.gfl_cls.weight"], ssd["bbox_head.gfl_cls.weight"])


# the update census: which entries of the library one optimisation step calls for its update, with which ranges, in which order
UPDATES = ("erd_sgd_momentum", "erd_sgd_momentum_groups", "erd_adam_groups")
DERIVED = ("erd_bn_fold_batch", "erd_weight_prep_batch")       # BnPrefold.run / run_group, ParamPrep.run / run_group
CENSUS = UPDATES + DERIVED + ("erd_grad_sqnorm", "erd_clip_coef", "erd_grad_accumulate")
CENSUS_CASES = {                # trainer options, ERD_BUCKET_UPDATE, train_step calls
    "plain-whole": (dict(), "0", 3),
    "plain-buckets": (dict(), "1", 3),
    "table-whole": (dict(paramwise_cfg=TABLE_CFG), "0", 3),
    "table-buckets": (dict(paramwise_cfg=TABLE_CFG), "1", 3),
    "table-clip-buckets": (dict(paramwise_cfg=TABLE_CFG, clip_grad=dict(max_norm=35, norm_type=2)), "1", 3),
    "table-clip-whole": (dict(paramwise_cfg=TABLE_CFG, clip_grad=dict(max_norm=35, norm_type=2)), "0", 3),
    "accumulate-whole": (dict(accumulative_counts=2), "0", 5),
    "accumulate-buckets": (dict(accumulative_counts=2), "1", 5),
    "adamw-whole": (dict(optimizer=dict(type='AdamW', lr=1e-3)), "0", 3),
    "adamw-buckets": (dict(optimizer=dict(type='AdamW', lr=1e-3)), "1", 3),
}


@pytest.fixture(scope="module")
def census_inputs():
    return f7_state_dicts(), _batches((0, 1, 2))


@pytest.mark.parametrize("case", sorted(CENSUS_CASES))
def test_update_census(K, case, census_inputs, monkeypatch):
    """every call the trainer makes into the library goes through kernels.call: recorded for `steps` train_step +
    flush(close_window=False) and a closing flush(), the update-path entries of each step are exactly
      whole buffers: [erd_grad_accumulate] then, when the step closes its window, [erd_grad_sqnorm, erd_clip_coef,] ONE update launch
                     over flat.total;
      per bucket:    for each bucket in order [erd_grad_accumulate,] and, closing, the update launch over the bucket -- with clipping
                     erd_grad_sqnorm per bucket instead, then one erd_clip_coef, then the update launches of all buckets in order;
    each update launch is followed at once by the derived state of ITS range (the BN folds of that bucket / of all, then at most two
    weight preparation launches of that bucket / of all) and a step that closes no window issues none."""
    from erd_amd.engine import ERDTrainer
    opts, bucket_update, steps = CENSUS_CASES[case]
    (tsd, ssd), batches = census_inputs
    monkeypatch.setenv("ERD_BUCKET_UPDATE", bucket_update)
    log, cur = [], {}
    real = K.call
    ptr = lambda a: getattr(a, "value", a)

    def owner(name, args):
        """the range a derived-state launch works on, from the device table it is given: a bucket, or None for everything"""
        tr, t = cur["tr"], ptr(args[0])
        if name == "erd_bn_fold_batch":
            if t == tr.prefold.table.data_ptr():
                return None
            return next(g for g, ent in tr.prefold.gtables.items() if ent[0].data_ptr() == t)
        if any(tab[0].data_ptr() == t for tab in (tr.prep._tables or [])):
            return None
        return next(g for g, tabs in tr.prep._gtables.items() if any(tab[0].data_ptr() == t for tab in tabs))

    def recorder(name, *args):
        if name in CENSUS and "tr" in cur:
            log.append((name, args, owner(name, args) if name in DERIVED else None))
        return real(name, *args)

    monkeypatch.setattr(K, "call", recorder)
    model = build_erd(tsd, ssd)
    tr = ERDTrainer(model, lr=0.02, batch_size_per_gpu=2, auto_scale_lr=False, warmup_iters=0, bucket_mb=1, **opts)
    cur["tr"] = tr
    buckets = [(s, e) for s, e, _ in tr.flat.buckets]
    nb, total = len(buckets), tr.flat.total
    assert tr.bucket_update == (bucket_update == "1") and nb >= 4
    accum, clip, adam = opts.get("accumulative_counts", 1), "clip_grad" in opts, "optimizer" in opts
    assert not adam or tuple(tr.opt["betas"]) == (0.9, 0.999)
    kind = "erd_adam_groups" if adam else "erd_sgd_momentum_groups" if "paramwise_cfg" in opts else "erd_sgd_momentum"
    ranges = list(enumerate(buckets)) if tr.bucket_update else [(None, (0, total))]
    folded = lambda b: bool(tr.prefold.bns) if b is None else b in tr.prefold.gtables

    def token(name, args):
        """(entry, base or None, n, what else the table of the issue pins)"""
        if name == "erd_sgd_momentum":
            return (name, None, args[3])
        if name == "erd_sgd_momentum_groups":
            return (name, args[3], args[4])
        if name == "erd_adam_groups":
            return (name, args[4], args[5], args[16], args[17])
        if name == "erd_grad_accumulate":
            return (name, args[2], args[3])
        if name == "erd_grad_sqnorm":
            return (name, args[1])
        return (name,)

    def update_token(s, e, t):
        if kind == "erd_sgd_momentum":
            return (kind, None, e - s)
        if kind == "erd_sgd_momentum_groups":
            return (kind, s, e - s)
        # `step` does not cross the C ABI: the entry takes the two bias corrections of update t, 1 / (1 - beta1^t) and
        # 1 / sqrt(1 - beta2^t) in double, written out here (torch's defaults: betas 0.9, 0.999)
        return (kind, s, e - s, 1.0 / (1.0 - 0.9 ** t), 1.0 / (1.0 - 0.999 ** t) ** 0.5)

    def check(entries, micro_first, close, t, ranges, what):
        want = []
        for b, (s, e) in ranges:
            if accum > 1 and micro_first is not None:
                want.append(("erd_grad_accumulate", e - s, 1 if micro_first else 0))
            if close and clip:
                want.append(("erd_grad_sqnorm", e - s))
            elif close:
                want.append(update_token(s, e, t))
        if close and clip:
            want.append(("erd_clip_coef",))
            want += [update_token(s, e, t) for _, (s, e) in ranges]
        got = [token(n, a) for n, a, _ in entries if n not in DERIVED]
        assert got == want, (what, got, want)
        # the derived state: right behind the update launch of its range, the folds first
        runs, run = [], None
        for n, _, o in entries:
            if n in UPDATES:
                run = []
                runs.append(run)
            elif n in DERIVED:
                assert run is not None, (what, "derived state without an update launch right in front of it", n)
                run.append((n, o))
            else:
                run = None
        assert len(runs) == (len(ranges) if close else 0), what
        for (b, _), run in zip(ranges, runs):
            assert [o for _, o in run] == [b] * len(run), (what, b, run)
            names = [n for n, _ in run]
            nfold = names.count("erd_bn_fold_batch")
            assert names == ["erd_bn_fold_batch"] * nfold + ["erd_weight_prep_batch"] * (len(names) - nfold), (what, b, names)
            assert nfold == (1 if folded(b) else 0) and len(names) - nfold <= 2, (what, b, names)
            if t >= 2:                   # (from the second update on every range has registered its prepared weights)
                assert len(names) - nfold >= 1, (what, b, names)

    t = window = 0
    for it in range(steps):
        del log[:]
        tr.train_step(*batches[it % len(batches)])
        tr.flush(close_window=False)
        micro_first, window = window == 0, window + 1
        close = (it + 1) % accum == 0
        if close:
            t, window = t + 1, 0
        check(list(log), micro_first, close, t, ranges, f"{case} step {it + 1}")
    del log[:]
    tr.flush()
    if window:                           # the partial window: ONE update over the whole buffers, nothing left to accumulate
        t += 1
    check(list(log), None, window > 0, t, [(None, (0, total))], f"{case} closing flush")
    torch.cuda.synchronize()
    assert tr._t == t and not tr._first
    assert (tr._acc is not None) == (accum > 1) and (tr.exp_avg_sq is not None) == adam


def test_runner_example_config_logs_grad_norm_checkpoints_groups_and_resumes(tmp_path):
    from erd_amd import Config
    from erd_amd.runner import Runner, SyntheticDetData
    teacher = tmp_path / "teacher.pth"
    torch.save(dict(state_dict=O.procedural_state_dict(40, seed=0)), teacher)

    def cfg(**over):
        c = Config.fromfile(CFG_OPTIM)
        c.work_dir = str(tmp_path / "w")
        c.merge_from_dict({"train_dataloader.batch_size": 2, "train_cfg.max_epochs": 1, "model.backbone.init_cfg": None,
                           "default_hooks.logger.interval": 1, "model.ori_setting.ori_checkpoint_file": str(teacher),
                           "model.ori_setting.ori_config_file": CFG_FIRST, **over})
        return c

    lines = []
    torch.manual_seed(3)
    r = Runner.from_cfg(cfg(), data=SyntheticDetData(2, 40, 4, image_hw=(123, 153), seed=1), log=lines.append)
    tr = r.trainer
    assert tr.accum == 4 and tr.clip == dict(max_norm=35.0, error_if_nonfinite=False) and tr.resolved is not None
    d0 = tr.flat.data.clone()
    hist = r.train()
    assert len(hist) == 4 and tr.iter == 4
    assert ["grad_norm" in h for h in hist] == [False, False, False, True]        # one update per 4 micro-steps
    assert hist[3]["grad_norm"] > 0 and "grad_norm: " in [l for l in lines if "Epoch(train) [1][4/4]" in l][0]
    assert not any("grad_norm" in l for l in lines if "Epoch(train) [1][3/4]" in l)
    assert not torch.equal(tr.flat.data, d0)
    ck = torch.load(tmp_path / "w" / "epoch_1.pth", map_location="cpu", weights_only=False)
    names = [n for n, _ in r.model.named_parameters()]
    groups = ck["optimizer"]["param_groups"]
    assert len(groups) == len(names) and ck["meta"]["iter"] == 4
    base_lr = 0.01 * 2 / 16                                        # auto_scale_lr: one GPU x 2 images against 16
    factor = r.schedule.iter_factor(3) * r.schedule.epoch_factor(0)   # of the iteration that triggered the update
    assert 0 < factor < 0.01
    for name, (lr, wd) in {"backbone.layer4.0.conv1.weight": (0.5, 2e-4), "backbone.layer2.0.bn1.weight": (0.1, 1e-4),
                           "bbox_head.cls_convs.0.gn.weight": (1.0, 0.0), "bbox_head.cls_convs.0.gn.bias": (1.0, 0.0),
                           "bbox_head.gfl_cls.bias": (2.0, 0.0), "neck.lateral_convs.0.conv.bias": (2.0, 0.0),
                           "bbox_head.gfl_cls.weight": (1.0, 1e-4)}.items():
        g = groups[names.index(name)]
        assert g["params"] == [names.index(name)]
        assert g["lr"] == pytest.approx(base_lr * lr * factor, rel=1e-9) and g["initial_lr"] == pytest.approx(base_lr * lr, rel=1e-9)
        assert g["weight_decay"] == pytest.approx(wd, rel=1e-9, abs=0)
    assert len(ck["optimizer"]["state"]) == len(tr.flat.params)
    # resume: bit-equal momenta, the same groups, the same iteration count.  (`lr` is the schedule's value at the last step TAKEN:
    # the resumed trainer has taken none yet, so it is left out; not "the same next weights" either -- two runs of one step differ
    # in the last bits of their 1-D gradients)
    r2 = Runner.from_cfg(cfg(resume=True), data=SyntheticDetData(2, 40, 4, image_hw=(123, 153), seed=1), log=lambda *_: None)
    assert r2.epoch == 1 and r2.trainer.iter == 4
    sd2 = r2.trainer.optimizer_state_dict()
    assert sd2["state"].keys() == ck["optimizer"]["state"].keys()
    for i, st in ck["optimizer"]["state"].items():
        assert torch.equal(sd2["state"][i]["momentum_buffer"], st["momentum_buffer"]), i
    strip = lambda gs: [{k: v for k, v in g.items() if k != "lr"} for g in gs]
    assert strip(sd2["param_groups"]) == strip(groups)
    for k, v in ck["state_dict"].items():
        assert torch.equal(r2.model.state_dict()[k].cpu(), v), k
