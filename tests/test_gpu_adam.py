"""GPU: AdamW / Adam in the update -- erd_adam_groups against torch.optim.AdamW / torch.optim.Adam, and ERDTrainer / Runner with
`optimizer=dict(type='AdamW', ...)`.  The reference of every update is torch's own optimizer on the host, evaluated in fp64 from
the same fp32 inputs (torch's fp32 host AdamW itself lies 1.9e-7 / 1.0e-7 / 1.9e-7 from that for weights / exp_avg / exp_avg_sq
on the kernel test's inputs, Adam at eps 1e-3 2.8e-7 / 1.1e-7 / 2.1e-7); the measure is `relerr` (max abs difference over max
abs reference) and the bound the 1e-6 erd_sgd_momentum is held to.  Coupled Adam at eps 1e-8 is left out: there g + wd * p
cancels and the fp32 host reference itself sits at 1.2e-5."""
import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import golden_inputs as G
from e2e_util import CFG_FIRST, CFG_INCRE, ROOT, build_erd, f7_state_dicts, make_samples
from oracle import erd_oracle as O

CFG_ADAMW = os.path.join(ROOT, "configs", "gfl_increment", "gfl_r50_fpn_1x_coco_first_40_incre_last_40_cats_adamw.py")
TABLE_CFG = dict(norm_decay_mult=0., bias_lr_mult=2., bias_decay_mult=0.,
                 custom_keys={'backbone': dict(lr_mult=0.1), 'backbone.layer4': dict(lr_mult=0.5, decay_mult=2.)})
ALIGN = 64
BETAS = (0.9, 0.999)
# the 40-segment layout of tests/test_gpu_optim_cfg.py: ragged tails and padding in every position of a 256-float4 tile
SIZES = [1, 4, 68, 256 * 3 * 3 * 256, 64, 80, 256, 2048, 512 * 128, 3, 65, 128, 5, 1024 * 256, 17, 256, 256, 63, 64 * 3 * 3 * 64,
         1, 1, 1, 1, 1, 640, 12, 2048 * 512, 7, 255, 257, 4096, 4100, 9, 80 * 256 * 9, 68, 68, 2, 31, 333, 100000]
LR, GS, COEF, STEPS = 0.1, 0.5, 0.37, 3


@pytest.fixture(scope="module")
def K():
    from erd_amd import kernels
    assert torch.cuda.is_available()
    return kernels


def relerr(a, b):      # (tests/test_gpu_kernels.py)
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def table_expect(name):
    """(lr multiplier, decay multiplier) of TABLE_CFG for a parameter of the GFL-R50 student, written out by hand (as in
    tests/test_gpu_optim_cfg.py, not the resolver)"""
    if "backbone.layer4" in name:
        return 0.5, 2.0
    if "backbone" in name:
        return 0.1, 1.0
    norm = ".gn." in name
    bias = name.endswith(".bias")
    return (2.0 if bias and not norm else 1.0), (0.0 if norm or bias else 1.0)


def host_adam(kind, ps, gs, ms, vs, t, lrs, wds, betas, eps, scale, max_norm=None, coef=None):
    """update number t (1-based) of torch.optim.AdamW / Adam in fp64 on the host, one parameter group per tensor: gradients are
    g * scale, clipped by clip_grad_norm_(max_norm) or multiplied by a given coefficient; ms / vs None: no state yet (t == 1).
    -> fp64 params, exp_avg, exp_avg_sq, norm"""
    params = [torch.nn.Parameter(p.detach().cpu().double()) for p in ps]
    cls = dict(AdamW=torch.optim.AdamW, Adam=torch.optim.Adam)[kind]
    opt = cls([dict(params=[p], lr=lr, weight_decay=wd) for p, lr, wd in zip(params, lrs, wds)], lr=1.0, betas=betas, eps=eps,
              foreach=False)
    if t > 1:
        for p, m, v in zip(params, ms, vs):
            opt.state[p] = dict(step=torch.tensor(float(t - 1)), exp_avg=m.detach().cpu().double().clone(),
                                exp_avg_sq=v.detach().cpu().double().clone())
    for p, g in zip(params, gs):
        p.grad = g.detach().cpu().double() * scale
        if coef is not None:
            p.grad.mul_(coef)
    norm = torch.nn.utils.clip_grad_norm_(params, max_norm) if max_norm is not None else None
    opt.step()
    assert all(float(opt.state[p]["step"]) == t for p in params)
    return ([p.detach() for p in params], [opt.state[p]["exp_avg"] for p in params], [opt.state[p]["exp_avg_sq"] for p in params],
            norm)


def _layout(sizes):
    offs, total = [], 0
    for n in sizes:
        offs.append(total)
        total += (n + ALIGN - 1) // ALIGN * ALIGN
    return offs, total


def _flatten(offs, total, ts, dtype=torch.float32):
    flat = torch.zeros(total, dtype=dtype)
    for o, t in zip(offs, ts):
        flat[o:o + t.numel()] = t
    return flat


@functools.lru_cache(maxsize=None)
def _inputs():
    """weights, per-step gradients, per-segment lr multipliers in [0, 2) and decays in [0, 0.1) with a few exact zeros and ones.
    The generators and the multipliers' seed are those of tests/test_gpu_optim_cfg.py; the seeds of weights and gradients start
    at 901 and 1016 instead of 900 and 1000, for the sake of the PER-SEGMENT measure.  At lr 0.1 a weight moves by up to 0.6 in
    three updates, and with 900 + i the ONE weight of segment 21 goes 0.149 -> 0.0038.  Every update stores a weight rounded to
    fp32 (2^-24 of its size THEN), so against a result 39 times smaller storage alone is worth up to 39 * 3 * 6e-8 = 7e-6:
    torch's own fp32 AdamW is 4.6e-6 off the fp64 run on that segment, whatever the arithmetic in between.  With 1000 + 50 * it
    + i the one-element exp_avg of segment 19 cancels the same way (0.0156 -> 0.0005 in the Adam case).  `relerr` over a segment
    tests the kernel only where the segment does not cancel like that, so _reference measures it on the fp64 run -- the largest
    |value| a segment holds after any update over the largest it ends with, for weights and exp_avg (exp_avg_sq sums squares
    and cannot cancel) -- and the test requires at most 2: a storage floor of 2 * 3 * 6e-8 = 3.6e-7 under the bound.  These are
    the first seed bases (gradients from 1000, then weights from 900) that meet it in all six cases."""
    rng = torch.Generator().manual_seed(5)
    lrm = (torch.rand(len(SIZES), generator=rng) * 2).tolist()
    wds = (torch.rand(len(SIZES), generator=rng) * 0.1).tolist()
    lrm[3], lrm[9], lrm[26], wds[4], wds[0], wds[13] = 1.0, 0.0, 1.0, 0.0, 0.0, 0.0
    p0 = [G.randn(901 + i, n) for i, n in enumerate(SIZES)]
    grads = [[G.randn(1016 + 50 * it + i, n) for i, n in enumerate(SIZES)] for it in range(STEPS)]
    return lrm, wds, p0, grads


@functools.lru_cache(maxsize=None)
def _reference(kind, eps, with_coef):
    """STEPS host updates in fp64 -> flat fp64 (weights, exp_avg, exp_avg_sq) and the worst cancellation of a segment (_inputs);
    computed once per case and shared (read only)"""
    lrm, wds, p0, grads = _inputs()
    offs, total = _layout(SIZES)
    peak = lambda ts: [float(t.abs().max()) for t in ts]
    ps, ms, vs = p0, None, None
    top_p, top_m = peak(ps), [0.0] * len(SIZES)
    for it in range(STEPS):
        ps, ms, vs, _ = host_adam(kind, ps, grads[it], ms, vs, it + 1, [LR * m for m in lrm], wds, BETAS, eps, GS,
                                  coef=COEF if with_coef else None)
        top_p, top_m = [max(a, b) for a, b in zip(top_p, peak(ps))], [max(a, b) for a, b in zip(top_m, peak(ms))]
    cancel = max(a / b for a, b in zip(top_p + top_m, peak(ps) + peak(ms)))
    return tuple(_flatten(offs, total, x, torch.float64) for x in (ps, ms, vs)) + (cancel,)


def _device_run(K, kind, eps, with_coef):
    """STEPS updates on the device twice: one launch over the buffer (a), one launch per run of whole segments (b)"""
    lrm, wds, p0, grads = _inputs()
    offs, total = _layout(SIZES)
    table = K.SgdSegTable(offs + [total], lrm, wds, "cuda")
    coef_dev = torch.tensor([COEF], device="cuda") if with_coef else None
    flat = _flatten(offs, total, p0)
    a = [flat.cuda(), torch.zeros(total, device="cuda"), torch.zeros(total, device="cuda")]
    b = [flat.cuda(), torch.zeros(total, device="cuda"), torch.zeros(total, device="cuda")]
    cuts = [0, offs[3], offs[4], offs[20], offs[33], total]          # "buckets": runs of whole segments, base != 0
    for it in range(STEPS):
        gd = _flatten(offs, total, grads[it]).cuda()
        K.adam_groups_(a[0], gd, a[1], a[2], 0, table, LR, 0.0, BETAS, eps, it + 1, GS, kind == "AdamW", coef_dev)
        for s, e in zip(cuts[:-1], cuts[1:]):
            K.adam_groups_(b[0][s:e], gd[s:e], b[1][s:e], b[2][s:e], s, table, LR, 0.0, BETAS, eps, it + 1, GS, kind == "AdamW",
                           coef_dev)
    torch.cuda.synchronize()
    return [x.cpu() for x in a], [x.cpu() for x in b]


@pytest.mark.parametrize("with_coef", [False, True])
@pytest.mark.parametrize("kind,eps", [("AdamW", 1e-8), ("AdamW", 1e-3), ("Adam", 1e-3)])
def test_adam_groups_follows_torch_adamw_and_adam_in_fp64(K, kind, eps, with_coef):
    """3 updates (bias corrections of t = 1..3) over 40 segments with their own learning rates and decays, lr 0.1, grad_scale
    0.5, clip coefficient 0.37 on and off: weights, exp_avg and exp_avg_sq below 1e-6 of the fp64 host optimizer over the whole
    buffers and per segment; one launch and one launch per run of segments give equal bits; the padding stays zero.  The bound
    has teeth at this lr and eps: the decay coupling and eps each move the reference by far more than 1e-3, and the device
    result is that far from the OTHER optimizer's / eps's reference."""
    offs, total = _layout(SIZES)
    a, b = _device_run(K, kind, eps, with_coef)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    *flats, cancel = _reference(kind, eps, with_coef)
    assert cancel <= 2.0, cancel          # the inputs: no segment's weights cancel (_inputs)
    names = ("weights", "exp_avg", "exp_avg_sq")
    whole = [relerr(x.double(), r) for x, r in zip(a, flats)]
    worst = [max(relerr(x[o:o + n].double(), r[o:o + n]) for o, n in zip(offs, SIZES)) for x, r in zip(a, flats)]
    print(f"adam_groups {kind} eps={eps:g} coef={with_coef}: relerr whole buffer "
          + " ".join(f"{n} {e:.3e}" for n, e in zip(names, whole)) + "; worst segment "
          + " ".join(f"{n} {e:.3e}" for n, e in zip(names, worst)))
    pad = torch.ones(total, dtype=torch.bool)
    for o, n in zip(offs, SIZES):
        pad[o:o + n] = False
    assert int(pad.sum()) > 0
    for x, n in zip(a, names):
        assert float(x[pad].abs().max()) == 0.0, n                # the padding stays exactly zero
    if eps == 1e-3:
        other = _reference("Adam" if kind == "AdamW" else "AdamW", eps, with_coef)[0]
        far = relerr(a[0].double(), other)
        print(f"  ... and {far:.3e} from the {'Adam' if kind == 'AdamW' else 'AdamW'} reference")
        assert far > 1e-3
    else:
        far = relerr(a[0].double(), _reference(kind, 1e-3, with_coef)[0])
        print(f"  ... and {far:.3e} from the eps=1e-3 reference")
        assert far > 1e-3
    assert max(whole) < 1e-6 and max(worst) < 1e-6


@pytest.mark.parametrize("kind", ["AdamW", "Adam"])
def test_adam_groups_null_table_is_bit_equal_to_unit_multipliers(K, kind):
    offs, total = _layout(SIZES)
    table = K.SgdSegTable(offs + [total], [1.0] * len(SIZES), [0.03] * len(SIZES), "cuda")
    p = G.randn(77, total)
    a = [p.cuda(), torch.zeros(total, device="cuda"), torch.zeros(total, device="cuda")]
    b = [p.cuda(), torch.zeros(total, device="cuda"), torch.zeros(total, device="cuda")]
    for it in range(3):
        g = G.randn(78 + it, total).cuda()
        K.adam_groups_(a[0], g, a[1], a[2], 0, None, 0.02 * (it + 1), 0.03, BETAS, 1e-8, it + 1, 0.5, kind == "AdamW")
        K.adam_groups_(b[0], g, b[1], b[2], 0, table, 0.02 * (it + 1), 0.5, BETAS, 1e-8, it + 1, 0.5, kind == "AdamW")
    torch.cuda.synchronize()
    assert not torch.equal(a[0].cpu(), p)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_adam_groups_on_four_elements_and_on_none(K):
    """n == 4: one float4, checked against the host; n == 0: returns without a launch and without touching anything"""
    p, g = G.randn(31, 4), G.randn(32, 4)
    bufs = [p.cuda(), torch.zeros(4, device="cuda"), torch.zeros(4, device="cuda")]
    K.adam_groups_(bufs[0], g.cuda(), bufs[1], bufs[2], 0, None, 0.1, 0.05, BETAS, 1e-8, 1, 1.0, True)
    ps, ms, vs, _ = host_adam("AdamW", [p], [g], None, None, 1, [0.1], [0.05], BETAS, 1e-8, 1.0)
    torch.cuda.synchronize()
    for x, r in zip(bufs, (ps[0], ms[0], vs[0])):
        assert relerr(x.cpu().double(), r) < 1e-6
    big = [G.randn(33, 64).cuda() for _ in range(4)]
    keep = [x.clone() for x in big]
    table = K.SgdSegTable([0, 64], [1.0], [0.05], "cuda")
    for tab in (None, table):
        K.adam_groups_(big[0][8:8], big[1][8:8], big[2][8:8], big[3][8:8], 8, tab, 0.1, 0.05, BETAS, 1e-8, 1, 1.0, True)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(big, keep))
    from erd_amd._lib import ErdHipError
    with pytest.raises(ErdHipError, match="multiples of 4"):
        K.adam_groups_(big[0][:6], big[1][:6], big[2][:6], big[3][:6], 0, None, 0.1, 0.05, BETAS, 1e-8, 1, 1.0, True)


# ---------------------------------------------------------------------------------------------------------------------
# trainer
# ---------------------------------------------------------------------------------------------------------------------
OPT = dict(type="AdamW", lr=2e-3, betas=BETAS, eps=1e-8, weight_decay=0.05)


def _batches(seeds=(0, 1)):
    out = []
    for seed in seeds:
        imgs, boxes, labels = O.synthetic_batch(2, 123, 153, 40, seed=seed)
        x, metas = O.preprocess(imgs)
        out.append((x.cuda(), make_samples(boxes, labels, metas)))
    return out


def _slices(tr, t):
    return [t[o:o + p.numel()] for o, p in zip(tr.flat.offsets, tr.flat.params)]


def _check_update(tr, d0, m0, v0, t, g, lr, scale, max_norm, what):
    """flat.data / flat.momentum (exp_avg) / exp_avg_sq of `tr` against update number t of the fp64 host AdamW from (d0, m0, v0, g)
    under TABLE_CFG: below 1e-6 per parameter"""
    mult = [table_expect(n) for n in tr.flat.names]
    ps, ms, vs, norm = host_adam(tr.opt["type"], _slices(tr, d0), _slices(tr, g), _slices(tr, m0), _slices(tr, v0), t,
                                 [lr * a for a, _ in mult], [tr.weight_decay * b for _, b in mult], tr.opt["betas"], tr.opt["eps"],
                                 scale, max_norm)
    msg = []
    worst = 0.0
    for name, got, ref in (("weights", tr.flat.data, ps), ("exp_avg", tr.flat.momentum, ms), ("exp_avg_sq", tr.exp_avg_sq, vs)):
        errs = [relerr(a.cpu().double(), b) for a, b in zip(_slices(tr, got), ref)]
        i = errs.index(max(errs))
        msg.append(f"{name} {errs[i]:.3e} ({tr.flat.names[i]})")
        worst = max(worst, errs[i])
    print(f"{what}: worst parameter " + " ".join(msg))
    assert worst < 1e-6, what
    return norm


@pytest.mark.parametrize("bucket_update", ["1", "0"])
def test_trainer_adamw_update_with_paramwise_cfg_and_active_clipping(bucket_update, monkeypatch):
    """two train_step + flush() per round: the new weights and both moments equal the fp64 host AdamW step of (old state,
    flat.grad, t) with TABLE_CFG's groups and clip_grad_norm_ -- out of reach in the first round, at half the measured norm in
    the second -- to 1e-6 per parameter; the logged grad_norm equals the fp64 norm to 1e-6; t counts the updates."""
    from erd_amd.engine import ERDTrainer
    monkeypatch.setenv("ERD_BUCKET_UPDATE", bucket_update)
    tsd, ssd = f7_state_dicts()
    batches = _batches()
    norm0 = None
    for rnd in range(2):
        model = build_erd(tsd, ssd)
        max_norm = 1e9 if rnd == 0 else 0.5 * norm0
        tr = ERDTrainer(model, batch_size_per_gpu=2, auto_scale_lr=False, warmup_iters=0, bucket_mb=1, paramwise_cfg=TABLE_CFG,
                        clip_grad=dict(max_norm=max_norm, norm_type=2), optimizer=OPT)
        assert tr.bucket_update == (bucket_update == "1") and len(tr.flat.buckets) >= 4
        assert tr.base_lr == OPT["lr"] and tr.weight_decay == OPT["weight_decay"] and tr.optimizer_state_dict()["state"] == {}
        for step in range(2):
            d0, m0, v0 = tr.flat.data.clone(), tr.flat.momentum.clone(), tr.exp_avg_sq.clone()
            log = tr.train_step(*batches[step])
            tr.flush()
            torch.cuda.synchronize()
            assert tr._t == step + 1
            if bucket_update == "1":
                assert tr.sync.late_buckets == 0
            g = tr.flat.grad.clone()
            host_norm = float(g.cpu().double().norm())
            got = float(log["grad_norm"])
            print(f"bucket_update={bucket_update} max_norm={max_norm:.6g} step {step}: grad_norm {got:.9g} host {host_norm:.9g}")
            assert abs(got - host_norm) / host_norm < 1e-6
            assert (host_norm > max_norm) == (rnd == 1)            # clipping is active in the second round only
            _check_update(tr, d0, m0, v0, step + 1, g, tr.last_lr, 1.0, max_norm,
                          f"bucket_update={bucket_update} round {rnd} step {step}")
            if norm0 is None:
                norm0 = host_norm
        state = tr.optimizer_state_dict()["state"]
        assert len(state) == len(tr.flat.params) and all(float(st["step"]) == 2.0 for st in state.values())


@pytest.mark.parametrize("bucket_update", ["1", "0"])
def test_trainer_adamw_counts_one_update_per_closed_window(bucket_update, monkeypatch):
    from erd_amd.engine import ERDTrainer
    monkeypatch.setenv("ERD_BUCKET_UPDATE", bucket_update)
    tsd, ssd = f7_state_dicts()
    batches = _batches((0, 1, 2))
    model = build_erd(tsd, ssd)
    tr = ERDTrainer(model, batch_size_per_gpu=2, auto_scale_lr=False, warmup_iters=0, bucket_mb=1, paramwise_cfg=TABLE_CFG,
                    accumulative_counts=2, optimizer=OPT)
    state = lambda: (tr.flat.data.clone(), tr.flat.momentum.clone(), tr.exp_avg_sq.clone())
    same = lambda s: all(torch.equal(a, b) for a, b in zip(s, (tr.flat.data, tr.flat.momentum, tr.exp_avg_sq)))
    # first call: the window stays open -- weights, both moments and t are as before
    s0 = state()
    tr.train_step(*batches[0])
    tr.flush(close_window=False)
    torch.cuda.synchronize()
    assert same(s0) and tr._t == 0 and float(tr._acc.abs().max()) > 0
    # second call: the window closes -- scale 1/2, t = 1
    tr.train_step(*batches[1])
    tr.flush(close_window=False)
    torch.cuda.synchronize()
    assert tr._t == 1
    _check_update(tr, *s0, 1, tr._acc, tr.last_lr, 0.5, None, f"bucket_update={bucket_update} window of 2")
    # third call: open again
    s1 = state()
    tr.train_step(*batches[2])
    tr.flush(close_window=False)
    torch.cuda.synchronize()
    assert same(s1) and tr._t == 1
    # ... and flush() closes the partial window: one micro-step, scale 1, t = 2
    tr.flush()
    torch.cuda.synchronize()
    assert tr._t == 2
    _check_update(tr, *s1, 2, tr._acc, tr.last_lr, 1.0, None, f"bucket_update={bucket_update} window of 1")
    sd = tr.optimizer_state_dict()
    assert len(sd["param_groups"]) == len(list(model.parameters())) and all(float(st["step"]) == 2.0 for st in sd["state"].values())


def test_plain_trainer_allocates_no_second_moment():
    from erd_amd.engine import ERDTrainer
    tsd, ssd = f7_state_dicts()
    tr = ERDTrainer(build_erd(tsd, ssd))
    assert tr.exp_avg_sq is None and not tr.adam and tr.opt["type"] == "SGD"
    tr = ERDTrainer(build_erd(tsd, ssd), optimizer=dict(type="SGD", lr=0.01, momentum=0.9, weight_decay=1e-4))
    assert tr.exp_avg_sq is None and not tr.adam
    tr = ERDTrainer(build_erd(tsd, ssd), optimizer=dict(type="Adam"))
    assert tr.exp_avg_sq is not None and tr.exp_avg_sq.shape == tr.flat.momentum.shape and tr._table is None
    with pytest.raises(ValueError, match="SGD.*Adam"):
        tr.load_optimizer_state_dict(dict(state={0: dict(momentum_buffer=torch.zeros(1))}, param_groups=[]))


def test_runner_adamw_config_trains_checkpoints_torch_layout_and_resumes(tmp_path):
    from erd_amd import Config
    from erd_amd.runner import Runner, SyntheticDetData
    teacher = tmp_path / "teacher.pth"
    torch.save(dict(state_dict=O.procedural_state_dict(40, seed=0)), teacher)

    def cfg(path, work, **over):
        c = Config.fromfile(path)
        c.work_dir = str(tmp_path / work)
        c.merge_from_dict({"train_dataloader.batch_size": 2, "train_cfg.max_epochs": 1, "model.backbone.init_cfg": None,
                           "default_hooks.logger.interval": 1, "model.ori_setting.ori_checkpoint_file": str(teacher),
                           "model.ori_setting.ori_config_file": CFG_FIRST, **over})
        return c

    data = lambda: SyntheticDetData(2, 40, 4, image_hw=(123, 153), seed=1)
    torch.manual_seed(3)
    r = Runner.from_cfg(cfg(CFG_ADAMW, "w"), data=data(), log=lambda *_: None)
    tr = r.trainer
    assert tr.adam and tr.opt == dict(type="AdamW", lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
    assert tr.clip == dict(max_norm=35.0, error_if_nonfinite=False) and tr.resolved is not None and tr.accum == 1
    d0 = tr.flat.data.clone()
    hist = r.train()
    assert len(hist) == 4 and tr.iter == 4 and tr._t == 4 and all(h["grad_norm"] > 0 for h in hist)
    assert not torch.equal(tr.flat.data, d0) and bool(torch.isfinite(tr.flat.data).all())
    ck = torch.load(tmp_path / "w" / "epoch_1.pth", map_location="cpu", weights_only=False)
    names = [n for n, _ in r.model.named_parameters()]
    groups, state = ck["optimizer"]["param_groups"], ck["optimizer"]["state"]
    assert len(groups) == len(names) and len(state) == len(tr.flat.params)
    assert all(st["step"].dtype == torch.float32 and st["step"].dim() == 0 and float(st["step"]) == 4.0 for st in state.values())
    base_lr = 1e-4 * 2 / 16                                        # auto_scale_lr: one GPU x 2 images against 16
    for name, (lr, wd) in {"backbone.layer4.0.conv1.weight": (0.1, 0.05), "backbone.layer2.0.bn1.weight": (0.1, 0.05),
                           "bbox_head.cls_convs.0.gn.weight": (1.0, 0.0), "bbox_head.gfl_cls.weight": (1.0, 0.05)}.items():
        g = groups[names.index(name)]
        assert g["params"] == [names.index(name)] and g["betas"] == (0.9, 0.999) and g["eps"] == 1e-8 and g["amsgrad"] is False
        assert g["initial_lr"] == pytest.approx(base_lr * lr, rel=1e-9) and g["weight_decay"] == pytest.approx(wd, rel=1e-9, abs=0)
    # the checkpoint loads into a stock torch.optim.AdamW with matching groups, and that optimizer steps
    host = [torch.nn.Parameter(torch.zeros_like(p, device="cpu")) for p in r.model.parameters()]
    opt = torch.optim.AdamW([dict(params=[p]) for p in host], lr=1e-4)
    import copy
    opt.load_state_dict(copy.deepcopy(ck["optimizer"]))       # (load_state_dict keeps the tensors it is given: the step below is in place)
    i = names.index("bbox_head.gfl_cls.weight")
    assert torch.equal(opt.state[host[i]]["exp_avg_sq"], state[i]["exp_avg_sq"]) and float(opt.state[host[i]]["step"]) == 4.0
    assert float(state[i]["exp_avg_sq"].max()) > 0 and state[i]["exp_avg"].shape == host[i].shape
    host[i].grad = torch.zeros_like(host[i])
    opt.step()
    assert float(opt.state[host[i]]["step"]) == 5.0
    # resume: the same state bit for bit, the same groups (but `lr`: the resumed trainer has taken no step yet), the same count
    r2 = Runner.from_cfg(cfg(CFG_ADAMW, "w", resume=True), data=data(), log=lambda *_: None)
    assert r2.epoch == 1 and r2.trainer.iter == 4 and r2.trainer._t == 4
    sd2 = r2.trainer.optimizer_state_dict()
    assert sd2["state"].keys() == state.keys()
    for j, st in state.items():
        assert all(torch.equal(sd2["state"][j][k], st[k]) for k in ("step", "exp_avg", "exp_avg_sq")), j
    strip = lambda gs: [{k: v for k, v in g.items() if k != "lr"} for g in gs]
    assert strip(sd2["param_groups"]) == strip(groups)
    # the state of one optimizer kind does not load into the other
    rs = Runner.from_cfg(cfg(CFG_INCRE, "s"), data=data(), log=lambda *_: None)
    rs.train()
    assert "momentum_buffer" in next(iter(rs.trainer.optimizer_state_dict()["state"].values()))
    with pytest.raises(ValueError, match="AdamW/Adam.*SGD"):
        Runner.from_cfg(cfg(CFG_INCRE, "w", resume=True), data=data(), log=lambda *_: None)
    with pytest.raises(ValueError, match="SGD.*AdamW"):
        Runner.from_cfg(cfg(CFG_ADAMW, "s", resume=True), data=data(), log=lambda *_: None)
