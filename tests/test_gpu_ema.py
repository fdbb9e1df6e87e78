"""GPU: the EMAHook in ERDTrainer and Runner on the tiny ERD model (R50 40+40, batch 2 at 128x160).

The average is checked bit for bit against the host restatement tests/ema_refs.py replayed over snapshots of the weights.

Comparisons BETWEEN TWO RUNS (with / without the hook, swapped / never swapped, resumed / straight, captured / eager) are bit for
bit as well, which needs one precaution: the gradients of the 0-d and 1-d parameters (biases, BN / GN affine pairs, the head's
scales) are float-atomic column sums whose last bits depend on arrival order, so two identical runs of this
trainer part after one step.  Every trainer of this file therefore gives those parameters a learning-rate multiplier of exactly 0
through `paramwise_cfg` (`_freeze_small`): their gradients are still computed, the update leaves them as they are, the matrices
train, and a run is reproducible to the bit (tests/test_gpu_optim_cfg.py::test_unit_custom_key_leaves_the_weights_of_a_plain_trainer
holds the >= 2-d parameters of two runs bit-equal in the same way).  The average covers every trainable tensor either way."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("oracle_threads")]

import e2e_util as U
import ema_refs as E
from e2e_util import ROOT, build_erd, f7_state_dicts, make_samples
from oracle import erd_oracle as O

CFG_EMA = os.path.join(ROOT, "configs", "gfl_increment", "gfl_r50_fpn_1x_coco_first_40_incre_last_40_cats_ema.py")
HALF = dict(ema_type="ExponentialMovingAverage", momentum=0.5, interval=2)
EXP3 = dict(ema_type="ExpMomentumEMA", momentum=0.0002, gamma=3)
HOOK_HALF = [dict(type="EMAHook", momentum=0.5, priority=49)]
UPDATE_PATH = ("erd_sgd_momentum", "erd_sgd_momentum_groups", "erd_adam_groups", "erd_bn_fold_batch", "erd_weight_prep_batch",
               "erd_grad_accumulate", "erd_to_bf16", "erd_ema_update", "erd_swap_f32")


def _checked(**kw):
    from erd_amd import optim_cfg as OC
    return OC.check_custom_hooks([dict(type="EMAHook", **kw)])


@functools.lru_cache(maxsize=None)
def _state():
    return f7_state_dicts()


@functools.lru_cache(maxsize=None)
def _batch(seed):
    imgs, boxes, labels = O.synthetic_batch(2, 128, 160, 40, seed=seed)
    x, metas = O.preprocess(imgs)
    assert tuple(x.shape[2:]) == (128, 160)
    return x.cuda(), make_samples(boxes, labels, metas)


def _freeze_small(model):
    """paramwise_cfg: learning-rate multiplier 0 for every trainable parameter with fewer than two dimensions (module docstring)"""
    names = [n for n, p in model.named_parameters() if p.requires_grad and p.dim() < 2 and not n.startswith("ori_model.")]
    assert len(names) > 50
    return dict(custom_keys={n: dict(lr_mult=0.) for n in names})


def _trainer(ema=None, **kw):
    from erd_amd.engine import ERDTrainer
    model = build_erd(*_state())
    tr = ERDTrainer(model, lr=0.02, batch_size_per_gpu=2, auto_scale_lr=False, warmup_iters=0, bucket_mb=1,
                    paramwise_cfg=_freeze_small(model), ema=ema, **kw)
    small = {id(p) for p in tr.flat.params if p.dim() < 2}
    index = {id(q): i for i, q in enumerate(model.parameters())}
    assert all((tr.resolved[index[id(p)]]["lr_mult"] == 0.0) == (id(p) in small) for p in tr.flat.params)
    return tr


def _run(tr, steps, look_ahead=False, first=0):
    """`steps` training steps on batches first, first + 1, ...; after each the step's own update is settled (the accumulation
    window is left as it is) and the weights -- and the average -- are copied to the host"""
    ws, avgs = [], []
    for i in range(first, first + steps):
        nxt = _batch(i + 1) if look_ahead and i + 1 < first + steps else None
        log = tr.train_step(*_batch(i), next_batch=nxt)
        tr.flush(close_window=False)
        torch.cuda.synchronize()
        assert np.isfinite(float(torch.as_tensor(log["loss"]).detach()))
        ws.append(tr.flat.data.cpu().numpy().copy())
        if tr.ema is not None:
            avgs.append(tr.ema_buf.cpu().numpy().copy())
    return ws, avgs


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


@pytest.fixture(scope="module")
def plain_run():
    """five steps of the trainer WITHOUT the hook: the weights after each (shared, read only) and its update-path calls"""
    from erd_amd import kernels as K
    calls, real = [], K.call
    K.call = lambda name, *a: (calls.append(name) if name in UPDATE_PATH else None, real(name, *a))[1]
    try:
        tr = _trainer()
        assert tr.ema is None and tr.ema_buf is None and tr.bucket_update and len(tr.flat.buckets) >= 4
        ws, _ = _run(tr, 5)
    finally:
        K.call = real
    return ws, calls, len(tr.flat.buckets)


def test_training_is_untouched_by_the_hook(plain_run):
    """the same five steps with the hook: the weights after EVERY step are bit-equal to the run without it, and the update path
    issues the same launches in the same order plus one erd_ema_update behind each bucket's update -- none without the hook"""
    from erd_amd import kernels as K
    ws0, calls0, nb = plain_run
    assert "erd_ema_update" not in calls0 and "erd_swap_f32" not in calls0
    calls, real = [], K.call
    K.call = lambda name, *a: (calls.append(name) if name in UPDATE_PATH else None, real(name, *a))[1]
    try:
        tr = _trainer(_checked(**HALF))
        ws, avgs = _run(tr, 5)
    finally:
        K.call = real
    assert not _same(ws0[0], ws0[1]) and not _same(ws[4], avgs[4])
    for i in range(5):
        assert _same(ws[i], ws0[i]), i
    assert [c for c in calls if c != "erd_ema_update"] == calls0
    # interval 2: copy, skip, average, skip, average -> three of the five steps launch, once per bucket, right behind the update
    assert calls.count("erd_ema_update") == 3 * nb
    upd = [i for i, c in enumerate(calls) if c == "erd_sgd_momentum_groups"]
    assert len(upd) == 5 * nb and sum(calls[i + 1] == "erd_ema_update" for i in upd) == 3 * nb


CASES = {
    # name: (hook keys, trainer options, ERD_BUCKET_UPDATE, teacher look-ahead)
    "interval2-buckets": (HALF, {}, "1", False),
    "interval2-whole": (HALF, {}, "0", False),
    "expmomentum-buckets-lookahead": (EXP3, {}, "1", True),
    "expmomentum-whole-lookahead": (EXP3, {}, "0", True),
    "begin3-buckets": (dict(momentum=0.5, begin_iter=3), {}, "1", False),
    "accumulate2-buckets": (EXP3, dict(accumulative_counts=2), "1", False),
    "accumulate2-whole": (EXP3, dict(accumulative_counts=2), "0", True),
    "adamw-buckets": (EXP3, dict(optimizer=dict(type="AdamW", lr=1e-3)), "1", False),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_average_is_the_restatement_replayed_over_the_weights(case, monkeypatch):
    keys, opts, bucket_update, look_ahead = CASES[case]
    monkeypatch.setenv("ERD_BUCKET_UPDATE", bucket_update)
    cfg = _checked(**keys)
    tr = _trainer(cfg, **opts)
    assert tr.bucket_update == (bucket_update == "1") and _same(tr.ema_buf.cpu().numpy(), tr.flat.data.cpu().numpy())
    ws, avgs = _run(tr, 5, look_ahead=look_ahead)
    want, steps = E.replay(cfg, ws)
    for i in range(5):
        assert E.same_bits(avgs[i], want[i]), (case, i, int((avgs[i].view(np.uint32) != want[i].view(np.uint32)).sum()))
    assert tr.ema_steps == steps == (3 if "begin3" in case else 5)
    moved = [not _same(ws[i], ws[i - 1]) for i in range(1, 5)]
    assert moved == ([True, False, True, False] if "accumulate2" in case else [True] * 4), "the weights the average follows do move"
    assert not _same(avgs[4], ws[4]) and not _same(avgs[4], avgs[1])
    if "begin3" in case:                      # not started: a copy after iterations 1 and 2; started at the third: a copy once more
        assert all(_same(avgs[i], ws[i]) for i in range(3)) and not _same(avgs[3], ws[3])
    if "accumulate2" in case:                 # the hook runs on every micro-step; closing the open window is no iteration
        assert _same(ws[2], ws[1]) and not _same(avgs[2], avgs[1])
        tr.flush()
        torch.cuda.synchronize()
        assert not _same(tr.flat.data.cpu().numpy(), ws[4]) and _same(tr.ema_buf.cpu().numpy(), avgs[4]) and tr.ema_steps == 5
    assert "ema" not in str(sorted(tr.optimizer_state_dict())), "the optimizer state is as before: the average travels apart"


def _derived(tr):
    out = {"data": tr.flat.data, "average": tr.ema_buf, "momentum": tr.flat.momentum, "grad": tr.flat.grad}
    if tr.flat.data_bf16 is not None:
        out["data_bf16"] = tr.flat.data_bf16
    if tr.prefold is not None and tr.prefold.bns:
        out["bn folds"] = tr.prefold.buf
    for k, r in (tr.prep.recipes.items() if tr.prep is not None else []):
        if tr.prep.lookup(k) is r:
            out[f"prep{k}"] = r.out
    return {k: v.detach().clone() for k, v in out.items()}


def _predict(model, seed=7):
    imgs, boxes, labels = O.synthetic_batch(2, 128, 160, 40, seed=seed)
    x, metas = O.preprocess(imgs)
    for m in metas:
        m["scale_factor"] = (0.8, 0.8)
    x, samples = x.cuda(), make_samples(boxes, labels, metas)
    was, head = model.training, model.bbox_head
    cfg = head.test_cfg
    head.test_cfg = dict(cfg, score_thr=0.001)          # (procedural weights score low: keep detections to compare)
    model.eval()
    try:
        with torch.no_grad():
            out = model(x, samples, mode="predict")
    finally:
        model.train(was)
        head.test_cfg = cfg
    return [(d.pred_instances.bboxes.cpu(), d.pred_instances.scores.cpu(), d.pred_instances.labels.cpu()) for d in out]


@pytest.mark.parametrize("mode", ["f32x3", "bf16"])
def test_swap_carries_every_piece_of_derived_state(mode):
    from erd_amd import kernels as K
    K.set_compute(mode)
    try:
        cfg = _checked(momentum=0.5)
        straight = _trainer(cfg)
        ws0, avgs0 = _run(straight, 5)
        tr = _trainer(cfg)
        ws, avgs = _run(tr, 3)
        assert _same(ws[2], ws0[2]) and _same(avgs[2], avgs0[2])
        tr.flush()
        torch.cuda.synchronize()
        before = _derived(tr)
        assert (mode == "bf16") == ("data_bf16" in before) and len(before) > 6
        raw_predictions = _predict(tr.model)
        tr.swap_ema()
        torch.cuda.synchronize()
        assert tr.ema_swapped and _same(tr.flat.data.cpu().numpy(), avgs[2]) and _same(tr.ema_buf.cpu().numpy(), ws[2])
        if mode == "bf16":
            assert torch.equal(tr.flat.data_bf16, tr.flat.data.to(torch.bfloat16))
        with pytest.raises(RuntimeError, match="swap_ema"):
            tr.train_step(*_batch(3))
        # the live model under the averaged weights == a fresh model that was given them
        got = _predict(tr.model)
        fresh = build_erd(*_state())
        fresh.load_state_dict({k: v.detach().cpu() for k, v in tr.model.state_dict().items()}, strict=True)
        want = _predict(fresh.cuda())
        del fresh
        assert sum(int(b.shape[0]) for b, _, _ in want) > 0
        for g, w in zip(got, want):
            assert all(torch.equal(a, b) for a, b in zip(g, w))
        assert any(not torch.equal(a, b) for g, w in zip(got, raw_predictions) for a, b in zip(g, w) if a.shape == b.shape) or \
            any(a.shape != b.shape for g, w in zip(got, raw_predictions) for a, b in zip(g, w)), "the average predicts differently"
        tr.swap_ema()
        torch.cuda.synchronize()
        after = _derived(tr)
        assert not tr.ema_swapped and sorted(after) == sorted(before)
        for k, v in before.items():
            assert torch.equal(v, after[k]), k
        # ... and training goes on as if nothing had happened
        ws2, avgs2 = _run(tr, 2, first=3)
        for i in range(2):
            assert _same(ws2[i], ws0[3 + i]) and _same(avgs2[i], avgs0[3 + i]), i
    finally:
        K.set_compute(K.DEFAULT_COMPUTE)


def test_step_graph_with_the_hook_replays_and_averages_like_the_eager_run():
    cfg = _checked(**EXP3)
    eager = _trainer(cfg)
    ws0, avgs0 = _run(eager, 3)
    tr = _trainer(cfg, step_graph=True)
    assert tr.step_graph
    ws, avgs = _run(tr, 3)
    assert len(tr._step_graphs) == 1
    want, _ = E.replay(cfg, ws)
    for i in range(3):
        assert E.same_bits(avgs[i], want[i]), i
        assert _same(ws[i], ws0[i]) and _same(avgs[i], avgs0[i]), i
    tr.swap_ema()
    assert len(tr._step_graphs) == 0          # a captured step is recorded anew after the exchange
    tr.swap_ema()
    ws2, avgs2 = _run(tr, 1, first=3)
    assert E.same_bits(avgs2[0], E.update(avgs[2], ws2[0], E.coefficient("ExpMomentumEMA", 0.0002, 3, 3))) and len(tr._step_graphs) == 1


# ---- Runner: validation, checkpoints, resume, tools/train.py ------------------------------------------------------------------------
def _cfg(tmp_path, work, hooks=HOOK_HALF, epochs=1, **over):
    from erd_amd import Config, MODELS
    teacher = tmp_path / "teacher.pth"
    if not teacher.exists():
        torch.save(dict(state_dict=O.procedural_state_dict(40, seed=0)), teacher)
    c = Config.fromfile(U.CFG_INCRE)
    c.work_dir = str(tmp_path / work)
    c.merge_from_dict({"train_dataloader.batch_size": 2, "train_cfg.max_epochs": epochs, "model.backbone.init_cfg": None,
                       "default_hooks.logger.interval": 1, "model.ori_setting.ori_checkpoint_file": str(teacher),
                       "model.ori_setting.ori_config_file": U.CFG_FIRST, **over})
    probe = Config.fromfile(U.CFG_INCRE)
    probe.model.latest_model_flag = False
    c.merge_from_dict({"optim_wrapper.paramwise_cfg": _freeze_small(MODELS.build(probe.model))})
    if hooks is not None:
        c.merge_from_dict({"custom_hooks": hooks})
    return c


def _data(iters=2):
    from erd_amd.runner import SyntheticDetData
    return SyntheticDetData(2, 40, iters, image_hw=(128, 160), seed=1)


def _runner(cfg, lines=None, **kw):
    from erd_amd.runner import Runner
    torch.manual_seed(5)
    return Runner(cfg, data=_data(), log=(lines.append if lines is not None else (lambda *_: None)), **kw)


def test_runner_validates_the_averaged_weights_and_trains_on_the_raw_ones(tmp_path):
    from test_gpu_validation import _same_stats, _trainer_state, _val_data, _val_set
    from erd_amd import Config, MODELS
    _val_set(tmp_path)
    cfg = _cfg(tmp_path, "w", **{"train_cfg.val_interval": 1, "model.test_cfg.score_thr": 0.001,
                                 "val_evaluator.ann_file": str(tmp_path / "val.json")})
    lines = []
    r = _runner(cfg, lines, val_data=_val_data(tmp_path))
    assert r.ema == _checked(momentum=0.5) and r.trainer.ema == r.ema
    seen, run = [], r.validator.run
    r.validator.run = lambda model, *a, **k: (seen.append((r.trainer.flat.data.clone(), r.trainer.ema_swapped)), run(model, *a, **k))[1]
    hist = r.train()
    tr = r.trainer
    vals = [h for h in hist if h.get("mode") == "val"]
    assert len(vals) == 1 and len(seen) == 1 and "Epoch(val) [1][3/3]" in "\n".join(lines)
    assert seen[0][1] is True and torch.equal(seen[0][0], tr.ema_buf), "the pass saw the average"
    assert not tr.ema_swapped and not torch.equal(tr.flat.data, tr.ema_buf) and tr.ema_steps == 2
    # the saved checkpoint evaluated the way tools/test.py does it: a fresh detector with `state_dict` as it stands
    probe = Config.fromfile(U.CFG_INCRE)
    probe.merge_from_dict({"model.test_cfg.score_thr": 0.001})
    probe.model.latest_model_flag = False
    fresh = MODELS.build(probe.model).cuda().eval()
    sd = torch.load(tmp_path / "w" / "epoch_1.pth", map_location="cpu", weights_only=False)["state_dict"]
    own = fresh.state_dict()
    fresh.load_state_dict({**own, **{k: v for k, v in sd.items() if k in own}}, strict=True)
    stats = run(fresh)
    _same_stats(stats, {k[5:]: v for k, v in vals[0].items() if k.startswith("coco/")})
    # one more pass: the same numbers, and every piece of trainer state is bitwise as it was (the test of the plain runner)
    before = _trainer_state(r), tr.ema_buf.clone(), tr.ema_steps
    again = r.validate()
    after = _trainer_state(r), tr.ema_buf.clone(), tr.ema_steps
    _same_stats(again, stats)
    # (the prepared weights were rebuilt twice, for the average and for the raw weights again: their stamp moved on)
    drop = lambda meta: {k: v for k, v in meta.items() if k != "prep_stamp"}
    assert drop(before[0][1]) == drop(after[0][1]) and before[2] == after[2] and torch.equal(before[1], after[1])
    assert sorted(before[0][0]) == sorted(after[0][0]) and all(torch.equal(v, after[0][0][k]) for k, v in before[0][0].items())
    # a failing pass still exchanges back
    r.validator.run = lambda *a, **k: (_ for _ in ()).throw(RuntimeError("boom"))
    with pytest.raises(RuntimeError, match="boom"):
        r.validate()
    assert not tr.ema_swapped and torch.equal(tr.flat.data, before[0][0]["data"])


@pytest.fixture(scope="module")
def first_epoch(tmp_path_factory):
    """one epoch (two iterations) under the hook: the runner, its work directory's parent and epoch_1.pth (shared, read only)"""
    tmp_path = tmp_path_factory.mktemp("ema_ckpt")
    r1 = _runner(_cfg(tmp_path, "a"))
    r1.train()
    return r1, tmp_path, str(tmp_path / "a" / "epoch_1.pth")


def test_checkpoint_holds_the_average_and_the_raw_weights_apart(first_epoch):
    r1, tmp_path, path = first_epoch
    tr = r1.trainer
    ck = torch.load(path, map_location="cpu", weights_only=False)
    sd, esd = ck["state_dict"], ck["ema_state_dict"]
    assert sorted(ck) == ["ema_state_dict", "meta", "optimizer", "state_dict"] and ck["meta"]["iter"] == 2
    assert esd["steps"].dtype == torch.long and esd["steps"].dim() == 0 and int(esd["steps"]) == 2
    assert sorted(k for k in esd if k != "steps") == sorted("module." + k for k in sd if not k.startswith("ori_model."))
    assert any(k.startswith("ori_model.") for k in sd) and not any(k.startswith("module.ori_model.") for k in esd)
    raw = tr.ema_state()["tensors"]           # name -> (training weights, average), device copies
    assert len(raw) == len(tr.flat.params) and not tr.ema_swapped
    differ = 0
    for k in sd:
        if k.startswith("ori_model."):
            continue
        if k in raw:                          # trainable: state_dict holds the average, ema_state_dict the training weights
            assert torch.equal(sd[k], raw[k][1].cpu()) and torch.equal(esd["module." + k], raw[k][0].cpu()), k
            assert sd[k].is_contiguous() and esd["module." + k].is_contiguous()
            differ += int(not torch.equal(sd[k], esd["module." + k]))
        else:                                 # frozen tensors and buffers are the model's own under both sets of weights
            assert torch.equal(sd[k], esd["module." + k]), k
    assert differ > 50


def test_resume_exchanges_back_and_ends_where_the_straight_run_does(first_epoch):
    """resume: the two dictionaries are exchanged back, `steps` is restored, and two more steps end where four straight ones do"""
    r1, tmp_path, path = first_epoch
    tr = r1.trainer
    lines = []
    r2 = _runner(_cfg(tmp_path, "b", epochs=2, load_from=path, resume=True), lines)
    t2 = r2.trainer
    assert r2.epoch == 1 and t2.iter == 2 and t2.ema_steps == 2 and "resumed" in lines[-1]
    assert torch.equal(t2.flat.data, tr.flat.data) and torch.equal(t2.ema_buf, tr.ema_buf) and torch.equal(t2.flat.momentum, tr.flat.momentum)
    r2.train()
    r4 = _runner(_cfg(tmp_path, "c", epochs=2))
    r4.train()
    assert t2.iter == r4.trainer.iter == 4 and t2.ema_steps == r4.trainer.ema_steps == 4
    assert torch.equal(t2.flat.data, r4.trainer.flat.data) and torch.equal(t2.ema_buf, r4.trainer.ema_buf)
    assert not torch.equal(t2.flat.data, tr.flat.data)


def test_loading_without_resume_and_the_two_mismatches(first_epoch):
    from erd_amd.runner import load_checkpoint
    r1, tmp_path, path = first_epoch
    tr = r1.trainer
    ck = torch.load(path, map_location="cpu", weights_only=False)
    sd = ck["state_dict"]
    # loading without resume takes `state_dict` as it stands (the average), and the new average starts as a copy of it
    r5 = _runner(_cfg(tmp_path, "d", load_from=path))
    assert torch.equal(r5.trainer.flat.data, tr.ema_buf) and torch.equal(r5.trainer.ema_buf, tr.ema_buf) and r5.trainer.ema_steps == 0
    # the hook without ema_state_dict: the average starts as a copy of the weights, one line says so
    plain = dict(ck)
    del plain["ema_state_dict"]
    torch.save(plain, tmp_path / "plain.pth")
    lines = []
    r6 = _runner(_cfg(tmp_path, "e", epochs=2, load_from=str(tmp_path / "plain.pth"), resume=True), lines)
    assert sum("holds no ema_state_dict" in l and "copy" in l for l in lines) == 1
    assert r6.trainer.ema_steps == 0 and torch.equal(r6.trainer.flat.data, tr.ema_buf) and torch.equal(r6.trainer.ema_buf, tr.ema_buf)
    # ema_state_dict without the hook: the RAW weights are restored and one line says that the average was dropped
    lines = []
    r7 = _runner(_cfg(tmp_path, "f", hooks=None, epochs=2, load_from=path, resume=True), lines)
    assert sum("ema_state_dict" in l and "dropped" in l for l in lines) == 1
    assert r7.trainer.ema is None and r7.trainer.ema_buf is None and torch.equal(r7.trainer.flat.data, tr.flat.data)
    assert torch.equal(r7.trainer.flat.momentum, tr.flat.momentum)
    # ... and a model alone (no trainer: tools/test.py, the next phase's teacher) reads the average
    fresh = build_erd(*_state())
    load_checkpoint(path, fresh)
    assert torch.equal(fresh.bbox_head.gfl_cls.weight.detach().cpu(), sd["bbox_head.gfl_cls.weight"])
    with pytest.raises(ValueError, match="SyncNormHook"):
        _runner(_cfg(tmp_path, "g", hooks=[dict(type="SyncNormHook")]))


def test_train_py_runs_one_epoch_on_the_ema_config(tmp_path):
    teacher = tmp_path / "teacher.pth"
    torch.save(dict(state_dict=O.procedural_state_dict(40, seed=0)), teacher)
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train.py"), CFG_EMA, "--work-dir", str(tmp_path / "w"),
           "--synthetic", "4", "--image-size", "128", "160", "--cfg-options", "train_dataloader.batch_size=2", "train_cfg.max_epochs=1",
           f"model.ori_setting.ori_checkpoint_file={teacher}", f"model.ori_setting.ori_config_file={U.CFG_FIRST}",
           "model.backbone.init_cfg=None", "default_hooks.logger.interval=1"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "Epoch(train) [1][4/4]" in out.stdout
    ck = torch.load(tmp_path / "w" / "epoch_1.pth", map_location="cpu", weights_only=False)
    sd, esd = ck["state_dict"], ck["ema_state_dict"]
    assert int(esd["steps"]) == 4
    keys = [k for k in sd if not k.startswith("ori_model.")]
    assert all("module." + k in esd for k in keys)
    assert any(not torch.equal(sd[k], esd["module." + k]) for k in keys), "state_dict holds the average, not the training weights"
    assert all(sd[k].shape == esd["module." + k].shape for k in keys)
