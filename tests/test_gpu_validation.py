"""GPU: validation inside the training loop (Runner.validate after each epoch: train_cfg.val_interval, val_dataloader, val_evaluator)
and the sharded test (tools/test.py --launcher pytorch).  (a) the log and scalars.json carry one `Epoch(val)` record per epoch;
(b) the epoch-2 stats equal tools/test.py on epoch_2.pth at batch size 1 with the host and with the device evaluator, bit for bit;
(c) a validation pass leaves every piece of trainer state bitwise as it was; (d) two gloo ranks on one GPU give the world-1 stats."""
import json
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import e2e_util as U
from e2e_util import ROOT


def _val_set(tmp_path):
    """three small PNGs, 80 categories with ids 10..89 (the incremental model's label space), two boxes per image"""
    from PIL import Image
    rng = np.random.RandomState(3)
    (tmp_path / "val").mkdir()
    images, anns = [], []
    for i, (h, w) in enumerate([(120, 150), (140, 100), (100, 160)]):
        Image.fromarray(rng.randint(0, 256, (h, w, 3), dtype=np.uint8)).save(tmp_path / "val" / f"{i:04d}.png")
        images.append(dict(id=100 + i, file_name=f"{i:04d}.png", width=w, height=h))
        for k in range(2):
            x, y = rng.uniform(0, w - 20), rng.uniform(0, h - 20)
            bw, bh = rng.uniform(8, w - x), rng.uniform(8, h - y)
            anns.append(dict(id=len(anns) + 1, image_id=100 + i, category_id=10 + 38 + 2 * k + i, iscrowd=0,
                             bbox=[float(x), float(y), float(bw), float(bh)], area=float(bw * bh)))
    ds = dict(images=images, annotations=anns, categories=[dict(id=10 + k, name=f"k{k}") for k in range(80)])
    json.dump(ds, open(tmp_path / "val.json", "w"))
    return ds


def _over(tmp_path, teacher):
    return {"train_dataloader.batch_size": 2, "train_cfg.max_epochs": 2, "train_cfg.val_interval": 1,
            "model.backbone.init_cfg": None, "default_hooks.logger.interval": 1, "model.test_cfg.score_thr": 0.001,
            "model.ori_setting.ori_checkpoint_file": str(teacher), "model.ori_setting.ori_config_file": U.CFG_FIRST,
            "val_evaluator.ann_file": str(tmp_path / "val.json")}


def _val_data(tmp_path):
    return dict(data_root=f"{tmp_path}/", ann_file="val.json", data_prefix=dict(img="val/"))


def _test_opts(tmp_path):
    return ["--cfg-options", f"test_dataloader.dataset.data_root={tmp_path}/", "test_dataloader.dataset.ann_file=val.json",
            "test_dataloader.dataset.data_prefix.img=val/", "model.test_cfg.score_thr=0.001"]


def _same_stats(a, b):
    assert sorted(a) == sorted(b), (sorted(a), sorted(b))
    for k in a:
        assert a[k] == b[k] or (math.isnan(a[k]) and math.isnan(b[k])), (k, a[k], b[k])


def _trainer_state(r):
    """every tensor the trainer carries between steps, plus its counters and the RNGs a sampler could draw from"""
    t = r.trainer
    snap = {"data": t.flat.data, "grad": t.flat.grad, "momentum": t.flat.momentum}
    if getattr(t.flat, "data_bf16", None) is not None:
        snap["data_bf16"] = t.flat.data_bf16
    if t.prefold is not None and getattr(t.prefold, "buf", None) is not None:
        snap["bn_folds"] = t.prefold.buf
    for key, rec in (t.prep.recipes.items() if t.prep is not None else []):
        snap[f"prep{key}"] = rec.out
    for k, v in r.model.state_dict().items():
        snap["model." + k] = v
    snap = {k: v.detach().clone() for k, v in snap.items()}
    meta = dict(iter=t.iter, epoch=r.epoch, lr=t.last_lr, plan=t._plan, epoch_factor=t.epoch_factor,
                pending=t._pending, first=t._first, ahead=t._teacher_ahead is None,
                prep_stamp=None if t.prep is None else t.prep.stamp, prefold_valid=None if t.prefold is None else list(t.prefold.valid),
                training=r.model.training, recipes=None if t.prep is None else sorted(map(str, t.prep.recipes)))
    rngs = (torch.get_rng_state(), torch.cuda.get_rng_state(), np.random.get_state()[1].copy())
    return snap, meta, rngs


def test_validation_each_epoch_matches_test_py_and_leaves_the_trainer_alone(tmp_path):
    from oracle import erd_oracle as O
    from erd_amd.runner import Runner, SyntheticDetData
    from erd_amd import Config
    _val_set(tmp_path)
    teacher = tmp_path / "teacher.pth"
    torch.save(dict(state_dict=O.procedural_state_dict(40, seed=0)), teacher)
    cfg = Config.fromfile(U.CFG_INCRE)
    cfg.work_dir = str(tmp_path / "w")
    cfg.merge_from_dict(_over(tmp_path, teacher))
    lines = []
    torch.manual_seed(5)
    r = Runner(cfg, data=SyntheticDetData(2, 40, 2, image_hw=(123, 153), seed=1), val_data=_val_data(tmp_path),
               log=lines.append)
    hist = r.train()
    # (a) one validation record per epoch, in the log and in scalars.json
    log = "\n".join(lines)
    assert "Epoch(val) [1][3/3]  coco/bbox_mAP:" in log and "Epoch(val) [2][3/3]  coco/bbox_mAP:" in log, log[-2000:]
    assert "coco/bbox_mAP_50:" in log and "coco/old_mAP:" in log and "coco/new_mAP:" in log
    vals = [h for h in hist if h.get("mode") == "val"]
    assert [v["epoch"] for v in vals] == [1, 2]
    recs = [json.loads(l) for l in open(tmp_path / "w" / "scalars.json")]
    assert [x["epoch"] for x in recs if x.get("mode") == "val"] == [1, 2]
    assert sum(1 for x in recs if "mode" not in x) == 4                     # the training records are as before
    print(f"\nvalidation pass (3 images): {vals[-1]['time']:.3f} s")
    # (c) a validation pass changes no trainer state
    before = _trainer_state(r)
    stats = r.validate()
    after = _trainer_state(r)
    assert before[1] == after[1]
    assert sorted(before[0]) == sorted(after[0])
    for k, v in before[0].items():
        assert torch.equal(v, after[0][k]), k
    assert all(torch.equal(a, b) for a, b in zip(before[2][:2], after[2][:2])) and np.array_equal(before[2][2], after[2][2])
    ep2 = {k[5:]: v for k, v in vals[-1].items() if k.startswith("coco/")}
    _same_stats(stats, ep2)
    # (b) the epoch-2 stats == tools/test.py on epoch_2.pth at batch size 1, host and device evaluators
    ckpt = str(tmp_path / "w" / "epoch_2.pth")
    for extra in ([], ["--gpu-eval"]):
        out = tmp_path / f"test{len(extra)}.json"
        cmd = [sys.executable, os.path.join(ROOT, "tools", "test.py"), U.CFG_INCRE, ckpt, "--batch-size", "1", "--out", str(out)]
        p = subprocess.run(cmd + extra + _test_opts(tmp_path), capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        _same_stats(json.load(open(out))["stats"], ep2)
    json.dump(ep2, open(tmp_path / "world1.json", "w"))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_dist_test_world2_gloo_equals_world1(tmp_path):
    """tools/test.py --launcher pytorch at world 2 (gloo, both ranks on one GPU; 3 images: rank 1 predicts a padding duplicate)
    == the world-1 device evaluation, bit for bit"""
    from erd_amd.runner import save_checkpoint
    _val_set(tmp_path)
    tsd, ssd = U.f7_state_dicts()
    ckpt = tmp_path / "epoch_1.pth"
    save_checkpoint(str(ckpt), U.build_erd(tsd, ssd), with_teacher=False)
    test_py = os.path.join(ROOT, "tools", "test.py")
    w1 = subprocess.run([sys.executable, test_py, U.CFG_INCRE, str(ckpt), "--batch-size", "1", "--gpu-eval", "--out",
                         str(tmp_path / "w1.json")] + _test_opts(tmp_path), capture_output=True, text=True, timeout=600)
    assert w1.returncode == 0, w1.stderr[-3000:]
    env = dict(os.environ, ERD_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), test_py, U.CFG_INCRE, str(ckpt), "--launcher", "pytorch", "--batch-size", "1",
           "--out", str(tmp_path / "w2.json")] + _test_opts(tmp_path)
    w2 = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert w2.returncode == 0, (w2.stdout[-2000:], w2.stderr[-3000:])
    a, b = json.load(open(tmp_path / "w1.json")), json.load(open(tmp_path / "w2.json"))
    _same_stats(a["stats"], b["stats"])
    assert list(a["classwise"]) == list(b["classwise"]) and np.array_equal(
        np.array(list(a["classwise"].values())), np.array(list(b["classwise"].values())), equal_nan=True)
    assert b["stats"]["bbox_mAP"] >= 0.0 and w2.stdout.count("bbox_mAP ") == 1            # rank 0 prints, once
