"""GPU: test-time augmentation -- erd_tta_merge against the reference's DetTTAModel (fixture F12, UNPINNED vs mmcv's NMS)
and the host restatement (tests/tta_util.py) on both sides of the kernel's LDS capacity; DetTTAModel on the 40+40 model
against every view run alone through mode="predict" and merged on the host; tools/test.py --tta end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tta_util as T
from e2e_util import CFG_INCRE, ROOT

F12 = os.path.join(ROOT, "tests", "golden", "f12_tta_merge_unpinned_nms.npz")
CFG_TTA = os.path.join(ROOT, "configs", "gfl_increment", "gfl_r50_fpn_1x_coco_first_40_incre_last_40_cats_tta.py")


def _merge_gpu(dets, labels, num, flips, ori_w, iou, mpi):
    from erd_amd import kernels as K
    d, l, n = K.tta_merge(torch.from_numpy(np.ascontiguousarray(dets)).cuda(), torch.from_numpy(labels).cuda(),
                          torch.from_numpy(num).cuda(), flips, ori_w, iou, mpi)
    d, l, n = d.cpu(), l.cpu(), n.cpu()
    assert d.shape == (len(ori_w), mpi, 5) and l.dtype == torch.int64
    return [(d[i, :n[i], :4], d[i, :n[i], 4], l[i, :n[i]]) for i in range(len(ori_w))], d, l, n


@pytest.mark.parametrize("case", range(len(T.F12_CASES)))
def test_tta_merge_vs_reference_fixture(case):
    g = np.load(F12)
    dets, labels, num, flips, ori_w, iou, mpi = T.f12_inputs(case)
    got, d, l, n = _merge_gpu(dets, labels, num, flips, ori_w, iou, mpi)
    for i, (b, s, lab) in enumerate(got):
        assert np.array_equal(b.numpy(), g[f"c{case}_i{i}_bboxes"]), (case, i)     # same set, same order, bit-equal boxes
        assert np.array_equal(s.numpy(), g[f"c{case}_i{i}_scores"]) and np.array_equal(lab.numpy(), g[f"c{case}_i{i}_labels"])
        assert (d[i, n[i]:] == 0).all() and (l[i, n[i]:] == 0).all()             # rows past the count stay zero


def _random_views(V, N, P, counts, seed, ties=False, n_labels=4):
    rng = np.random.RandomState(seed)
    W = rng.uniform(200, 900, N).astype(np.float32).round()
    H = rng.uniform(200, 900, N).astype(np.float32).round()
    dets = np.zeros((V, N, P, 5), np.float32)
    labels = np.zeros((V, N, P), np.int64)
    num = np.zeros((V, N), np.int32)
    for v in range(V):
        for n in range(N):
            m = counts[v][n]
            cx, cy = rng.uniform(0, W[n], m), rng.uniform(0, H[n], m)
            bw, bh = rng.uniform(4, 120, m), rng.uniform(4, 120, m)
            b = np.stack([np.clip(cx - bw / 2, 0, W[n]), np.clip(cy - bh / 2, 0, H[n]),
                          np.clip(cx + bw / 2, 0, W[n]), np.clip(cy + bh / 2, 0, H[n])], 1).astype(np.float32)
            s = (rng.randint(1, 8, m) / 8.0 if ties else rng.uniform(0, 1, m)).astype(np.float32)
            o = np.argsort(-s, kind="stable")
            dets[v, n, :m, :4], dets[v, n, :m, 4] = b[o], s[o]
            labels[v, n, :m] = rng.randint(0, n_labels, m)[o]
            num[v, n] = m
    flips = [bool(v % 2 == 0) for v in range(V)]
    return dets, labels, num, flips, [float(w) for w in W]


@pytest.mark.parametrize("V,P,per_image,mpi,ties", [
    (2, 1024, [2048, 1000, 0], 100, False),       # LDS path at its capacity; an image with no row at all
    (6, 342, [2049, 37, 0], 100, True),           # one past it: the global-workspace path; ties everywhere
    (6, 342, [2049, 2052, 1], 5000, False),       # max_per_img above every merged count
    (2, 60, [120, 0, 77], 3000, True),
])
def test_tta_merge_vs_restatement_random(V, P, per_image, mpi, ties):
    rng = np.random.RandomState(V * 1000 + P + mpi)
    counts = [[] for _ in range(V)]
    for n, k in enumerate(per_image):              # split each image's total over its views (each view <= P)
        left = k
        for v in range(V):
            m = min(P, left) if v == V - 1 else min(P, int(rng.randint(0, P + 1)), left)
            counts[v].append(m)
            left -= m
        if left:                                   # top the views up to P in view order
            for v in range(V):
                add = min(P - counts[v][n], left)
                counts[v][n] += add
                left -= add
        assert left == 0 and sum(counts[v][n] for v in range(V)) == k
    dets, labels, num, flips, ori_w = _random_views(V, len(per_image), P, counts, seed=V + P, ties=ties)
    got, _, _, n = _merge_gpu(dets, labels, num, flips, ori_w, 0.5, mpi)
    want = T.merge(dets, labels, num, flips, ori_w, 0.5, mpi)
    for i, ((gb, gs, gl), (wb, ws, wl)) in enumerate(zip(got, want)):
        assert torch.equal(gb, wb) and torch.equal(gs, ws) and torch.equal(gl, wl), (i, len(gb), len(wb))
    for i, k in enumerate(per_image):
        assert (int(n[i]) == 0) == (k == 0)


def _coco_dir(tmp_path, sizes, n_cat=80):
    from PIL import Image
    rng = np.random.RandomState(11)
    (tmp_path / "val").mkdir()
    images, anns = [], []
    for i, (h, w) in enumerate(sizes):
        arr = rng.randint(0, 256, (h, w, 3), dtype=np.uint8)
        arr[h // 4: h // 2, w // 5: w // 2] = rng.randint(0, 256, 3, dtype=np.uint8)     # a flat block: something to find
        Image.fromarray(arr).save(tmp_path / "val" / f"{i:04d}.png")
        images.append(dict(id=100 + i, file_name=f"{i:04d}.png", width=w, height=h))
        anns.append(dict(id=i + 1, image_id=100 + i, category_id=10 + 40 + i % 40, bbox=[w / 5, h / 4, w / 2 - w / 5, h / 4],
                         area=w * h / 40, iscrowd=0))
    ds = dict(images=images, annotations=anns, categories=[dict(id=10 + k, name=f"k{k}") for k in range(n_cat)])
    json.dump(ds, open(tmp_path / "val.json", "w"))
    return ds


def test_det_tta_model_equals_views_run_alone_and_merged_on_the_host(tmp_path):
    """2 images, scales (2000, 1200) and (666, 400) x flip 1 / 0: DetTTAModel (two forwards of 2N images, one merge launch)
    against each view through today's mode="predict" on its own and the restated merge on the host"""
    import e2e_util as U
    from erd_amd import MODELS
    from erd_amd.datasets import CocoAnnotations, GpuDetPipeline
    from test_gpu_predict import assert_same_detections
    ds = _coco_dir(tmp_path, [(123, 153), (100, 140)])
    ann = CocoAnnotations(str(tmp_path / "val.json"), None, data_prefix=str(tmp_path / "val"), test_mode=True)
    pipe = GpuDetPipeline(ann, flip_prob=0.0)
    tsd, ssd = U.f7_state_dicts()
    model = U.build_erd(tsd, ssd).eval()
    model.bbox_head.test_cfg = dict(model.bbox_head.test_cfg, score_thr=0.001)
    scales, flips = [(2000, 1200), (666, 400)], [True, False]
    imgs = pipe.decode([0, 1])
    views = pipe.assemble_tta([0, 1], imgs, scales, flips)
    assert len(views) == 4 and [v[1][0].metainfo["flip"] for v in views] == [True, False, True, False]
    assert views[0][0].data_ptr() + views[0][0].numel() * 4 == views[1][0].data_ptr()        # one 2N batch per scale
    assert views[0][1][0].metainfo["flip_direction"] == "horizontal" and views[1][1][0].metainfo["flip_direction"] is None
    P = int(model.bbox_head.test_cfg["max_per_img"])
    dets, labels, num = np.zeros((4, 2, P, 5), np.float32), np.zeros((4, 2, P), np.int64), np.zeros((4, 2), np.int32)
    for v, (x, samples) in enumerate(views):
        out = model(x.clone(), samples, mode="predict")
        for n, d in enumerate(out):
            p = d.pred_instances
            k = len(p.scores)
            dets[v, n, :k, :4], dets[v, n, :k, 4] = p.bboxes.cpu().numpy(), p.scores.cpu().numpy()
            labels[v, n, :k], num[v, n] = p.labels.cpu().numpy(), k
    assert num.min() > 0
    ori_w = [float(d["width"]) for d in ds["images"]]
    want = T.merge(dets, labels, num, flips * 2, ori_w, 0.5, 100)
    tta = MODELS.build(dict(type="DetTTAModel", module=model,
                            tta_cfg=dict(nms=dict(type="nms", iou_threshold=0.5), max_per_img=100)))
    got = tta(pipe.assemble_tta([0, 1], imgs, scales, flips), mode="predict")
    assert len(got) == 2
    for n, d in enumerate(got):
        p = d.pred_instances
        assert d.metainfo["img_id"] == 100 + n and d.metainfo["flip"] is True            # view 0's sample, as the reference
        assert len(p.scores) > 0 and p.labels.dtype == torch.int64
        assert_same_detections((p.bboxes, p.scores, p.labels), want[n])
        b = p.bboxes.cpu()
        im = ds["images"][n]
        assert (b >= -1e-3).all() and (b[:, 0::2] <= im["width"] + 1e-2).all() and (b[:, 1::2] <= im["height"] + 1e-2).all()


@pytest.mark.parametrize("config", [CFG_INCRE, CFG_TTA])
def test_test_py_tta_runs_on_real_files(tmp_path, config):
    """tools/test.py --tta: the flip-only defaults (a config without tta_model / tta_pipeline) and the 3-scale x 2-flip
    config, through the CLI on PNG files, with the class-wise table"""
    import e2e_util as U
    from erd_amd.runner import save_checkpoint
    ds = _coco_dir(tmp_path, [(120, 150), (140, 100), (100, 160)])
    tsd, ssd = U.f7_state_dicts()
    ckpt = tmp_path / "epoch_12.pth"
    save_checkpoint(str(ckpt), U.build_erd(tsd, ssd), with_teacher=False)
    cmd = [sys.executable, os.path.join(ROOT, "tools", "test.py"), config, str(ckpt), "--tta", "--batch-size", "2", "--out",
           str(tmp_path / "res.json"), "--cfg-options", f"test_dataloader.dataset.data_root={tmp_path}/",
           "test_dataloader.dataset.ann_file=val.json", "test_dataloader.dataset.data_prefix.img=val/",
           "model.test_cfg.score_thr=0.001", "test_evaluator.classwise=True"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "bbox_mAP" in out.stdout and "bbox_mAP_50" in out.stdout and "old_mAP" in out.stdout and "new_mAP" in out.stdout
    assert "k79" in out.stdout                                                   # the class-wise table
    assert ("Cannot find ``tta_pipeline``" in out.stderr) == (config == CFG_INCRE)
    res = json.load(open(tmp_path / "res.json"))
    assert res["results"] and len(res["classwise"]) == 80
    for r in res["results"]:                                                    # merged boxes in ORIGINAL image coordinates
        im = next(i for i in ds["images"] if i["id"] == r["image_id"])
        assert r["bbox"][0] >= -1e-3 and r["bbox"][0] + r["bbox"][2] <= im["width"] + 1e-2
        assert r["bbox"][1] >= -1e-3 and r["bbox"][1] + r["bbox"][3] <= im["height"] + 1e-2
