"""GPU: the device COCO evaluator (CocoBBoxEvalGPU, erd_coco_eval) against the host restatement CocoBBoxEval -- precision and
recall bit for bit (np.array_equal) on seeded sets that cover crowd regions matched repeatedly, `ignore` flags, annotation areas
of exactly 32^2 / 96^2, tied scores, empty categories and images, pairs above 100 detections, zero-area and touching boxes, K = 1
and K = 80 with a reordered subset of cat_ids, and detections added from device tensors; one val2017-sized case prints its time."""
import multiprocessing as mp
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from coco_eval_util import make_dets, make_gt
from erd_amd.evaluation import CocoBBoxEval, CocoBBoxEvalGPU, coco_stats, split_map


def _fill(ev, dets, extra_img=None):
    for img_id, (b, s, l) in dets.items():
        ev.add_predictions(img_id, b, s, l)
    if extra_img is not None:                                    # an image id outside gt["images"]: never counted
        ev.add_predictions(extra_img, np.array([[1, 1, 50, 50]], np.float32), np.array([0.99], np.float32), np.array([0]))
    return ev


def _eq_nan(a, b):
    return list(a) == list(b) and np.array_equal(np.array(list(a.values())), np.array(list(b.values())), equal_nan=True)


def _same(host, dev):
    assert host.precision.shape == dev.precision.shape and host.recall.shape == dev.recall.shape
    assert np.array_equal(host.precision, dev.precision), np.argwhere(host.precision != dev.precision)[:5]
    assert np.array_equal(host.recall, dev.recall), np.argwhere(host.recall != dev.recall)[:5]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_device_eval_bit_equal_to_host(seed):
    rng = np.random.RandomState(seed)
    cat_ids = [3, 5, 8, 9, 11, 14]
    gt = make_gt(rng, 24, cat_ids, empty_cats=(9, 14), crowd_p=0.15, ignore_p=0.1)
    order = [11, 3, 14, 8, 5, 9]                                  # the dataset's class order, not sorted
    dets = make_dets(rng, gt, len(order), per_img=(0, 60), no_det_cats=(5, 14), big_pair=True, cat_ids=order)
    host = _fill(CocoBBoxEval(gt, cat_ids=order), dets, extra_img=5)
    dev = _fill(CocoBBoxEvalGPU(gt, cat_ids=order), dets, extra_img=5)
    stats_h, stats_d = host.evaluate(), dev.evaluate()
    _same(host, dev)
    assert stats_h == stats_d and _eq_nan(host.classwise(), dev.classwise())
    assert _eq_nan(split_map(host, order[:3]), split_map(dev, order[:3]))
    k5, k9, k14 = order.index(5), order.index(9), order.index(14)
    assert (dev.precision[:, :, k9] == -1).all() and (dev.precision[:, :, k14] == -1).all()      # no ground truth
    assert (dev.precision[:, :, k5, 0, 2] == 0).all() and (dev.recall[:, k5, 0, 2] == 0).all()   # ground truth, no detections
    assert any(a["iscrowd"] for a in gt["annotations"]) and any(a.get("ignore") for a in gt["annotations"])


def test_crowd_region_matched_repeatedly_and_area_bounds():
    """hand-made: three detections inside one crowd region (all ignored, not false positives), one true positive of area exactly
    32^2 (small AND medium), one of 96^2 (medium AND large), an `ignore` box, equal scores across images"""
    gt = dict(images=[dict(id=1), dict(id=2)], categories=[dict(id=7, name="x")], annotations=[
        dict(id=1, image_id=1, category_id=7, bbox=[0, 0, 200, 200], area=40000.0, iscrowd=1),
        dict(id=2, image_id=1, category_id=7, bbox=[300, 300, 32, 32], area=32.0 ** 2, iscrowd=0),
        dict(id=3, image_id=2, category_id=7, bbox=[10, 10, 96, 96], area=96.0 ** 2, iscrowd=0),
        dict(id=4, image_id=2, category_id=7, bbox=[200, 10, 50, 50], area=2500.0, iscrowd=0, ignore=1)])
    b = {1: np.array([[10, 10, 60, 60], [20, 20, 80, 80], [100, 100, 150, 150], [300, 300, 332, 332]], np.float32),
         2: np.array([[10, 10, 106, 106], [200, 10, 250, 60], [400, 400, 420, 420]], np.float32)}
    s = {1: np.array([0.9, 0.8, 0.8, 0.7], np.float32), 2: np.array([0.8, 0.7, 0.9], np.float32)}
    host, dev = CocoBBoxEval(gt), CocoBBoxEvalGPU(gt)
    for ev in (host, dev):
        for i in (1, 2):
            ev.add_predictions(i, b[i], s[i], np.zeros(len(s[i]), np.int64))
    host.evaluate(), dev.evaluate()
    _same(host, dev)
    assert dev.recall[0, 0, 0, 2] == 1.0 and dev.recall[0, 0, 1, 2] == 1.0 and dev.recall[0, 0, 3, 2] == 1.0


@pytest.mark.parametrize("K", [1, 80])
def test_device_eval_k1_and_k80(K):
    rng = np.random.RandomState(10 + K)
    all_ids = list(range(1, 91))
    cat_ids = list(rng.permutation(all_ids)[:K])                 # a reordered subset of the file's categories
    gt = make_gt(rng, 30, all_ids if K > 1 else cat_ids, gt_per_img=(0, 12))
    dets = make_dets(rng, gt, K, per_img=(0, 100), cat_ids=cat_ids)
    host = _fill(CocoBBoxEval(gt, cat_ids=cat_ids), dets)
    dev = _fill(CocoBBoxEvalGPU(gt, cat_ids=cat_ids), dets)
    assert host.evaluate() == dev.evaluate()
    _same(host, dev)


def test_device_add_equals_host_add():
    """predict's padded tensors straight into the evaluator (add_batch, no host synchronisation) == add_predictions of the
    same rows; padding rows past num are never read as detections"""
    rng = np.random.RandomState(4)
    cat_ids = [1, 2, 3, 4]
    gt = make_gt(rng, 12, cat_ids)
    dets = make_dets(rng, gt, 4, per_img=(0, 30), cat_ids=cat_ids)
    ids = [im["id"] for im in gt["images"]]
    P = 40
    a, b = CocoBBoxEvalGPU(gt), CocoBBoxEvalGPU(gt)
    _fill(a, dets)
    for b0 in range(0, len(ids), 5):
        chunk = ids[b0:b0 + 5]
        d = np.full((len(chunk), P, 5), 7.0, np.float32)         # garbage in the padding
        lab = np.full((len(chunk), P), 3, np.int64)
        num = np.zeros(len(chunk), np.int32)
        for n, i in enumerate(chunk):
            bb, sc, lb = dets[i]
            num[n] = len(sc)
            d[n, :len(sc), :4], d[n, :len(sc), 4], lab[n, :len(sc)] = bb, sc, lb
        b.add_batch(chunk, torch.from_numpy(d).cuda(), torch.from_numpy(lab).cuda(), torch.from_numpy(num).cuda())
    assert a.evaluate() == b.evaluate()
    _same(a, b)
    host = _fill(CocoBBoxEval(gt), dets)
    host.evaluate()
    _same(host, b)


def _host_one_category(args):
    gt, cat, k, dets = args
    ev = CocoBBoxEval(gt, cat_ids=[cat])
    for img_id, (b, s, l) in dets.items():
        m = l == k
        if m.any():
            ev.add_predictions(img_id, b[m], s[m], np.zeros(int(m.sum()), np.int64))
    ev.evaluate()
    return ev.precision[:, :, 0], ev.recall[:, 0]


def test_val2017_sized_timing():
    """5000 images x 100 detections, 80 categories, ~36k ground-truth boxes: prints the device evaluate() time (copy back
    included); the host reference is assembled per category (each category's arrays are independent) in worker processes"""
    rng = np.random.RandomState(2017)
    cat_ids = list(range(1, 81))
    gt = make_gt(rng, 5000, cat_ids, gt_per_img=(1, 13))
    dets = make_dets(rng, gt, 80, per_img=(100, 100), score_grid=1000, cat_ids=cat_ids)
    dev = _fill(CocoBBoxEvalGPU(gt), dets)
    torch.cuda.synchronize()
    dev.evaluate()                                               # warm: workspace allocation, code load
    t0 = time.perf_counter()
    stats = dev.evaluate()
    dt = time.perf_counter() - t0
    ctx = mp.get_context("fork")
    t1 = time.perf_counter()
    with ctx.Pool(8) as pool:
        parts = pool.map(_host_one_category, [(gt, c, k, dets) for k, c in enumerate(cat_ids)])
    th = time.perf_counter() - t1
    prec = np.stack([p for p, _ in parts], 2)
    rec = np.stack([r for _, r in parts], 1)
    print(f"\nval2017-sized: {len(gt['annotations'])} ground-truth boxes, device evaluate() {dt:.3f} s, "
          f"host reference {th:.1f} s over 8 processes")
    assert np.array_equal(prec, dev.precision) and np.array_equal(rec, dev.recall)
    assert coco_stats(prec, rec) == stats
