"""No GPU: the index maths of sharded evaluation against mmengine's DefaultSampler(shuffle=False, round_up=True) and its
collect_results order, the validation schedule (val_begin, val_interval, last epoch), the conditions that skip validation, and the
prefix property the device evaluator rests on -- CocoBBoxEval's matchings for maxDet 1 and 10 are prefixes of the maxDet-100 one."""
import json
import math

import numpy as np
import pytest

from coco_eval_util import make_dets, make_gt
from erd_amd.evaluation import AREA_RNG, IOU_THRS, CocoBBoxEval
from erd_amd.validation import gathered_order, shard_indices, skip_reason, val_due


def _default_sampler(n, rank, world):
    """mmengine/dataset/sampler.py DefaultSampler.__iter__ with shuffle=False, round_up=True, restated"""
    num_samples = math.ceil(n / world)
    total = num_samples * world
    indices = list(range(n))
    indices = (indices * int(total / len(indices) + 1))[:total]
    return indices[rank:total:world]


@pytest.mark.parametrize("n,world", [(7, 2), (10, 4), (9, 3), (2, 4), (1, 8), (5, 1)])
def test_shards_follow_default_sampler(n, world):
    shards = [shard_indices(n, r, world) for r in range(world)]
    assert shards == [_default_sampler(n, r, world) for r in range(world)]
    assert len({len(s) for s in shards}) == 1                                   # fixed shapes to gather
    order = gathered_order(n, world)
    # collect_results: zip the ranks' parts, then drop what is past the dataset's size
    zipped = [x for part in zip(*shards) for x in part]
    assert order == zipped and order[:n] == list(range(n))
    assert set(order[n:]) <= set(range(n)) and len(order) - n == len(shards[0]) * world - n


@pytest.mark.parametrize("begin,interval,max_epochs,want", [
    (1, 1, 3, [1, 2, 3]), (1, 2, 5, [2, 4, 5]), (3, 1, 4, [3, 4]), (2, 3, 7, [3, 6, 7]), (1, 12, 12, [12]),
    (5, 2, 4, [])])
def test_validation_schedule(begin, interval, max_epochs, want):
    assert [e for e in range(1, max_epochs + 1) if val_due(e, max_epochs, begin, interval)] == want


def test_validation_skip_conditions(tmp_path):
    from erd_amd import Config
    ann = tmp_path / "val.json"
    cfg = Config(dict(val_cfg=dict(type="ValLoop"), val_evaluator=dict(type="CocoMetric", ann_file=str(ann)),
                      val_dataloader=dict(batch_size=1, dataset=dict(data_root=f"{tmp_path}/", ann_file="val.json"))))
    assert "does not exist" in skip_reason(cfg)
    ann.write_text(json.dumps(dict(images=[], annotations=[], categories=[])))
    assert skip_reason(cfg) is None
    assert "does not exist" in skip_reason(cfg, dict(ann_file="other.json"))     # a handed-in dataset replaces the config's
    for key in ("val_cfg", "val_dataloader", "val_evaluator"):
        c = Config(dict(cfg))
        c[key] = None
        assert skip_reason(c) == f"{key} is None"
    c = Config(dict(cfg))
    c.val_evaluator = dict(type="CocoMetric", ann_file=str(tmp_path / "missing.json"))
    assert "missing.json" in skip_reason(c)


def _matching(ev, img, cat, rng, max_det):
    e = ev._evaluate_img(img, cat, rng, max_det)
    return None if e is None else (e["dtm"], e["dt_ig"], e["scores"], e["n_gt"])


def test_maxdet_matchings_are_prefixes_of_the_maxdet_100_matching():
    rng = np.random.RandomState(11)
    cat_ids = [1, 2, 3]
    gt = make_gt(rng, 12, cat_ids, crowd_p=0.2, ignore_p=0.15)
    ev = CocoBBoxEval(gt)
    for img_id, (b, s, l) in make_dets(rng, gt, 3, per_img=(20, 120), big_pair=True, cat_ids=cat_ids).items():
        ev.add_predictions(img_id, b, s, l)
    checked = 0
    for img in ev.img_ids:
        for cat in cat_ids:
            for r in AREA_RNG.values():
                full = _matching(ev, img, cat, r, 100)
                if full is None:
                    continue
                for md in (1, 10):
                    part = _matching(ev, img, cat, r, md)
                    k = part[0].shape[1]
                    assert k == min(md, full[0].shape[1])
                    assert np.array_equal(part[0], full[0][:, :k]) and np.array_equal(part[1], full[1][:, :k])
                    assert np.array_equal(part[2], full[2][:k]) and part[3] == full[3]
                    checked += 1
    assert checked > 100
    assert full[0].shape[0] == len(IOU_THRS)
