#!/usr/bin/env python3
"""Writes tests/golden/f12_tta_merge_unpinned_nms.npz: the reference's own DetTTAModel._merge_single_sample
(mmdet/models/test_time_augs/det_tta.py, imported in place through oracle/ref_stub.py) on the seeded view outputs of
tests/tta_util.py.  mmcv's batched_nms is ref_stub's restatement, so the fixture is UNPINNED vs mmcv (as F5 / F8).
Build container only (it needs the reference tree):

    python tools/gen_tta_golden.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_stub  # noqa: E402
import tta_util as T  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "f12_tta_merge_unpinned_nms.npz")


class BaseTTAModel(nn.Module):
    """mmengine.model.BaseTTAModel stand-in: holds the wrapped module (the merge never calls it)"""

    def __init__(self, module=None, data_preprocessor=None):
        super().__init__()
        self.module = module


class Pred(ref_stub.InstanceData):
    def get(self, k, default=None):
        return getattr(self, k) if k in self else default


def load_det_tta():
    ref_stub.load_reference()
    sys.modules["mmengine.model"].BaseTTAModel = BaseTTAModel
    return ref_stub._load("mmdet.models.test_time_augs.det_tta", "mmdet/models/test_time_augs/det_tta.py")


def main():
    det_tta = load_det_tta()
    out = {}
    for case in range(len(T.F12_CASES)):
        dets, labels, num, flips, ori_w, iou, mpi = T.f12_inputs(case)
        model = det_tta.DetTTAModel(tta_cfg=ref_stub.ConfigDict(nms=dict(type="nms", iou_threshold=iou), max_per_img=mpi))
        metas = T.f12_metas(case)
        out[f"c{case}_dets"], out[f"c{case}_labels"], out[f"c{case}_num"] = dets, labels, num
        out[f"c{case}_flips"], out[f"c{case}_ori_w"] = np.array(flips, np.int32), np.array(ori_w, np.float32)
        out[f"c{case}_iou_max"] = np.array([iou, mpi], np.float64)
        for n in range(len(ori_w)):
            samples = []
            for v in range(len(flips)):
                d = ref_stub.DetDataSample(metainfo=metas[v][n])
                m = int(num[v, n])
                d.pred_instances = Pred(bboxes=torch.from_numpy(dets[v, n, :m, :4].copy()),
                                        scores=torch.from_numpy(dets[v, n, :m, 4].copy()),
                                        labels=torch.from_numpy(labels[v, n, :m].copy()))
                samples.append(d)
            r = model._merge_single_sample(samples).pred_instances
            out[f"c{case}_i{n}_bboxes"] = r.bboxes.numpy()
            out[f"c{case}_i{n}_scores"] = r.scores.numpy()
            out[f"c{case}_i{n}_labels"] = r.labels.numpy()
            print(f"case {case} image {n}: {sum(int(num[v, n]) for v in range(len(flips)))} merged -> {len(r.scores)} kept")
    np.savez_compressed(OUT, **out)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
