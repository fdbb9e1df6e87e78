"""COCO bbox validation of a live detector: what mmengine's ValLoop + CocoMetric do for `train_cfg.val_interval`, and the sharded
test of `tools/test.py --launcher pytorch`.

The test pipeline is tools/test.py's (GpuDetPipeline without flipping, detections rescaled to the original image); predict's
padded device outputs go straight into CocoBBoxEvalGPU.  At world > 1 each rank predicts the shard of mmengine's
DefaultSampler(shuffle=False, round_up=True) -- indices padded cyclically to a multiple of the world size, rank r takes r::world --
the padded outputs are gathered to every rank as fixed-shape tensors (RCCL on the device; gloo stages through host memory), the
padding duplicates are dropped, rank 0 evaluates on its GPU and broadcasts the stats.
"""
from __future__ import annotations

import json
import math
import os
from typing import Dict, List, Optional

import torch
import torch.distributed as dist


def val_due(epoch: int, max_epochs: int, val_begin: int = 1, val_interval: int = 1) -> bool:
    """mmengine EpochBasedTrainLoop: validate after (1-based) epoch `epoch`"""
    return epoch >= val_begin and (epoch % val_interval == 0 or epoch == max_epochs)


def shard_indices(n: int, rank: int, world: int) -> List[int]:
    """DefaultSampler(shuffle=False, round_up=True) of a dataset of n items at rank `rank` of `world`"""
    if n == 0:
        return []
    total = math.ceil(n / world) * world
    idx = (list(range(n)) * (total // n + 1))[:total]
    return idx[rank:total:world]


def gathered_order(n: int, world: int) -> List[int]:
    """dataset index of each row of the rank-major gathered shards read as (row j, rank r) pairs, j outer (mmengine's
    collect_results zips the ranks' parts); the first n rows are the dataset in order, the rest are the padding duplicates"""
    shards = [shard_indices(n, r, world) for r in range(world)]
    return [shards[r][j] for j in range(len(shards[0])) for r in range(world)]


def skip_reason(cfg, val_data: Optional[dict] = None) -> Optional[str]:
    """why a config gets no validation pass (None: it gets one)"""
    for key in ("val_cfg", "val_dataloader", "val_evaluator"):
        if cfg.get(key) is None:
            return f"{key} is None"
    dcfg = dict(cfg.val_dataloader.get("dataset") or {})
    dcfg.update(val_data or {})
    path = os.path.join(dcfg.get("data_root", ""), dcfg.get("ann_file", ""))
    ann = (cfg.val_evaluator or {}).get("ann_file") or path
    for f in {path, ann}:
        if not os.path.isfile(f):
            return f"annotation file {f} does not exist"
    return None


class CocoValidator:
    """One dataset + pipeline + evaluator description; run(detector) predicts this rank's shard and returns the stats (the same
    on every rank).  `dataset_cfg`: a `val_dataloader.dataset` / `test_dataloader.dataset` dict; `ann_file`: the evaluator's
    annotation file (default: the dataset's)."""

    def __init__(self, dataset_cfg: dict, batch_size: int = 1, num_workers: int = 0, ann_file: Optional[str] = None,
                 classwise: bool = False, old_classes: Optional[int] = None, device=None):
        from .datasets import CocoAnnotations, GpuDetPipeline
        root = dataset_cfg.get("data_root", "")
        self.gt = json.load(open(os.path.join(root, dataset_cfg["ann_file"])))
        self.eval_gt = self.gt if ann_file is None or os.path.abspath(ann_file) == os.path.abspath(
            os.path.join(root, dataset_cfg["ann_file"])) else json.load(open(ann_file))
        self.ann = CocoAnnotations(self.gt, (dataset_cfg.get("metainfo") or {}).get("classes"),
                                   data_prefix=os.path.join(root, (dataset_cfg.get("data_prefix") or {}).get("img", "")),
                                   test_mode=True)
        scale = next((t["scale"] for t in dataset_cfg.get("pipeline", []) if t.get("type") == "Resize"), (1333, 800))
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        self.pipe = GpuDetPipeline(self.ann, scale=tuple(scale), flip_prob=0.0, device=self.device)
        self.bs, self.workers = int(batch_size), int(num_workers)
        self.classwise, self.old_classes = bool(classwise), old_classes
        self.evaluator = None

    @classmethod
    def from_cfg(cls, cfg, val_data: Optional[dict] = None, device=None) -> "CocoValidator":
        dl, ev = cfg.val_dataloader, cfg.val_evaluator
        dcfg = dict(dl.dataset)
        dcfg.update(val_data or {})
        ori = cfg.model.get("ori_setting")
        return cls(dcfg, batch_size=int(dl.get("batch_size", 1)), num_workers=int(dl.get("num_workers", 0)),
                   ann_file=ev.get("ann_file"), classwise=bool(ev.get("classwise", False)),
                   old_classes=(ori.ori_num_classes if ori else None), device=device)

    def __len__(self):
        return len(self.ann)

    @torch.no_grad()
    def run(self, detector, max_images: Optional[int] = None) -> Dict[str, float]:
        """detector: a GFL-family model (its student half for ERD); evaluated in eval mode, its mode restored afterwards"""
        from .datasets import pinned, prefetch_map
        from .dist_utils import all_gather_stacked
        from .evaluation import CocoBBoxEvalGPU, split_map
        rank = dist.get_rank() if dist.is_initialized() else 0
        world = dist.get_world_size() if dist.is_initialized() else 1
        n = len(self.ann) if max_images is None else min(len(self.ann), max_images)
        mine = shard_indices(n, rank, world)
        head = detector.bbox_head
        P = int(head.test_cfg["max_per_img"])
        ev = CocoBBoxEvalGPU(self.eval_gt, cat_ids=self.ann.cat_ids, device=self.device) if rank == 0 else None
        if world > 1:
            dets = torch.zeros((len(mine), P, 5), dtype=torch.float32, device=self.device)
            labels = torch.zeros((len(mine), P), dtype=torch.int64, device=self.device)
            num = torch.zeros((len(mine),), dtype=torch.int32, device=self.device)
        was_training = detector.training
        detector.eval()
        try:
            batches = [mine[b0:b0 + self.bs] for b0 in range(0, len(mine), self.bs)]
            decode = lambda idx: (idx, [pinned(im) for im in self.pipe.decode(idx)])
            row = 0
            for idx, imgs in prefetch_map(decode, batches, self.workers, 2):
                x, samples = self.pipe.assemble(idx, imgs)
                cls, bbox, sizes = detector._forward_cat(x)
                metas = [s.metainfo for s in samples]
                if world == 1:
                    d, l, c = head.predict_padded_cat(cls, bbox, sizes, metas, rescale=True)
                    ev.add_batch([self.ann.get_data_info(i)["img_id"] for i in idx], d, l, c)
                else:
                    r1 = row + len(idx)
                    head.predict_padded_cat(cls, bbox, sizes, metas, rescale=True,
                                            out=(dets[row:r1], labels[row:r1], num[row:r1]))
                row += len(idx)
        finally:
            detector.train(was_training)
        if world > 1:
            g = [all_gather_stacked(t) for t in (dets, labels, num)]
            if rank == 0:
                order = gathered_order(n, world)[:n]                  # rows (j, r) -> dataset order; padding dropped
                d, l, c = (t.transpose(0, 1).reshape(-1, *t.shape[2:])[:n] for t in g)
                ev.add_batch([self.ann.get_data_info(i)["img_id"] for i in order], d.contiguous(), l.contiguous(),
                             c.contiguous())
        out = [None]
        if rank == 0:
            stats = dict(ev.evaluate())
            if self.old_classes:
                stats.update(split_map(ev, self.ann.cat_ids[:self.old_classes]))
            out = [dict(stats=stats, classwise=ev.classwise())]
            self.evaluator = ev
        if world > 1:
            dist.broadcast_object_list(out, src=0)
        self.last = out[0]
        return out[0]["stats"]

    def format(self, epoch: int, stats: Dict[str, float], n: Optional[int] = None) -> List[str]:
        """mmengine's log line of a validation pass (+ the class-wise table with classwise=True)"""
        n = len(self) if n is None else n
        keys = ["bbox_mAP", "bbox_mAP_50", "bbox_mAP_75", "bbox_mAP_s", "bbox_mAP_m", "bbox_mAP_l"]
        line = "Epoch(val) [%d][%d/%d]  %s" % (epoch, n, n, "  ".join(f"coco/{k}: {stats[k]:.4f}" for k in keys))
        extra = [k for k in ("old_mAP", "new_mAP") if k in stats]
        if extra:
            line += "  " + "  ".join(f"coco/{k}: {stats[k]:.4f}" for k in extra)
        lines = [line]
        if self.classwise:
            lines.append(f"{'category':24s} mAP")
            for name, v in self.last["classwise"].items():
                lines.append(f"{str(name):24s} {v:.4f}")
        return lines

