"""Thin training launcher around ERDTrainer: what ``tools/train.py`` -> mmengine ``Runner``
does for this path and nothing more -- config -> model, epoch loop, LinearLR warm-up + MultiStepLR, 50-iteration
logging, per-epoch checkpoints in the reference's file format, resume.

Reference: tools/train.py:15-129, configs/_base_/schedules/schedule_1x.py:2-28, configs/_base_/default_runtime.py:3-24,
detectors/gfl_increment_erd.py:67-122 (checkpoint keys).
"""
from __future__ import annotations

import bisect
import json
import os
import math
import time
from collections import OrderedDict, deque
from typing import Callable, Dict, Iterable, List, Optional

import numpy as np
import torch
import torch.distributed as dist

from .config import Config
from .engine import ERDTrainer
from .optim_cfg import check_custom_hooks, check_optimizer
from .registry import MODELS
from .structures import DetDataSample, InstanceData
from .validation import val_due


# ---------------------------------------------------------------------------------------------------------
# checkpoints: {'meta': ..., 'state_dict': OIHW fp32 tensors keyed as the reference's, 'optimizer': torch-SGD (or AdamW / Adam) layout}
# ---------------------------------------------------------------------------------------------------------
def model_state_dict(model: torch.nn.Module, with_teacher: bool = True) -> "OrderedDict[str, torch.Tensor]":
    """CPU copy of the state dict in the reference's layout (dense OIHW).  ``with_teacher=False`` drops the frozen
    ``ori_model.*`` copy (it is re-read from ``ori_setting.ori_checkpoint_file`` at build time anyway)."""
    out = OrderedDict()
    for k, v in model.state_dict().items():
        if not with_teacher and k.startswith("ori_model."):
            continue
        out[k] = v.detach().to("cpu").contiguous(memory_format=torch.contiguous_format).clone()
    return out


def save_checkpoint(path: str, model: torch.nn.Module, trainer: Optional[ERDTrainer] = None, meta: Optional[dict] = None,
                    with_teacher: bool = True) -> None:
    if trainer is not None:
        trainer.flush()        # the SGD update of the last step is deferred behind the next teacher forward: apply it
                               # BEFORE the weights are read, or the file pairs stale weights with newer momentum
    ckpt = dict(meta=dict(meta or {}), state_dict=model_state_dict(model, with_teacher))
    if trainer is not None and trainer.ema is not None:
        # the way mmengine's EMAHook leaves a checkpoint: `state_dict` holds the AVERAGED weights (tools/test.py and the next
        # phase's ori_checkpoint_file read the average as they stand), `ema_state_dict` the count and the raw training weights
        # under `module.<key>` for every key outside the teacher copy.  Written from device copies: the live model is not swapped
        host = lambda t: t.to("cpu").contiguous(memory_format=torch.contiguous_format)
        st = trainer.ema_state()
        missing = [k for k in st["tensors"] if k not in ckpt["state_dict"]]
        if missing:
            raise KeyError(f"averaged tensors without a state_dict key of their name: {missing[:4]}")
        ema_sd = OrderedDict(steps=torch.tensor(st["steps"], dtype=torch.long))
        for k, v in ckpt["state_dict"].items():
            if not k.startswith("ori_model."):
                ema_sd["module." + k] = host(st["tensors"][k][0]) if k in st["tensors"] else v.clone()
        for k, (_, avg) in st["tensors"].items():
            ckpt["state_dict"][k] = host(avg)
        ckpt["ema_state_dict"] = ema_sd
    if trainer is not None:
        ckpt["optimizer"] = trainer.optimizer_state_dict()
        ckpt["meta"].update(iter=trainer.iter)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tmp = path + ".tmp"
    torch.save(ckpt, tmp)
    os.replace(tmp, path)


def load_checkpoint(path: str, model: torch.nn.Module, trainer: Optional[ERDTrainer] = None, strict: bool = True,
                    log: Optional[Callable[[str], None]] = None) -> dict:
    """trainer given: a RESUME -- optimizer state and iteration are restored, and a checkpoint written under an EMAHook is
    exchanged back (the model gets `ema_state_dict`'s raw weights, the trainer's average `state_dict`'s, `steps` is restored).
    Without a trainer `state_dict` is loaded as it stands (under an EMAHook: the average)."""
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    sd = ckpt["state_dict"] if "state_dict" in ckpt else ckpt
    if sd and next(iter(sd)).startswith("module."):
        sd = OrderedDict((k[7:], v) for k, v in sd.items())
    ema_sd = ckpt.get("ema_state_dict") if "state_dict" in ckpt else None
    averaged = None
    if trainer is not None and ema_sd is not None:
        raw = OrderedDict((k[7:], v) for k, v in ema_sd.items() if k.startswith("module."))
        averaged = {k: sd[k] for k in raw if k in sd}
        sd = OrderedDict(sd)
        sd.update(raw)
        if trainer.ema is None and log is not None:      # never train on the average silently
            log(f"{path} holds ema_state_dict and the config has no EMAHook: the raw weights were restored, the average was dropped")
    own = model.state_dict()
    if not any(k.startswith("ori_model.") for k in sd):      # saved without the teacher copy: keep ours
        sd = OrderedDict(sd)
        for k, v in own.items():
            if k.startswith("ori_model."):
                sd[k] = v
    model.load_state_dict(sd, strict=strict)
    if trainer is not None and "optimizer" in ckpt:
        trainer.load_optimizer_state_dict(ckpt["optimizer"])
        trainer.iter = int(ckpt.get("meta", {}).get("iter", 0))
    if trainer is not None and trainer.ema is not None:
        if ema_sd is not None:
            trainer.load_ema_state(int(ema_sd["steps"]), averaged)
        else:
            trainer.load_ema_state(0, None)
            if log is not None:
                log(f"{path} holds no ema_state_dict: the average starts as a copy of the loaded weights")
    return ckpt.get("meta", {})


# ---------------------------------------------------------------------------------------------------------
# schedule (schedule_1x.py:7-17)
# ---------------------------------------------------------------------------------------------------------
class ParamSchedule:
    """LinearLR (by iteration) x MultiStepLR (by epoch), composed multiplicatively as mmengine's scheduler list."""

    def __init__(self, param_scheduler: Iterable[dict]):
        self.linear, self.multistep = None, None
        for s in param_scheduler or []:
            s = dict(s)
            t = s.pop("type")
            if t == "LinearLR":
                if s.get("by_epoch", True):
                    raise NotImplementedError("LinearLR by_epoch=True is not used by the ERD configs")
                self.linear = (float(s.get("start_factor", 1 / 3)), float(s.get("end_factor", 1.0)),
                               int(s.get("begin", 0)), int(s["end"]))
            elif t == "MultiStepLR":
                self.multistep = (sorted(int(m) for m in s["milestones"]), float(s.get("gamma", 0.1)))
            else:
                raise NotImplementedError(f"param scheduler {t}")

    def iter_factor(self, it: int) -> float:
        if self.linear is None:
            return 1.0
        s0, s1, b, e = self.linear
        if it >= e:
            return s1
        # mmengine/torch LinearLR: factor interpolates over (end - begin - 1) steps
        return s0 + (s1 - s0) * max(it - b, 0) / max(e - b - 1, 1)

    def epoch_factor(self, epoch: int) -> float:
        if self.multistep is None:
            return 1.0
        ms, gamma = self.multistep
        return gamma ** bisect.bisect_right(ms, epoch)


# ---------------------------------------------------------------------------------------------------------
# data: synthetic batches of the reference's demo_mm_inputs shape (mmdet/testing/_utils.py:89-202)
# ---------------------------------------------------------------------------------------------------------
class SyntheticDetData:
    """``iters_per_epoch`` batches of uint8 images + 1..9 random boxes each; deterministic per (seed, epoch, index)."""

    def __init__(self, batch_size: int, num_classes: int, iters_per_epoch: int, image_hw=(800, 1333), seed: int = 0):
        self.bs, self.nc, self.n, self.hw, self.seed = batch_size, num_classes, iters_per_epoch, tuple(image_hw), seed
        self.epoch = 0

    def set_epoch(self, epoch: int) -> None:
        self.epoch = epoch

    def __len__(self):
        return self.n

    def __iter__(self):
        H, W = self.hw
        for i in range(self.n):
            rng = np.random.RandomState((self.seed * 1000003 + self.epoch * 10007 + i) % (2 ** 31 - 1))
            imgs, samples = [], []
            for _ in range(self.bs):
                imgs.append(torch.from_numpy(rng.randint(0, 255, size=(3, H, W), dtype=np.uint8)))
                nb = rng.randint(1, 10)
                cx, cy, bw, bh = rng.rand(nb, 4).T
                boxes = np.vstack([(cx * W - W * bw / 2).clip(0, W), (cy * H - H * bh / 2).clip(0, H),
                                   (cx * W + W * bw / 2).clip(0, W), (cy * H + H * bh / 2).clip(0, H)]).T
                ds = DetDataSample(metainfo=dict(scale_factor=(1.0, 1.0), ori_shape=(H, W)))
                ds.gt_instances = InstanceData(bboxes=torch.from_numpy(boxes.astype(np.float32)),
                                               labels=torch.from_numpy(rng.randint(0, self.nc, size=nb).astype(np.int64)))
                samples.append(ds)
            yield dict(inputs=imgs, data_samples=samples)


class CocoTrainData:
    """The real-data source of `train_dataloader` (configs/_base_/datasets/coco_detection.py:37-50): CocoDataset
    annotations restricted to `metainfo.classes`, DefaultSampler(shuffle=True) sharded over ranks, AspectRatioBatchSampler,
    and the GPU image pipeline.  Batches arrive normalised and padded (`preprocessed=True`)."""

    def __init__(self, dataset_cfg: dict, batch_size: int, classes=None, scale=(1333, 800), seed: int = 0, rank: int = 0,
                 world: int = 1, device="cuda", num_workers: int = 0, prefetch_factor: int = 2, flip_prob: float = 0.5,
                 scale_sampler=None):
        """num_workers / prefetch_factor: `train_dataloader.num_workers` decoding threads working `prefetch_factor`
        batches ahead of the training step (0 = decode in the training thread); flip_prob / scale_sampler: the RandomFlip
        and the resize stage of the pipeline (datasets.resolve_train_pipeline; None = the fixed `scale`)"""
        from .datasets import AspectRatioBatchSampler, CocoAnnotations, GpuDetPipeline
        self.num_workers, self.prefetch_factor = int(num_workers), int(prefetch_factor)
        root = dataset_cfg.get("data_root", "")
        classes = classes or (dataset_cfg.get("metainfo") or {}).get("classes")     # None: every category of the file
        fc = dataset_cfg.get("filter_cfg") or {}
        self.ann = CocoAnnotations(os.path.join(root, dataset_cfg["ann_file"]), classes,
                                   data_prefix=os.path.join(root, (dataset_cfg.get("data_prefix") or {}).get("img", "")),
                                   filter_empty_gt=fc.get("filter_empty_gt", True), min_size=fc.get("min_size", 32))
        self.pipe = GpuDetPipeline(self.ann, scale=scale, flip_prob=flip_prob, seed=seed, device=device, scale_sampler=scale_sampler)
        self.bs, self.seed, self.rank, self.world, self.epoch = batch_size, seed, rank, world, 0
        self._sampler_cls = AspectRatioBatchSampler

    @classmethod
    def from_cfg(cls, cfg, rank: int = 0, world: int = 1, seed: int = 0, device="cuda") -> "CocoTrainData":
        """the config's `train_dataloader`: batch size, decoding threads and the dataset's pipeline, READ by
        datasets.resolve_train_pipeline (a transform this path does not perform raises there instead of being skipped)"""
        from .datasets import resolve_train_pipeline
        dl = cfg["train_dataloader"]
        dcfg = dl["dataset"]
        if dcfg.get("pipeline") is None:
            raise ValueError("train_dataloader.dataset has no pipeline")
        pl = resolve_train_pipeline(dcfg["pipeline"])
        fixed = pl["sampler"].type == "Resize"
        return cls(dcfg, int(dl["batch_size"]), scale=pl["sampler"].scale if fixed else (1333, 800), seed=seed, rank=rank,
                   world=world, device=device, num_workers=int(dl.get("num_workers", 0)),
                   prefetch_factor=int(dl.get("prefetch_factor") or 2), flip_prob=pl["flip_prob"],
                   scale_sampler=None if fixed else pl["sampler"])

    def set_epoch(self, epoch: int) -> None:
        self.epoch = epoch
        self.pipe.set_epoch(epoch)

    def _indices(self) -> List[int]:
        g = torch.Generator()
        g.manual_seed(self.seed + self.epoch)                    # DefaultSampler: randperm per epoch, same on every rank
        perm = torch.randperm(len(self.ann), generator=g).tolist()
        total = -(-len(perm) // self.world) * self.world          # padded so that every rank sees the same count
        perm = (perm * (total // max(len(perm), 1) + 1))[:total]
        return perm[self.rank::self.world]

    def __len__(self):
        return -(-len(self._indices()) // self.bs)

    def __iter__(self):
        from .datasets import prefetch_map
        batches = list(self._sampler_cls(self._indices(), self.ann, self.bs))
        epoch = self.epoch                                        # the draws of a batch decoded ahead belong to ITS epoch
        decode = lambda idx: (idx, self.pipe.pack(idx, epoch=epoch))       # one page-locked buffer per batch: pixels + records
        for idx, packed in prefetch_map(decode, batches, self.num_workers, self.prefetch_factor):
            x, samples = self.pipe.assemble(idx, packed)
            yield dict(inputs=x, data_samples=samples, preprocessed=True)


# ---------------------------------------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------------------------------------
def _with_next(it, prepare):
    """(item, following item or None) pairs of an iterable, every item passed through `prepare` exactly once"""
    it = iter(it)
    try:
        cur = prepare(next(it))
    except StopIteration:
        return
    for raw in it:
        nxt = prepare(raw)
        yield cur, nxt
        cur = nxt
    yield cur, None


class Runner:
    def __init__(self, cfg: Config, data=None, device: Optional[torch.device] = None, log: Callable[[str], None] = print,
                 val_data: Optional[dict] = None):
        """data: the training batches; val_data: keys that replace the config's `val_dataloader.dataset` ones (ann_file,
        data_root, data_prefix, ...)"""
        self.cfg = cfg
        self.rank = dist.get_rank() if dist.is_initialized() else 0
        self.world = dist.get_world_size() if dist.is_initialized() else 1
        self.log = log if self.rank == 0 else (lambda *_: None)
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        self.work_dir = cfg.get("work_dir") or os.path.join("work_dirs", "erd")
        model = MODELS.build(cfg.model)
        if not (cfg.get("load_from") or cfg.get("resume")):
            model.init_weights()      # backbone.init_cfg 'Pretrained' (a loaded checkpoint supersedes it); raises when unresolvable
        self.model = model.to(self.device).train()
        opt = cfg.optim_wrapper.optimizer
        checked = check_optimizer(opt)       # SGD, AdamW or Adam; anything else raises
        if cfg.optim_wrapper.get("type", "OptimWrapper") != "OptimWrapper":
            raise NotImplementedError("AMP is not built: the path computes in fp32")
        bs = int(cfg.train_dataloader.batch_size)
        self.schedule = ParamSchedule(cfg.get("param_scheduler"))
        asl = cfg.get("auto_scale_lr") or {}
        # the wrapper's own keys (mmengine OptimWrapper / DefaultOptimWrapperConstructor); passed on only when the config sets them
        ow = cfg.optim_wrapper
        extra = {k: (ow[k].to_dict() if hasattr(ow[k], "to_dict") else ow[k])
                 for k in ("paramwise_cfg", "clip_grad", "accumulative_counts") if ow.get(k) is not None}
        if checked["type"] != "SGD":
            extra["optimizer"] = checked
        # custom_hooks: EMAHook is the one hook built, anything else raises (optim_cfg.check_custom_hooks); none: nothing changes
        self.ema = check_custom_hooks(cfg.get("custom_hooks"))
        if self.ema is not None:
            extra["ema"] = self.ema
        self.trainer = ERDTrainer(self.model, lr=opt.lr if checked["type"] == "SGD" else checked["lr"], momentum=opt.get("momentum", 0.0),
                                  weight_decay=opt.get("weight_decay", 0.0),
                                  base_batch_size=asl.get("base_batch_size", 16), batch_size_per_gpu=bs,
                                  auto_scale_lr=bool(asl.get("enable", False)), warmup_iters=0, **extra)
        self.trainer.lr_factor = self.schedule.iter_factor          # warm-up comes from the config's LinearLR
        # data parallel: CUs the whole-chip grids leave to RCCL's resident kernels.  The launcher does not PROBE (ERDTrainer.
        # tune_cu_reserve spends optimisation steps on one batch: bench.py does that and prints `collectives.cu_reserve`); it takes
        # the value from ERD_CU_RESERVE, the same on every rank (tools/dist_train.sh passes the environment on)
        if self.trainer.world > 1 and os.environ.get("ERD_CU_RESERVE"):
            from . import kernels as _K
            _K.set_cu_reserve(int(os.environ["ERD_CU_RESERVE"]))
            self.trainer.cu_reserve = int(os.environ["ERD_CU_RESERVE"])
        self.max_epochs = int(cfg.train_cfg.max_epochs)
        hooks = cfg.get("default_hooks") or {}
        self.log_interval = int((hooks.get("logger") or {}).get("interval", 50))
        self.ckpt_interval = int((hooks.get("checkpoint") or {}).get("interval", 1))
        self.data = data
        self.epoch = 0
        self.history: List[Dict[str, float]] = []
        # validation after each epoch (mmengine ValLoop): train_cfg.val_begin / val_interval, val_dataloader, val_evaluator
        from .validation import CocoValidator, skip_reason
        self.val_begin = int(cfg.train_cfg.get("val_begin", 1))
        self.val_interval = int(cfg.train_cfg.get("val_interval", 1))
        why = skip_reason(cfg, val_data)
        self.validator = None if why else CocoValidator.from_cfg(cfg, val_data, device=self.device)
        if why:
            self.log(f"validation skipped: {why}")
        load_from, resume = cfg.get("load_from"), bool(cfg.get("resume", False))
        if resume and not load_from:
            last = os.path.join(self.work_dir, "last_checkpoint")
            if os.path.isfile(last):
                load_from = open(last).read().strip()
        if load_from:
            meta = load_checkpoint(load_from, self.model, self.trainer if resume else None, log=self.log)
            if resume:
                self.epoch = int(meta.get("epoch", 0))
            elif self.ema is not None:
                self.trainer.load_ema_state(0, None)          # the average starts as a copy of what was loaded
            self.log(f"{'resumed' if resume else 'loaded'} {load_from} (epoch {self.epoch}, iter {self.trainer.iter})")

    @classmethod
    def from_cfg(cls, cfg: Config, **kw) -> "Runner":
        return cls(cfg, **kw)

    def train(self, max_iters: Optional[int] = None) -> List[Dict[str, float]]:
        pre = self.model.data_preprocessor
        if pre is None:
            raise ValueError("the config has no data_preprocessor")
        window: deque = deque(maxlen=self.log_interval)
        done = 0
        while self.epoch < self.max_epochs:
            if hasattr(self.data, "set_epoch"):
                self.data.set_epoch(self.epoch)
            self.trainer.epoch_factor = self.schedule.epoch_factor(self.epoch)
            self.trainer.epoch = self.epoch                   # (EMAHook begin_epoch)
            t0 = time.perf_counter()
            for i, (out, nxt) in enumerate(_with_next(self.data, lambda b: b if b.get("preprocessed") else pre(b, True))):
                # one batch of look-ahead: the trainer queues the frozen teacher's half of the following step next to this
                # step's backward pass (ERDTrainer.train_step)
                logv = self.trainer.train_step(out["inputs"], out["data_samples"],
                                               next_batch=None if nxt is None else (nxt["inputs"], nxt["data_samples"]))
                window.append(logv)
                done += 1
                if (i + 1) % self.log_interval == 0 or (max_iters and done >= max_iters):
                    if self.trainer.clip is not None:
                        self.trainer.flush(close_window=False)    # the last step's update writes its grad_norm: queue it now
                    torch.cuda.synchronize()
                    keys = [k for k in window[0] if "loss" in k]
                    avg = {k: float(sum(float(w[k].detach()) for w in window) / len(window)) for k in keys}
                    # the reference's CheckInvalidLossHook (mmdet/engine/hooks/checkloss_hook.py:11-42: `isfinite(loss)`
                    # every `interval` iterations) rides on the logging read-back -- the values are on the host already
                    bad = [k for k, v in avg.items() if not math.isfinite(v)]
                    if bad:
                        raise FloatingPointError(f"loss became infinite or NaN! ({', '.join(bad)} at epoch {self.epoch + 1}, "
                                                 f"iteration {i + 1})")
                    # clip_grad: the norm of the (mean) gradient before clipping, averaged over the updates of the window
                    norms = [float(w["grad_norm"]) for w in window if "grad_norm" in w]
                    if norms:
                        avg["grad_norm"] = sum(norms) / len(norms)
                        if self.trainer.clip["error_if_nonfinite"] and not math.isfinite(avg["grad_norm"]):
                            raise FloatingPointError(f"the gradient norm became infinite or NaN (epoch {self.epoch + 1}, "
                                                     f"iteration {i + 1}; clip_grad.error_if_nonfinite)")
                    dt = (time.perf_counter() - t0) / (i + 1)
                    rec = dict(epoch=self.epoch + 1, iter=i + 1, lr=self.trainer.last_lr, time=dt, **avg)
                    self.history.append(rec)
                    self.log("Epoch(train) [%d][%d/%d]  lr: %.4e  time: %.3f  %s" % (
                        self.epoch + 1, i + 1, len(self.data), rec["lr"], dt,
                        "  ".join(f"{k}: {v:.4f}" for k, v in avg.items())))
                if max_iters and done >= max_iters:
                    self.trainer.flush()
                    return self.history
            if self.trainer.accum > 1:
                self.trainer.flush()      # an accumulation window never spans an epoch end
            self.epoch += 1
            if self.rank == 0 and self.ckpt_interval > 0 and self.epoch % self.ckpt_interval == 0:
                path = os.path.join(self.work_dir, f"epoch_{self.epoch}.pth")
                save_checkpoint(path, self.model, self.trainer, meta=dict(epoch=self.epoch))
                with open(os.path.join(self.work_dir, "last_checkpoint"), "w") as f:
                    f.write(path)
                self.log(f"saved {path}")
            if self.validator is not None and val_due(self.epoch, self.max_epochs, self.val_begin, self.val_interval):
                self.validate()
        self.trainer.flush()
        self._write_scalars()
        return self.history

    def validate(self) -> Dict[str, float]:
        """one validation pass of the live student on the weights after the epoch's last update (those epoch_{e}.pth holds):
        the deferred update is applied and every stream drained first; the pass reads the trainer's state and changes none of it.
        Under an EMAHook parameters and average are exchanged around the pass: it scores the averaged weights, training goes on
        with the raw ones"""
        if self.validator is None:
            raise RuntimeError("this runner has no validation (val_cfg / val_dataloader / val_evaluator or its file is missing)")
        self.trainer.flush()
        if self.ema is not None:
            self.trainer.swap_ema()
        try:
            torch.cuda.synchronize(self.device)               # teacher look-ahead stream, per-bucket update stream
            t0 = time.perf_counter()
            stats = self.validator.run(self.model)
            torch.cuda.synchronize(self.device)
        finally:
            if self.ema is not None:
                self.trainer.swap_ema()
        for line in self.validator.format(self.epoch, stats):
            self.log(line)
        rec = dict(mode="val", epoch=self.epoch, time=time.perf_counter() - t0, **{f"coco/{k}": v for k, v in stats.items()})
        self.history.append(rec)
        return stats

    def _write_scalars(self) -> None:
        if self.rank == 0:
            os.makedirs(self.work_dir, exist_ok=True)
            with open(os.path.join(self.work_dir, "scalars.json"), "w") as f:
                for rec in self.history:
                    f.write(json.dumps(rec) + "\n")
