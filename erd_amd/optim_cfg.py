"""The `optim_wrapper` options beside the optimizer itself, resolved on the host: `paramwise_cfg` -> one learning rate and
one weight decay per parameter, `clip_grad` and `accumulative_counts` checked, the window rule of gradient accumulation, and
the `param_groups` a checkpoint stores; and the optimizer's own dict (`check_optimizer`: SGD, AdamW, Adam).  Pure Python:
nothing here needs a GPU.

`resolve_paramwise` restates mmengine's `DefaultOptimWrapperConstructor.add_params` (mmengine/optim/optimizer/
default_constructor.py) from its documented rules; mmengine is not a dependency and the restatement is NOT pinned against it
by a fixture ("unpinned").
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch.nn as nn

PARAMWISE_KEYS = ("custom_keys", "bias_lr_mult", "bias_decay_mult", "norm_decay_mult", "flat_decay_mult",
                  "dwconv_decay_mult", "dcn_offset_lr_mult", "bypass_duplicate")
CUSTOM_KEYS = ("lr_mult", "decay_mult")
CLIP_KEYS = ("max_norm", "norm_type", "error_if_nonfinite")


def _is_norm(m: nn.Module) -> bool:
    from .modules import FrozenStatBN, GNHolder
    return isinstance(m, (FrozenStatBN, GNHolder, nn.modules.batchnorm._BatchNorm, nn.GroupNorm, nn.LayerNorm))


def check_paramwise(paramwise_cfg: Optional[dict]) -> dict:
    cfg = dict(paramwise_cfg or {})
    for k in cfg:
        if k not in PARAMWISE_KEYS:
            raise ValueError(f"paramwise_cfg: unknown key '{k}' (known: {', '.join(PARAMWISE_KEYS)})")
    ck = cfg.get("custom_keys", {})
    if not isinstance(ck, dict):
        raise ValueError(f"paramwise_cfg: 'custom_keys' must be a dict, got {type(ck).__name__}")
    for key, opts in ck.items():
        if not isinstance(opts, dict):
            raise ValueError(f"paramwise_cfg: custom_keys['{key}'] must be a dict, got {type(opts).__name__}")
        for k in opts:
            if k not in CUSTOM_KEYS:
                raise ValueError(f"paramwise_cfg: unknown key '{k}' in custom_keys['{key}'] (known: {', '.join(CUSTOM_KEYS)})")
    return cfg


def resolve_paramwise(model: nn.Module, base_lr: float, base_wd: float, paramwise_cfg: Optional[dict]) -> List[dict]:
    """-> one dict(name, lr_mult, lr, weight_decay, requires_grad) per parameter, in `model.parameters()` order.
    Per parameter with full dotted name n, own name `name` and owning module m:
      1. the keys of `custom_keys`, longest first and alphabetical among equal lengths; the first one that is a SUBSTRING of n
         sets lr = base_lr * lr_mult and weight_decay = base_wd * decay_mult (both default 1) and ends the search;
      2. otherwise lr = base_lr * bias_lr_mult for a `bias` that belongs neither to a normalisation layer nor to a deformable
         convolution (a DeformConvHolder or its `conv_offset` child), then lr = base_lr * dcn_offset_lr_mult for BOTH parameters of
         a `conv_offset` module inside a deformable convolution (mmengine 0.7.3's rule, restated from the published source,
         unpinned: mmengine is not a dependency), and
      3. weight_decay = base_wd * norm_decay_mult in a normalisation layer, else * bias_decay_mult for a `bias`, else
         * flat_decay_mult for a 1-D parameter; a multiplier that is not given is passed over (mmengine's `elif` chain: the
         bias of a normalisation layer takes bias_decay_mult when norm_decay_mult is absent);
      4. dwconv_decay_mult and bypass_duplicate have nothing to act on in these models (no depthwise convolution, no shared
         parameter); dcn_offset_lr_mult acts only in models with DCN blocks (ResNet(dcn=...)).
    Frozen parameters keep the base values."""
    cfg = check_paramwise(paramwise_cfg)
    custom = cfg.get("custom_keys", {})
    keys = sorted(sorted(custom.keys()), key=len, reverse=True)
    bias_lr, bias_wd = cfg.get("bias_lr_mult"), cfg.get("bias_decay_mult")
    norm_wd, flat_wd = cfg.get("norm_decay_mult"), cfg.get("flat_decay_mult")
    dcn_lr = cfg.get("dcn_offset_lr_mult")
    from .modules import DeformConvHolder
    in_dcn = {id(c) for m in model.modules() if isinstance(m, DeformConvHolder) for c in m.modules()}
    by_id: Dict[int, dict] = {}
    for prefix, m in model.named_modules():
        norm = _is_norm(m)
        dcn = id(m) in in_dcn
        for name, p in m.named_parameters(recurse=False):
            if id(p) in by_id:
                continue
            n = f"{prefix}.{name}" if prefix else name
            lr_mult, wd_mult = 1.0, 1.0
            if p.requires_grad:
                key = next((k for k in keys if k in n), None)
                if key is not None:
                    lr_mult = float(custom[key].get("lr_mult", 1.0))
                    wd_mult = float(custom[key].get("decay_mult", 1.0))
                else:
                    if name == "bias" and not (norm or dcn) and bias_lr is not None:
                        lr_mult = float(bias_lr)
                    if dcn and "conv_offset" in prefix and dcn_lr is not None:
                        lr_mult = float(dcn_lr)
                    if norm and norm_wd is not None:
                        wd_mult = float(norm_wd)
                    elif name == "bias" and bias_wd is not None:
                        wd_mult = float(bias_wd)
                    elif p.dim() == 1 and flat_wd is not None:
                        wd_mult = float(flat_wd)
            by_id[id(p)] = dict(name=n, lr_mult=lr_mult, lr=base_lr * lr_mult, weight_decay=base_wd * wd_mult,
                                requires_grad=bool(p.requires_grad))
    return [by_id[id(p)] for p in model.parameters()]


def check_clip_grad(clip_grad: Optional[dict]) -> Optional[dict]:
    """-> dict(max_norm, error_if_nonfinite) or None.  Only the 2-norm is built."""
    if clip_grad is None:
        return None
    cg = dict(clip_grad)
    for k in cg:
        if k not in CLIP_KEYS:
            raise ValueError(f"clip_grad: unknown key '{k}' (known: {', '.join(CLIP_KEYS)})")
    if "max_norm" not in cg:
        raise ValueError("clip_grad: 'max_norm' is missing")
    if float(cg.get("norm_type", 2)) != 2.0:
        raise NotImplementedError(f"clip_grad: norm_type={cg['norm_type']} (only the 2-norm is built)")
    if not float(cg["max_norm"]) > 0:
        raise ValueError(f"clip_grad: max_norm={cg['max_norm']} must be positive")
    return dict(max_norm=float(cg["max_norm"]), error_if_nonfinite=bool(cg.get("error_if_nonfinite", False)))


def check_accumulative_counts(k) -> int:
    if int(k) != k or int(k) < 1:
        raise ValueError(f"accumulative_counts={k!r} must be a positive integer")
    return int(k)


def should_update(it: int, k: int) -> bool:
    """mmengine's OptimWrapper.should_update by iteration: the call at 0-based iteration `it` applies the window"""
    return (it + 1) % k == 0


def accumulation_windows(iters: int, k: int) -> List[tuple]:
    """(0-based iteration that triggers the update or None for the closing flush, micro-steps in the window) of a run of
    `iters` iterations followed by a flush: the schedule ERDTrainer follows"""
    out, m = [], 0
    for it in range(iters):
        m += 1
        if should_update(it, k):
            out.append((it, m))
            m = 0
    if m:
        out.append((None, m))
    return out


def build_param_groups(resolved: List[dict], last_lr: float, base_lr: float, momentum: float,
                       optimizer: Optional[dict] = None) -> List[dict]:
    """`param_groups` of the optimizer state dict under a paramwise_cfg, in torch.optim.SGD's layout: one group per parameter
    in `model.parameters()` order (what mmengine's constructor builds), each with its own lr (the schedule's current factor
    last_lr / base_lr applied), initial_lr and weight_decay.  `optimizer`: a checked AdamW / Adam dict (check_optimizer) gives
    that optimizer's layout instead (`momentum` is not read)"""
    if optimizer is not None and optimizer["type"] in ADAM_TYPES:
        return [adam_param_group(optimizer, last_lr * r["lr_mult"], base_lr * r["lr_mult"], r["weight_decay"], [i])
                for i, r in enumerate(resolved)]
    return [dict(lr=last_lr * r["lr_mult"], momentum=momentum, dampening=0, weight_decay=r["weight_decay"], nesterov=False,
                 maximize=False, foreach=None, differentiable=False, initial_lr=base_lr * r["lr_mult"], params=[i])
            for i, r in enumerate(resolved)]


# ---- the optimizer itself: SGD (the update the ERD configs use), AdamW, Adam ---------------------------------------------------
ADAM_TYPES = ("AdamW", "Adam")
ADAM_KEYS = ("type", "lr", "betas", "eps", "weight_decay", "amsgrad", "maximize")


def check_optimizer(cfg: Optional[dict]) -> dict:
    """`optim_wrapper.optimizer` -> a plain dict.  SGD (and None, the trainer's default) passes as it is: the trainer reads lr,
    momentum and weight_decay from it as before.  AdamW / Adam -> dict(type, lr, betas, eps, weight_decay) with torch's defaults
    filled in (weight_decay 0.01 decoupled for AdamW, 0 coupled for Adam)."""
    if cfg is None:
        return dict(type="SGD")
    cfg = dict(cfg.to_dict() if hasattr(cfg, "to_dict") else cfg)
    kind = cfg.get("type")
    if kind == "SGD":
        return cfg
    if kind not in ADAM_TYPES:
        raise NotImplementedError(f"optimizer: type={kind!r} is not built (built: SGD, {', '.join(ADAM_TYPES)})")
    for k in cfg:
        if k not in ADAM_KEYS:
            raise ValueError(f"optimizer: unknown key '{k}' for {kind} (known: {', '.join(ADAM_KEYS)})")
    for k in ("amsgrad", "maximize"):
        if cfg.get(k):
            raise NotImplementedError(f"optimizer: {k}=True is not built")
    betas = cfg.get("betas", (0.9, 0.999))
    if not isinstance(betas, (tuple, list)) or len(betas) != 2:
        raise ValueError(f"optimizer: betas={betas!r} must be a pair")
    betas = (float(betas[0]), float(betas[1]))
    if not all(0.0 <= b < 1.0 for b in betas):
        raise ValueError(f"optimizer: betas={betas} must lie in [0, 1)")
    lr, eps = float(cfg.get("lr", 1e-3)), float(cfg.get("eps", 1e-8))
    wd = float(cfg.get("weight_decay", 0.01 if kind == "AdamW" else 0.0))
    if lr < 0 or eps < 0 or wd < 0:
        raise ValueError(f"optimizer: lr={lr}, eps={eps} and weight_decay={wd} must not be negative")
    return dict(type=kind, lr=lr, betas=betas, eps=eps, weight_decay=wd)


def adam_bias_corrections(beta1: float, beta2: float, step: int) -> tuple:
    """(1 / (1 - beta1^t), 1 / sqrt(1 - beta2^t)) of the t-th update (t >= 1) in double: what torch.optim.Adam divides the step size
    and the root of the second moment by"""
    if int(step) < 1:
        raise ValueError(f"adam_bias_corrections: step={step!r} (updates count from 1)")
    return 1.0 / (1.0 - float(beta1) ** int(step)), 1.0 / (1.0 - float(beta2) ** int(step)) ** 0.5


def adam_param_group(optimizer: dict, lr: float, initial_lr: float, weight_decay: float, params: List[int]) -> dict:
    """one entry of `param_groups` in torch.optim.AdamW's / Adam's layout"""
    return dict(lr=lr, betas=tuple(optimizer["betas"]), eps=optimizer["eps"], weight_decay=weight_decay, amsgrad=False,
                maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                decoupled_weight_decay=optimizer["type"] == "AdamW", initial_lr=initial_lr, params=list(params))


# ---- custom_hooks: EMAHook (weight averaging) ------------------------------------------------------------------------------------
# mmengine's EMAHook / ExponentialMovingAverage restated from their documented behaviour (NOT pinned against mmengine, DESIGN.md
# section 8.9); the one formula the reference tree holds is mmdet's ExpMomentumEMA.avg_func (mmdet/models/layers/ema.py:53-66).
EMA_TYPES = ("ExponentialMovingAverage", "ExpMomentumEMA")
EMA_HOOK_KEYS = ("type", "ema_type", "strict_load", "begin_iter", "begin_epoch", "priority")
EMA_MODEL_KEYS = ("momentum", "interval", "update_buffers", "device")


def check_custom_hooks(custom_hooks) -> Optional[dict]:
    """`custom_hooks` -> None (absent or empty) or the checked EMAHook: dict(ema_type, momentum, gamma, interval, begin_iter,
    begin_epoch, update_buffers, strict_load).  EMAHook is the one hook type built; `priority` is accepted and ignored (the
    average is taken after the iteration's update, nothing else competes for the slot); `update_buffers` is accepted with either
    value and changes nothing (frozen tensors and BN statistics are not averaged); `strict_load` is accepted and
    has nothing to act on (a resumed average takes the keys the checkpoint holds, a missing one starts as a copy of its
    parameter).  Everything else raises ValueError naming the key."""
    if custom_hooks is None:
        return None
    if not isinstance(custom_hooks, (list, tuple)):
        raise ValueError(f"custom_hooks must be a list of dicts, got {type(custom_hooks).__name__}")
    if len(custom_hooks) == 0:
        return None
    hooks = [dict(h.to_dict() if hasattr(h, "to_dict") else h) for h in custom_hooks]
    for h in hooks:
        if h.get("type") != "EMAHook":
            raise ValueError(f"custom_hooks: type={h.get('type')!r} is not built (built: EMAHook)")
    if len(hooks) > 1:
        raise ValueError("custom_hooks: more than one 'EMAHook' entry (one average per model is built)")
    h = hooks[0]
    kind = h.get("ema_type", "ExponentialMovingAverage")
    if kind not in EMA_TYPES:
        raise ValueError(f"EMAHook: ema_type={kind!r} is not built (built: {', '.join(EMA_TYPES)})")
    known = EMA_HOOK_KEYS + EMA_MODEL_KEYS + (("gamma",) if kind == "ExpMomentumEMA" else ())
    for k in h:
        if k not in known:
            raise ValueError(f"EMAHook: unknown key '{k}' for {kind} (known: {', '.join(known)})")
    if h.get("device") is not None:
        raise ValueError(f"EMAHook: device={h['device']!r} is not built (the average lives beside the parameters)")
    momentum = float(h.get("momentum", 0.0002))
    if not 0.0 < momentum < 1.0:
        raise ValueError(f"EMAHook: momentum={momentum} must lie in (0, 1)")
    gamma = h.get("gamma", 2000)
    if not float(gamma) > 0:
        raise ValueError(f"EMAHook: gamma={gamma!r} must be positive")
    interval = h.get("interval", 1)
    if int(interval) != interval or int(interval) < 1:
        raise ValueError(f"EMAHook: interval={interval!r} must be a positive integer")
    begin = {}
    for k in ("begin_iter", "begin_epoch"):
        v = h.get(k, 0)
        if int(v) != v or int(v) < 0:
            raise ValueError(f"EMAHook: {k}={v!r} must be a non-negative integer")
        begin[k] = int(v)
    if begin["begin_iter"] > 0 and begin["begin_epoch"] > 0:
        raise ValueError("EMAHook: begin_iter and begin_epoch are both set (give one of them)")
    return dict(ema_type=kind, momentum=momentum, gamma=float(gamma), interval=int(interval), update_buffers=bool(h.get("update_buffers", False)),
                strict_load=bool(h.get("strict_load", False)), **begin)


def ema_coefficient(kind: str, momentum: float, gamma: float, steps: int) -> float:
    """the weight of the parameters in the average taken when `steps` averages have been counted, a double:
    ExponentialMovingAverage: momentum; ExpMomentumEMA: (1 - momentum) * exp(-(1 + steps) / gamma) + momentum (ema.py:64-65)"""
    import math
    if kind == "ExponentialMovingAverage":
        return float(momentum)
    if kind == "ExpMomentumEMA":
        return (1 - momentum) * math.exp(-float(1 + steps) / gamma) + momentum
    raise ValueError(f"ema_coefficient: ema_type={kind!r} is not built (built: {', '.join(EMA_TYPES)})")


def ema_started(ema: dict, it: int, epoch: int) -> bool:
    """has averaging begun at 0-based iteration `it` of 0-based epoch `epoch`?  By epoch when begin_epoch is given (> 0),
    otherwise by iteration"""
    if ema["begin_epoch"] > 0:
        return epoch + 1 >= ema["begin_epoch"]
    return it + 1 >= ema["begin_iter"]


def ema_action(ema: dict, steps: int, started: bool) -> tuple:
    """what EMAHook does after one training iteration -> (mode, coefficient, steps afterwards).  Not started: the average is a
    copy of the parameters and `steps` stays 0.  Started: the first call copies, later ones average when steps % interval == 0
    and otherwise leave the average alone; each of them counts."""
    if not started:
        return "copy", 0.0, steps
    if steps == 0:
        return "copy", 0.0, 1
    if steps % ema["interval"] == 0:
        return "average", ema_coefficient(ema["ema_type"], ema["momentum"], ema["gamma"], steps), steps + 1
    return "skip", 0.0, steps + 1
