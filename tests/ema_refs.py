"""Host restatement of the weight average an EMAHook keeps (mmengine's EMAHook / ExponentialMovingAverage as documented, mmdet's
ExpMomentumEMA, mmdet/models/layers/ema.py:53-66), in numpy.  Independent of erd_amd: the coefficient, the element update in the
kernel's stated order, the per-iteration rule and a replay over weight snapshots are all written out here.

The element update is  ema = fmaf(src, c32, fl32(ema * d32))  with c32 = fl32(c), d32 = fl32(1 - c), both rounded once from the
double: the multiply is rounded to fp32 on its own, then ONE fused multiply-add follows -- what
`averaged.mul_(1 - c).add_(src, alpha=c)` computes on a host whose `add_(alpha=)` is an FMA.

fmaf without an fmaf: the fused step is evaluated as a float64 multiply-add of the fp32 operands, rounded once to fp32.
  * the product src * c32 of two 24-bit significands has at most 48 significant bits, so it is EXACT in float64 (53 bits);
  * the sum of that product and the fp32 addend is exact in float64 whenever the two lie within 2^5 of each other (the random
    bulk).  When it is not, float64 rounds first and the cast to fp32 rounds again; two roundings differ from one only where the
    float64 sum landed exactly on the midpoint of two fp32 neighbours although the exact sum lies beside it.  `fma32` takes the
    rounding error of the float64 sum by Knuth's TwoSum (exact in float64) and, at such a midpoint, moves the sum one float64 step
    to the side the exact value lies on before the cast: the cast then rounds the way ONE rounding of the exact value does.
NaN results compare equal whatever their payload (`same_bits`)."""
import math

import numpy as np

EMA_TYPES = ("ExponentialMovingAverage", "ExpMomentumEMA")


def coefficient(kind, momentum, gamma, steps):
    """the parameters' weight in the average taken when `steps` averages have been counted (a Python double)"""
    if kind == "ExponentialMovingAverage":
        return float(momentum)
    assert kind == "ExpMomentumEMA", kind
    return (1 - momentum) * math.exp(-float(1 + steps) / gamma) + momentum        # ema.py:64-65


def fma32(a, b, c):
    """fl32(a * b + c) with ONE rounding, for fp32 arrays a, b, c (see the module docstring)"""
    a, b, c = (np.asarray(v, dtype=np.float32) for v in (a, b, c))
    with np.errstate(all="ignore"):
        x = a.astype(np.float64) * b.astype(np.float64)             # exact: 48 bits
        y = np.broadcast_to(c.astype(np.float64), x.shape)
        s = x + y
        bb = s - x
        err = (x - (s - bb)) + (y - bb)                             # TwoSum: s + err == x + y exactly
        f = s.astype(np.float32)
        toward = np.where(s > f.astype(np.float64), np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)
        other = np.nextafter(f, toward)
        mid = 0.5 * f.astype(np.float64) + 0.5 * other.astype(np.float64)
        tie = np.isfinite(s) & np.isfinite(other) & (f.astype(np.float64) != s) & (mid == s) & (err != 0)
        s = np.where(tie, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def update(ema, src, c):
    """one averaging step of fp32 arrays in the stated order; `c` is the double coefficient"""
    ema, src = np.asarray(ema, dtype=np.float32), np.asarray(src, dtype=np.float32)
    c32, d32 = np.float32(c), np.float32(1.0 - c)
    with np.errstate(all="ignore"):
        t = ema * d32                                               # fp32 multiply, rounded on its own
    return fma32(src, c32, t)


def started(cfg, it, epoch):
    """0-based iteration `it` of 0-based epoch `epoch`: has averaging begun?"""
    if cfg.get("begin_epoch", 0) > 0:
        return epoch + 1 >= cfg["begin_epoch"]
    return it + 1 >= cfg.get("begin_iter", 0)


def action(cfg, steps, is_started):
    """-> (mode, coefficient, steps afterwards); mode is 'copy', 'average' or 'skip'"""
    if not is_started:
        return "copy", None, steps
    if steps == 0:
        return "copy", None, 1
    if steps % cfg.get("interval", 1) == 0:
        c = coefficient(cfg.get("ema_type", EMA_TYPES[0]), cfg.get("momentum", 0.0002), cfg.get("gamma", 2000), steps)
        return "average", c, steps + 1
    return "skip", None, steps + 1


def replay(cfg, snapshots, ema=None, steps=0, first_iter=0, epoch=0):
    """the average after each of `snapshots` (the fp32 weights after iterations first_iter, first_iter + 1, ...), starting from the
    average `ema` (None: whatever -- the first call copies) with `steps` counted -> (list of averages, steps afterwards)"""
    out = []
    for k, w in enumerate(snapshots):
        w = np.asarray(w, dtype=np.float32)
        mode, c, steps = action(cfg, steps, started(cfg, first_iter + k, epoch))
        if mode == "copy":
            ema = w.copy()
        elif mode == "average":
            ema = update(ema, w, c)
        out.append(ema.copy())
    return out, steps


def same_bits(a, b):
    """equal as bit patterns, NaN payloads free"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def ulp_distance(a, b):
    """distance of finite fp32 arrays in units in the last place (on the ordered integer line of fp32 values)"""
    def key(v):
        i = np.asarray(v, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))
