#!/usr/bin/env python3
"""What the EMAHook costs (EXPERIMENTS 8.9): erd_ema_update / erd_swap_f32 alone over the flat parameter buffer of the default 40+40
step, by HIP events against their byte counts, and the batch-4 800x1344 step with and without the hook in alternating pairs on one box.

  average  12 B per element: the parameters read, the average read and written      copy  8 B      swap  16 B
  bound    bytes / 8 TB/s (HBM); two 129 MB buffers do not fit the 256 MB of last-level cache, repeated launches stream from HBM

usage: python tools/bench_ema.py [kernel] [step] [--pairs N] [--steps K]        (both by default, 3 pairs of 20 timed steps)"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import torch

import bench
from erd_amd import kernels as K
from erd_amd import optim_cfg as OC

HBM = 8e12
HOOK = [dict(type="EMAHook", ema_type="ExpMomentumEMA", momentum=0.0002, update_buffers=True, priority=49)]


def _trainer(dev, ema):
    from erd_amd.engine import ERDTrainer
    model, cfg = bench.build_model(dev, 0, "r50_40_40")
    opt = cfg.optim_wrapper.optimizer
    tr = ERDTrainer(model, lr=opt.lr, momentum=opt.momentum, weight_decay=opt.weight_decay,
                    base_batch_size=cfg.auto_scale_lr.base_batch_size, batch_size_per_gpu=4, auto_scale_lr=cfg.auto_scale_lr.enable,
                    ema=OC.check_custom_hooks(HOOK) if ema else None)
    return tr, cfg


def _time(fn, n=50):
    for _ in range(5):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / n


def kernel():
    dev = torch.device("cuda", 0)
    tr, _ = _trainer(dev, True)
    n = tr.flat.total
    p, avg, g, buf = tr.flat.data, tr.ema_buf, tr.flat.grad, tr.flat.momentum
    c = OC.ema_coefficient("ExpMomentumEMA", 0.0002, 2000, 1000)
    rows = [("erd_ema_update average", 12, lambda: K.ema_update(avg, p, c)),
            ("erd_ema_update copy", 8, lambda: K.ema_update(avg, p, c, copy=True)),
            ("erd_swap_f32 (twice: the buffers end as they were)", 32, lambda: (K.swap_(p, avg), K.swap_(p, avg))),
            ("erd_sgd_momentum (the update it follows, lr 0)", 20, lambda: K.sgd_momentum_(p, g, buf, 0.0, 0.9, 0.0, 1.0, False))]
    print(f"flat buffer: {n} floats = {4 * n / 1e6:.1f} MB, {len(tr.flat.buckets)} buckets")
    print(f"{'launch':52s} {'us':>8s} {'bytes':>12s} {'GB/s':>8s} {'HBM bound us':>13s} {'of bound':>9s}")
    for name, per, fn in rows:
        us = _time(fn)
        nbytes = per * n
        print(f"{name:52s} {us:8.1f} {nbytes:12d} {nbytes / us / 1e3:8.0f} {nbytes / HBM * 1e6:13.1f} {nbytes / HBM * 1e6 / us:9.2f}")
    # per bucket, as the trainer launches it behind each bucket's update
    def buckets():
        for s, e, _ in tr.flat.buckets:
            K.ema_update(avg[s:e], p[s:e], c)
    us = _time(buckets)
    print(f"{'erd_ema_update average, one launch per bucket':52s} {us:8.1f} {12 * n:12d} {12 * n / us / 1e3:8.0f} {12 * n / HBM * 1e6:13.1f} "
          f"{12 * n / HBM * 1e6 / us:9.2f}")


def step(pairs, steps=20):
    dev = torch.device("cuda", 0)
    res = {False: [], True: []}
    for rnd in range(pairs):
        for ema in (False, True):
            tr, cfg = _trainer(dev, ema)
            batches = [bench.synthetic_gpu_batch(4, seed=i, device=dev, cfg=cfg) for i in range(2)]
            for i in range(5):
                tr.train_step(*batches[i % 2], next_batch=batches[(i + 1) % 2])
            tr.flush()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps):
                log = tr.train_step(*batches[(i + 1) % 2], next_batch=batches[i % 2])
            tr.flush()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / steps
            res[ema].append(ms)
            print(f"pair {rnd + 1}  {'EMAHook' if ema else 'no hook':8s} {ms:7.2f} ms / step  {4e3 / ms:6.1f} img/s   loss {float(log['loss']):.4f}"
                  + (f"   steps counted {tr.ema_steps}" if ema else ""), flush=True)
            del tr, batches
            torch.cuda.empty_cache()
    a, b = sum(res[False]) / pairs, sum(res[True]) / pairs
    print(f"mean of {pairs} runs of {steps} steps: no hook {a:.2f} ms, EMAHook {b:.2f} ms ({(b - a) * 1e3:+.0f} us per step, {(b / a - 1) * 100:+.2f} %); "
          f"spread of the no-hook runs {max(res[False]) - min(res[False]):.2f} ms")


if __name__ == "__main__":
    args = sys.argv[1:]
    pairs = int(args[args.index("--pairs") + 1]) if "--pairs" in args else 3
    steps = int(args[args.index("--steps") + 1]) if "--steps" in args else 20
    what = [a for a in args if a in ("kernel", "step")] or ["kernel", "step"]
    if "kernel" in what:
        kernel()
    if "step" in what:
        step(pairs, steps)
