#!/usr/bin/env python3
"""The deformable-convolution kernels (erd_amd/csrc/conv_deform.hip) per launch at the DCN layers of a batch-4 800x1344 step, next to
their byte bounds, and the R50-dconv 40+40 step next to the plain R50 one.

  sampling  HBM bound = (x once + offsets + 36 * C bytes written per output pixel) / 8 TB/s
  backward  atomic bound = bytes added to dx (4 * C per in-range corner) / 1.3 TB/s, the chip-wide float-atomic rate; beside it the
            HBM bound of what it reads (dcol + offsets + x once)

usage: python tools/bench_deform.py [kernels] [step]        (both by default)"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import torch

import bench
from erd_amd import kernels as K

HBM, ATOMIC = 8e12, 1.3e12
# (IH, IW, C, stride) of conv2 in layer2 / layer3 / layer4 at batch 4, 800 x 1344: the stride-2 first block, then the stride-1 blocks
SHAPES = [(200, 336, 128, 2), (100, 168, 128, 1), (100, 168, 256, 2), (50, 84, 256, 1), (50, 84, 512, 2), (25, 42, 512, 1)]
OFFSET_SCALE = 0.15      # times the procedural conv_offset tensors: offsets of about a pixel (tests/test_gpu_dcn_backbone.py)


def _time(fn, n=20):
    for _ in range(3):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / n


def kernels():
    import deform_refs as R
    N = 4
    print(f"{'conv2 input':>22s} {'sampling us':>11s} {'HBM us':>7s} {'backward us':>11s} {'atomic us':>9s} {'read us':>8s}")
    for IH, IW, Cc, s in SHAPES:
        OH, OW = (IH - 1) // s + 1, (IW - 1) // s + 1
        g = torch.Generator(device="cuda").manual_seed(IH + Cc)
        x = torch.randn(N, IH, IW, Cc, device="cuda", generator=g)
        off = 0.75 * torch.randn(N, OH, OW, 18, device="cuda", generator=g)
        dcol = torch.randn(N, OH, OW, 9 * Cc, device="cuda", generator=g)
        col, dx, doff = torch.empty_like(dcol), torch.zeros_like(x), torch.empty_like(off)
        t_f = _time(lambda: K.deform_cols(x, off, s, out=col))
        t_b = _time(lambda: K.deform_cols_bwd(dcol, x, off, s, dx, doff))
        npix = N * OH * OW
        corners = float(R.corner_counts(off.cpu(), (IH, IW), s).sum())
        hbm_f = 4.0 * (x.numel() + off.numel() + col.numel()) / HBM * 1e6
        print(f"{N}x{IH}x{IW}x{Cc} s{s:<8d} {t_f:11.1f} {hbm_f:7.1f} {t_b:11.1f} {corners * 4 * Cc / ATOMIC * 1e6:9.1f} "
              f"{4.0 * (x.numel() + off.numel() + dcol.numel()) / HBM * 1e6:8.1f}      ({corners / (npix * 36):.2f} of the corners in range)")


def step():
    from erd_amd.engine import ERDTrainer
    dev = torch.device("cuda", 0)
    bench.ARCH["r50_dconv_40_40"] = dict(student="gfl_r50_dconv_c3-c5_fpn_1x_coco_first_40_incre_last_40_cats.py",
                                         teacher="gfl_r50_dconv_c3-c5_fpn_1x_coco_first_40_cats.py", c_old=40, c_all=80, batch=4, label="")
    for arch in ("r50_40_40", "r50_dconv_40_40", "r50_40_40", "r50_dconv_40_40"):
        model, cfg = bench.build_model(dev, 0, arch)
        with torch.no_grad():
            for n, p in model.named_parameters():
                if ".conv_offset." in n:
                    p.mul_(OFFSET_SCALE)
        opt = cfg.optim_wrapper.optimizer
        tr = ERDTrainer(model, lr=opt.lr, momentum=opt.momentum, weight_decay=opt.weight_decay,
                        base_batch_size=cfg.auto_scale_lr.base_batch_size, batch_size_per_gpu=4, auto_scale_lr=cfg.auto_scale_lr.enable)
        batches = [bench.synthetic_gpu_batch(4, seed=i, device=dev, cfg=cfg) for i in range(2)]
        for i in range(4):
            tr.train_step(*batches[i % 2])
        tr.flush()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps = 12
        for i in range(steps):
            log = tr.train_step(*batches[i % 2])
        tr.flush()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / steps
        print(f"{arch:18s} {ms:7.2f} ms / step  {4e3 / ms:6.1f} img/s   loss {float(log['loss']):.4f}")
        if arch == "r50_dconv_40_40":      # where the DCN launches stand in a serialized step
            tr.overlap_teacher = False
            K.timing_begin()
            for i in range(2):
                tr.train_step(*batches[i % 2])
            tr.flush()
            rec = K.timing_end()
            tot = sum(r["ms"] for r in rec.values()) / 2
            for k in ("deform_cols", "deform_cols_bwd"):
                if k in rec:
                    print(f"    {k:16s} {rec[k]['ms'] / 2:6.2f} ms / step in {rec[k]['launches'] // 2} launches  ({rec[k]['ms'] / 2 / tot:.1%} of {tot:.1f} ms of timed launches)")
        del tr, model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    what = sys.argv[1:] or ["kernels", "step"]
    if "kernels" in what:
        kernels()
    if "step" in what:
        step()
