#!/usr/bin/env python3
"""Writes tests/golden/f14_iou_losses.npz from the REAL reference losses (mmdet/models/losses/iou_loss.py, executed through
oracle/ref_stub.py) on the case tables of tests/iou_refs.py: per kind and case the fp32 rows (reduction='none'), the gradient of
sum_i coef_i rows_i w.r.t. the predicted boxes, and the modules' values for iou_refs.MODULE_RUNS (reductions none / mean / sum,
with and without avg_factor, [n], [n, 4] and all-zero weights).  Runs on the CPU where the reference tree is present."""
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def reference_module(ref, kind, loss_weight=1.0, reduction="mean"):
    """the reference's loss module of an iou_refs kind"""
    import iou_refs as IR
    if kind.startswith("iou_"):
        return ref.IoULoss(mode=kind[4:], eps=IR.EPS, loss_weight=loss_weight, reduction=reduction)
    cls = ref.DIoULoss if kind == "diou" else ref.CIoULoss
    return cls(eps=IR.EPS, loss_weight=loss_weight, reduction=reduction)


def reference_values(ref, kind, c):
    """{key: array} of one (kind, case): rows, grad and one entry per MODULE_RUNS line"""
    import iou_refs as IR
    out = {}
    mod = reference_module(ref, kind)
    p = c.pred.clone().requires_grad_(True)
    rows = mod(p, c.target, reduction_override="none")
    (rows * c.coef).sum().backward()
    out["rows"], out["grad"] = rows.detach().numpy(), p.grad.numpy()
    mod = reference_module(ref, kind, loss_weight=IR_LOSS_WEIGHT)
    for i, (reduction, avg_factor, form) in enumerate(IR.MODULE_RUNS):
        w = IR.module_weight(c, form)
        out[f"run{i}"] = mod(c.pred, c.target, weight=w, avg_factor=avg_factor, reduction_override=reduction).detach().numpy()
    return out


IR_LOSS_WEIGHT = 2.0


def main():
    import iou_refs as IR
    from oracle import ref_stub
    ref = ref_stub.load_reference()
    data = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for kind in IR.KINDS:
            for c in IR.cases():
                for k, v in reference_values(ref, kind, c).items():
                    data[f"{kind}.{c.name}.{k}"] = v
    out = os.path.join(ROOT, "tests", "golden", "f14_iou_losses.npz")
    np.savez_compressed(out, **data)
    print(out, os.path.getsize(out), "bytes;", len(data), "arrays")


if __name__ == "__main__":
    main()
