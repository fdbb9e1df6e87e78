#!/usr/bin/env python3
"""Writes tests/golden/f13_resnext.npz from the REAL reference backbone (mmdet/models/backbones/resnext.py, executed through
oracle/ref_stub.py): ResNeXt-50 32x4d with the oracle's procedural weights, N = 1, a 3 x 64 x 64 input.  Content: the input,
the four stage outputs and a seeded sample of the parameter gradients of the fixed weighted-sum loss of
tests/grouped_refs.stage_loss_weights.  Runs on the CPU where the reference tree is present."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

DEPTH, GROUPS, BASE_WIDTH, SEED = 50, 32, 4, 0
SAMPLES_PER_PARAM = 8


def reference_resnext(depth=DEPTH, groups=GROUPS, base_width=BASE_WIDTH):
    """the reference's ResNeXt class, built with the GFL configs' arguments (configs/gfl/gfl_x101-32x4d_fpn_ms-2x_coco.py)"""
    from oracle import ref_stub
    ref_stub.load_reference()
    mod = ref_stub._load("mmdet.models.backbones.resnext", "mmdet/models/backbones/resnext.py", ["mmdet.models.backbones"])
    return mod.ResNeXt(depth=depth, groups=groups, base_width=base_width, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=1,
                       norm_cfg=dict(type="BN", requires_grad=True), norm_eval=True, style="pytorch")


def golden_input():
    import golden_inputs as G
    return G.randn(1300, 1, 3, 64, 64)


def sample_index(name: str, numel: int) -> np.ndarray:
    """SAMPLES_PER_PARAM flat positions of a parameter's gradient, seeded by its name"""
    from oracle import erd_oracle as O
    rng = np.random.Generator(np.random.PCG64(O._name_seed(13, name)))
    return np.sort(rng.choice(numel, size=min(SAMPLES_PER_PARAM, numel), replace=False)).astype(np.int64)


def main():
    import grouped_refs as R
    from oracle import erd_oracle as O
    shapes = R.resnext_param_shapes(DEPTH, GROUPS, BASE_WIDTH)
    sd = {k: O.procedural_tensor(SEED, "backbone." + k, shp) for k, shp in shapes.items()}
    net = reference_resnext()
    net.load_state_dict(sd, strict=True)
    net.train()
    x = golden_input()
    outs = net(x)
    ws = R.stage_loss_weights(outs)
    sum((o * w).sum() for o, w in zip(outs, ws)).backward()
    data = {"x": x.numpy()}
    for i, o in enumerate(outs):
        data[f"out{i}"] = o.detach().numpy()
    names, idx, val = [], [], []
    for k, p in net.named_parameters():
        if p.grad is None:
            continue
        ii = sample_index(k, p.numel())
        names.append(k)
        idx.append(ii)
        val.append(p.grad.reshape(-1)[torch.from_numpy(ii)].numpy())
        data["gmax." + k] = np.float32(p.grad.abs().max())
    data["grad_names"] = np.array(names)
    for k, ii, v in zip(names, idx, val):
        data["gidx." + k] = ii
        data["gval." + k] = v
    out = os.path.join(ROOT, "tests", "golden", "f13_resnext.npz")
    np.savez_compressed(out, **data)
    print(out, os.path.getsize(out), "bytes;", len(names), "gradients sampled")


if __name__ == "__main__":
    main()
