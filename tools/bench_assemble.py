#!/usr/bin/env python3
"""Wall time per batch of the DEVICE half of the train data pipeline alone (GpuDetPipeline.assemble: host-to-device copies, the
resize / flip / normalise / pad launches, the data samples), synchronised at both ends of every call.  The host half (decode,
page-locked staging) is done before the clock starts, in the form the trainer's decode workers hand over.

    python tools/bench_assemble.py [--tree CHECKOUT] [--random] [--batches 300] [--label NAME]

--tree imports erd_amd from another checkout (A/B against an older commit on one box: a tree without `GpuDetPipeline.pack`
is timed through its list-of-pinned-images form); --random draws RandomResize(scale=[(1333, 480), (1333, 800)]) per image.
bs 4 of 480 x 640 sources, a dozen different images.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--random", action="store_true")
ap.add_argument("--batches", type=int, default=300)
ap.add_argument("--warmup", type=int, default=30)
ap.add_argument("--label", default="")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))

import numpy as np
import torch
from erd_amd import datasets as D

assert torch.cuda.is_available(), "needs an MI355X"
N, BS = 12, 4
rng = np.random.RandomState(0)
pixels = {f"{i}.jpg": rng.randint(0, 256, (480, 640, 3), dtype=np.uint8) for i in range(N)}
ds = dict(images=[dict(id=i, file_name=f"{i}.jpg", width=640, height=480) for i in range(N)],
          annotations=[dict(id=i + 1, image_id=i, category_id=1, bbox=[10.0, 20.0, 200.0, 150.0], area=30000.0, iscrowd=0) for i in range(N)],
          categories=[dict(id=1, name="a")])
ann = D.CocoAnnotations(ds, classes=("a",))
kw = {}
if args.random:
    kw["scale_sampler"] = D.ScaleSampler("RandomResize", scale=[(1333, 480), (1333, 800)])
pipe = D.GpuDetPipeline(ann, scale=(1333, 800), seed=0, loader=lambda p: pixels[p], **kw)
batched = hasattr(pipe, "pack")
times = []
for it in range(args.warmup + args.batches):
    pipe.set_epoch(it // (N // BS))                      # another epoch, other flips and scales
    idx = [(it * BS + k) % N for k in range(BS)]
    host = pipe.pack(idx) if batched else [D.pinned(im) for im in pipe.decode(idx)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    x, samples = pipe.assemble(idx, host)
    torch.cuda.synchronize()
    times.append(time.perf_counter() - t0)
t = np.array(times[args.warmup:]) * 1e3
print(json.dumps(dict(label=args.label, tree=os.path.abspath(args.tree), form="one launch per batch" if batched else "one launch per image",
                      random_scale=bool(args.random), batches=len(t), bs=BS, ms_per_batch_mean=round(float(t.mean()), 4),
                      ms_per_batch_median=round(float(np.median(t)), 4), ms_per_batch_p10=round(float(np.percentile(t, 10)), 4),
                      ms_per_batch_p90=round(float(np.percentile(t, 90)), 4), table_cache_keys=len(getattr(pipe, "_tables", {})),
                      last_shape=list(x.shape))))
