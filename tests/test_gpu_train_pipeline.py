"""GPU: multi-scale training -- the one-launch batch resize (erd_resize_normalize_batch: no host tables, coefficients computed
in the kernel) against the test oracle (oracle/image_ops.py, OpenCV's 8-bit bilinear resize restated, UNPINNED vs cv2) and against
the per-image launch, bit for bit; GpuDetPipeline / CocoTrainData with a RandomResize sampler; a trainer fed batches whose padded
shape changes every step."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import erd_oracle as O
from oracle import image_ops as I

PAD = 7.5            # not the pipeline's 0: padding must be seen to be WRITTEN
# (sh, sw, nh, nw, flip) -- one batch, slot 1333 x 1336:
BIG = [(48, 64, 30, 40, 0),        # downscale in both axes; smaller than its slot in both axes
       (1, 9, 4, 13, 1),           # a source one pixel high (y1 = min(y0 + 1, sh - 1) = 0), upscaled
       (40, 30, 25, 45, 0),        # mixed: wider but shorter
       (9, 1, 12, 1, 1),           # a source one pixel wide, nw == sw
       (3, 4, 1333, 1336, 1),      # fills its slot; upscale in both axes, flipped
       (2, 1279, 2, 1333, 0),      # long coefficient runs at the real sizes, almost no pixels
       (1279, 2, 1333, 2, 1)]      # ... and along y
# slot 33 x W for W = 48 (float4 rows) and W = 45 (element-wise rows; the filling image is W wide)
SMALL = [(48, 64, 30, 40, 0), (20, 24, 33, 41, 1), (40, 30, 25, 45, 0), (9, 1, 12, 1, 1), (1, 45, 4, 45, 1), (21, 31, 33, None, 1),
         (5, 5, 5, 5, 0)]


def _images(cases, seed):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, (sh, sw, 3), dtype=np.uint8) for sh, sw, _, _, _ in cases]


def _reference(cases, imgs, H, W, swap):
    """oracle resize -> flip -> (BGR -> RGB) -> (v - mean) / std, the arithmetic of test_pipeline_batch_bit_exact_vs_oracle"""
    mean = torch.tensor(O.PIXEL_MEAN).view(3, 1, 1)
    std = torch.tensor(O.PIXEL_STD).view(3, 1, 1)
    ref = torch.full((len(cases), 3, H, W), PAD, dtype=torch.float32)
    for k, ((sh, sw, nh, nw, flip), im) in enumerate(zip(cases, imgs)):
        u8 = I.resize_linear_u8(im, nw, nh)
        if flip:
            u8 = u8[:, ::-1]
        if swap:
            u8 = u8[:, :, ::-1]
        ref[k, :, :nh, :nw] = (torch.from_numpy(u8.copy()).permute(2, 0, 1).float() - mean) / std
    return ref


def _batch_launch(cases, imgs, H, W, swap):
    from erd_amd import kernels as K
    from erd_amd.datasets import pack_images
    packed = pack_images(imgs, [(nh, nw, flip) for _, _, nh, nw, flip in cases])
    out = torch.full((len(cases), 3, H, W), -1.0, dtype=torch.float32, device="cuda")
    K.resize_normalize_batch(packed.buf.cuda(), len(cases), out, O.PIXEL_MEAN, O.PIXEL_STD, swap, PAD)
    return out


def _per_image_launches(cases, imgs, H, W, swap):
    from erd_amd import kernels as K
    from erd_amd.datasets import linear_coeffs
    out = torch.full((len(cases), 3, H, W), -1.0, dtype=torch.float32, device="cuda")
    for k, ((sh, sw, nh, nw, flip), im) in enumerate(zip(cases, imgs)):
        xo, xc = linear_coeffs(sw, nw)
        yo, yc = linear_coeffs(sh, nh)
        tables = tuple(torch.from_numpy(a).cuda() for a in (xo, xc, yo, yc))
        K.resize_normalize_into(torch.from_numpy(im).cuda(), tables, (nh, nw), out[k], O.PIXEL_MEAN, O.PIXEL_STD, bool(flip), swap, PAD)
    return out


def _sets():
    """(name, cases, H, W): N = 7 at the real widths, N = 7 with float4 rows, N = 7 with W = 45 (element-wise rows), N = 1"""
    fill = lambda W: [c if c[3] is not None else (c[0], c[1], c[2], W, c[4]) for c in SMALL]
    return [("big", BIG, 1333, 1336), ("small48", fill(48), 33, 48), ("small45", fill(45), 33, 45), ("one", BIG[:1], 32, 40),
            ("one45", SMALL[2:3], 25, 45)]


@pytest.fixture(scope="module")
def launches():
    """every set through the batch launch and through the per-image launches, once, both channel orders"""
    got = {}
    for name, cases, H, W in _sets():
        imgs = _images(cases, seed=len(name))
        for swap in (True, False):
            got[name, swap] = (cases, imgs, H, W, _batch_launch(cases, imgs, H, W, swap), _per_image_launches(cases, imgs, H, W, swap))
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize("swap", [True, False])
@pytest.mark.parametrize("name", [s[0] for s in _sets()])
def test_batch_kernel_bit_exact_vs_oracle(launches, name, swap):
    cases, imgs, H, W, got, _ = launches[name, swap]
    assert W % 4 == (1 if name.endswith("45") else 0)
    ref = _reference(cases, imgs, H, W, swap).cuda()
    for k, (sh, sw, nh, nw, flip) in enumerate(cases):
        assert torch.equal(got[k, :, :nh, :nw], ref[k, :, :nh, :nw]), (name, k, cases[k])
        assert bool((got[k, :, nh:, :] == PAD).all()) and bool((got[k, :, :, nw:] == PAD).all()), (name, k)       # padding is written
    assert torch.equal(got, ref)


@pytest.mark.parametrize("swap", [True, False])
@pytest.mark.parametrize("name", [s[0] for s in _sets()])
def test_batch_kernel_equals_the_per_image_launches(launches, name, swap):
    _, _, _, _, got, per_image = launches[name, swap]
    assert torch.equal(got, per_image)


def test_batch_kernel_skips_a_record_that_leaves_the_buffer():
    """a record whose image would end behind the source buffer, or with a non-positive size, reads nothing: its slot is padding"""
    from erd_amd import kernels as K
    from erd_amd.datasets import RESIZE_ITEM, pack_images
    cases = [(6, 8, 9, 12, 0), (6, 8, 9, 12, 1), (6, 8, 9, 12, 0)]
    imgs = _images(cases, 3)
    packed = pack_images(imgs, [(nh, nw, f) for _, _, nh, nw, f in cases])
    rec = packed.buf.numpy()[:3 * RESIZE_ITEM.itemsize].view(RESIZE_ITEM)
    rec["offset"][1] = packed.buf.numel() - 16          # 6 * 8 * 3 bytes from here end behind the buffer
    rec["sw"][2] = 0
    out = torch.full((3, 3, 12, 12), -1.0, device="cuda")
    K.resize_normalize_batch(packed.buf.cuda(), 3, out, O.PIXEL_MEAN, O.PIXEL_STD, True, PAD)
    assert torch.equal(out[0], _reference(cases[:1], imgs[:1], 12, 12, True).cuda()[0])
    assert bool((out[1:] == PAD).all())


def _make_dataset(tmp_path, sizes):
    """(tests/test_gpu_datapipe.py's)"""
    from PIL import Image
    rng = np.random.RandomState(7)
    images, anns = [], []
    for i, (h, w) in enumerate(sizes):
        arr = rng.randint(0, 256, (h, w, 3), dtype=np.uint8)
        Image.fromarray(arr).save(tmp_path / f"{i:04d}.png")                    # RGB on disk
        images.append(dict(id=100 + i, file_name=f"{i:04d}.png", width=w, height=h))
        for k in range(2):
            x, y = rng.uniform(0, w - 20), rng.uniform(0, h - 20)
            bw, bh = rng.uniform(8, w - x), rng.uniform(8, h - y)
            anns.append(dict(id=len(anns) + 1, image_id=100 + i, category_id=1 + k, bbox=[float(x), float(y), float(bw), float(bh)],
                             area=float(bw * bh), iscrowd=0))
    ds = dict(images=images, annotations=anns, categories=[dict(id=1, name="a"), dict(id=2, name="b")])
    json.dump(ds, open(tmp_path / "ann.json", "w"))
    return ds


SIZES = [(48, 64), (60, 45), (33, 80), (50, 70), (64, 48), (40, 90), (70, 52)]
MS = [(133, 40), (133, 100)]            # RandomResize: long edge 133, short edge 40..100


def _drawn(seed, epoch, index, prob=0.5):
    """the rule restated: flip first, then one randint per edge"""
    rng = np.random.RandomState((seed * 1000003 + epoch * 7919 + index) % (2 ** 31 - 1))
    flip = bool(rng.rand() < prob)
    return flip, (int(rng.randint(133, 134)), int(rng.randint(40, 101)))


def test_pipeline_with_random_resize_vs_oracle(tmp_path):
    from erd_amd.datasets import CocoAnnotations, GpuDetPipeline, ScaleSampler, load_image_bgr
    _make_dataset(tmp_path, SIZES)
    ann = CocoAnnotations(str(tmp_path / "ann.json"), classes=("a", "b"), data_prefix=str(tmp_path), min_size=0)
    pipe = GpuDetPipeline(ann, flip_prob=0.5, seed=2, scale_sampler=ScaleSampler("RandomResize", scale=MS))
    pipe.set_epoch(1)
    idx = [0, 1, 2, 3]
    x, samples = pipe.batch(idx)
    mean = torch.tensor(O.PIXEL_MEAN).view(3, 1, 1)
    std = torch.tensor(O.PIXEL_STD).view(3, 1, 1)
    flips, scales, shapes = [], [], []
    for k, s in zip(idx, samples):
        bgr = load_image_bgr(str(tmp_path / f"{k:04d}.png"))
        m = s.metainfo
        flip, scale = _drawn(2, 1, k)
        flips.append(flip)
        scales.append(scale)
        want_u8, sf = I.resize_flip(bgr, scale, flip=flip)
        nh, nw = want_u8.shape[:2]
        shapes.append((nh, nw))
        assert m["flip"] == flip and m["img_shape"] == (nh, nw) and m["scale_factor"] == pytest.approx(sf)
        ref = (torch.from_numpy(want_u8[:, :, ::-1].copy()).permute(2, 0, 1).float() - mean) / std
        got = x[k].cpu()
        assert torch.equal(got[:, :nh, :nw], ref), k
        assert float(got[:, nh:, :].abs().max() if nh < got.shape[1] else 0) == 0 and \
            float(got[:, :, nw:].abs().max() if nw < got.shape[2] else 0) == 0
        d = ann.get_data_info(k)                              # boxes: scaled, clipped to the resized image, then mirrored
        b = torch.tensor([i["bbox"] for i in d["instances"]], dtype=torch.float32) * torch.tensor([sf[0], sf[1], sf[0], sf[1]],
                                                                                                    dtype=torch.float32)
        b[:, 0::2].clamp_(0, nw); b[:, 1::2].clamp_(0, nh)
        if flip:
            b = torch.stack([nw - b[:, 2], b[:, 1], nw - b[:, 0], b[:, 3]], 1)
        assert torch.allclose(s.gt_instances.bboxes, b) and s.gt_instances.labels.tolist() == [0, 1]
    assert len(set(scales)) > 1 and any(flips) and not all(flips)          # images of ONE batch at different scales
    H = -(-max(h for h, _ in shapes) // 32) * 32
    W = -(-max(w for _, w in shapes) // 32) * 32
    assert tuple(x.shape) == (4, 3, H, W) and all(s.metainfo["pad_shape"] == (H, W) for s in samples)
    x2, _ = pipe.batch(idx)
    assert torch.equal(x, x2)
    assert not pipe._tables                                    # the training path builds and uploads no coefficient tables


def test_train_data_equals_pipeline_batches_with_and_without_workers(tmp_path):
    """CocoTrainData with 0 and 3 decoding threads == GpuDetPipeline.batch on the same indices, bit for bit"""
    from erd_amd.datasets import CocoAnnotations, GpuDetPipeline, ScaleSampler
    from erd_amd.runner import CocoTrainData
    _make_dataset(tmp_path, SIZES)
    dcfg = dict(data_root=str(tmp_path), ann_file="ann.json", data_prefix=dict(img=""), metainfo=dict(classes=("a", "b")),
                filter_cfg=dict(filter_empty_gt=True, min_size=0))
    runs = []
    for workers in (0, 3):
        data = CocoTrainData(dcfg, batch_size=2, seed=5, num_workers=workers, prefetch_factor=2, flip_prob=0.5,
                             scale_sampler=ScaleSampler("RandomResize", scale=MS))
        data.set_epoch(1)
        runs.append([(b["inputs"].cpu(), [s.gt_instances.bboxes.cpu() for s in b["data_samples"]],
                      [s.metainfo["img_id"] for s in b["data_samples"]]) for b in data])
    assert len(runs[0]) == len(runs[1]) == 4
    ann = CocoAnnotations(str(tmp_path / "ann.json"), classes=("a", "b"), data_prefix=str(tmp_path), min_size=0)
    pipe = GpuDetPipeline(ann, flip_prob=0.5, seed=5, scale_sampler=ScaleSampler("RandomResize", scale=MS))
    pipe.set_epoch(1)
    shapes = set()
    for (xa, ba, ia), (xb, bb, ib) in zip(*runs):
        assert ia == ib and torch.equal(xa, xb) and all(torch.equal(p, q) for p, q in zip(ba, bb))
        x, samples = pipe.batch([i - 100 for i in ia])
        assert torch.equal(x.cpu(), xa) and all(torch.equal(s.gt_instances.bboxes.cpu(), p) for s, p in zip(samples, ba))
        shapes.add(tuple(xa.shape[2:]))
    assert len(shapes) > 1                                     # the padded shape moves from batch to batch


def test_training_across_padded_shapes_and_runner_from_cfg(tmp_path):
    """three batches whose padded shapes differ through ONE trainer; then CocoTrainData.from_cfg on a RandomResize pipeline feeds Runner"""
    import e2e_util as U
    from erd_amd import Config
    from erd_amd.datasets import CocoAnnotations, GpuDetPipeline, ScaleSampler
    from erd_amd.engine import ERDTrainer
    from erd_amd.runner import CocoTrainData, Runner
    (tmp_path / "train2017").mkdir()
    (tmp_path / "annotations").mkdir()
    ds = _make_dataset(tmp_path / "train2017", [(120, 150), (140, 100), (100, 160), (150, 120)])
    ann = CocoAnnotations(str(tmp_path / "train2017" / "ann.json"), classes=("a", "b"), data_prefix=str(tmp_path / "train2017"), min_size=0)
    pipe = GpuDetPipeline(ann, seed=1, scale_sampler=ScaleSampler("RandomChoiceResize", scales=[(160, 96), (160, 128), (200, 160)]))
    tsd, ssd = U.f7_state_dicts()
    tr = ERDTrainer(U.build_erd(tsd, ssd), lr=0.01, batch_size_per_gpu=2, auto_scale_lr=False, warmup_iters=0)
    shapes = []
    for epoch, idx in ((0, [0, 1]), (1, [2, 3]), (2, [0, 3]), (3, [1, 2]), (4, [0, 2]), (5, [1, 3])):
        pipe.set_epoch(epoch)
        x, samples = pipe.batch(idx)
        if tuple(x.shape[2:]) in shapes:
            continue
        shapes.append(tuple(x.shape[2:]))
        log = tr.train_step(x, samples)
        assert np.isfinite(float(log["loss"])) and float(log["loss"]) > 0, (epoch, float(log["loss"]))
        if len(shapes) == 3:
            break
    tr.flush()
    assert len(shapes) == 3, shapes
    del tr

    for c, k in zip(ds["categories"], (1, 2)):
        c["name"] = f"cat{k}"
    json.dump(ds, open(tmp_path / "annotations" / "train.json", "w"))
    teacher = tmp_path / "teacher.pth"
    torch.save(dict(state_dict=O.procedural_state_dict(40, seed=0)), teacher)
    cfg = Config.fromfile(U.CFG_INCRE)
    cfg.work_dir = str(tmp_path / "w")
    pipeline = [dict(type="LoadImageFromFile", backend_args=None), dict(type="LoadAnnotations", with_bbox=True),
                dict(type="RandomResize", scale=[(200, 96), (200, 160)], keep_ratio=True), dict(type="RandomFlip", prob=0.5),
                dict(type="PackDetInputs")]
    cfg.merge_from_dict({"train_dataloader.batch_size": 2, "train_dataloader.num_workers": 2, "train_cfg.max_epochs": 1,
                         "train_dataloader.dataset.data_root": f"{tmp_path}/", "train_dataloader.dataset.ann_file": "annotations/train.json",
                         "train_dataloader.dataset.filter_cfg.min_size": 0, "train_dataloader.dataset.pipeline": pipeline,
                         "model.ori_setting.ori_checkpoint_file": str(teacher), "model.ori_setting.ori_config_file": U.CFG_FIRST,
                         "model.backbone.init_cfg": None, "default_hooks.logger.interval": 1})
    data = CocoTrainData.from_cfg(cfg)
    assert data.pipe.scale_sampler.type == "RandomResize" and data.pipe.flip_prob == 0.5 and len(data) == 2
    hist = Runner.from_cfg(cfg, data=data, log=lambda *_: None).train(max_iters=2)
    assert len(hist) == 2 and all(np.isfinite(r["loss"]) and r["loss"] > 0 for r in hist)


def test_train_py_trains_the_multi_scale_config_from_real_files(tmp_path):
    """tools/train.py on configs/gfl_increment/*_ms.py with COCO files present: the RandomResize pipeline of the config file is read
    and two iterations train, through the CLI"""
    import subprocess, sys
    import e2e_util as U
    (tmp_path / "annotations").mkdir()
    (tmp_path / "train2017").mkdir()
    ds = _make_dataset(tmp_path / "train2017", [(120, 150), (140, 100), (100, 160), (150, 120)])
    for c, k in zip(ds["categories"], (1, 2)):
        c["name"] = f"cat{k}"
    json.dump(ds, open(tmp_path / "annotations" / "train.json", "w"))
    teacher = tmp_path / "teacher.pth"
    torch.save(dict(state_dict=O.procedural_state_dict(40, seed=0)), teacher)
    cfg = os.path.join(U.ROOT, "configs", "gfl_increment", "gfl_r50_fpn_1x_coco_first_40_incre_last_40_cats_ms.py")
    cmd = [sys.executable, os.path.join(U.ROOT, "tools", "train.py"), cfg, "--work-dir", str(tmp_path / "w"),
           "--max-iters", "2", "--cfg-options", "train_dataloader.batch_size=2",
           f"train_dataloader.dataset.data_root={tmp_path}/", "train_dataloader.dataset.ann_file=annotations/train.json",
           "train_dataloader.dataset.filter_cfg.min_size=0",
           f"model.ori_setting.ori_checkpoint_file={teacher}", f"model.ori_setting.ori_config_file={U.CFG_FIRST}",
           "default_hooks.logger.interval=1"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "Epoch(train) [1][2/2]" in out.stdout and "loss_dist_bbox" in out.stdout
