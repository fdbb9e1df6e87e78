"""CPU: the train pipeline of a config as the product READS it (datasets.resolve_train_pipeline, the training twin of resolve_tta),
the per-image draws of multi-scale training (flip first, then the scale; mmcv 2.x sampling rules restated, UNPINNED), the packed
host buffer of a batch, and what the compiler makes of the batch resize kernel's coefficient arithmetic."""
import glob
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from e2e_util import ROOT

MS_CFG = "gfl_r50_fpn_1x_coco_first_40_incre_last_40_cats_ms.py"
LOAD = [dict(type="LoadImageFromFile", backend_args=None), dict(type="LoadAnnotations", with_bbox=True)]
PACK = [dict(type="PackDetInputs")]


def _key(seed, epoch, index):
    return (seed * 1000003 + epoch * 7919 + index) % (2 ** 31 - 1)


def _pipe(sampler=None, flip_prob=0.5, seed=0, n=64):
    from erd_amd.datasets import CocoAnnotations, GpuDetPipeline
    ds = dict(images=[dict(id=i, file_name=f"{i}.png", width=64, height=48) for i in range(n)],
              annotations=[dict(id=i + 1, image_id=i, category_id=1, bbox=[1.0, 1.0, 20.0, 20.0], area=400.0, iscrowd=0) for i in range(n)],
              categories=[dict(id=1, name="a")])
    return GpuDetPipeline(CocoAnnotations(ds, classes=("a",), min_size=0), scale=(50, 12), flip_prob=flip_prob, seed=seed,
                          scale_sampler=sampler)


def test_every_shipped_config_resolves_to_what_it_trains_with():
    from erd_amd import Config
    from erd_amd.datasets import resolve_train_pipeline
    files = sorted(glob.glob(os.path.join(ROOT, "configs", "gfl_increment", "*.py")))
    assert len(files) >= 14 and any(f.endswith(MS_CFG) for f in files)
    for f in files:
        got = resolve_train_pipeline(Config.fromfile(f).train_dataloader.dataset.pipeline)
        s = got["sampler"]
        assert got["flip_prob"] == 0.5, f
        if f.endswith(MS_CFG):
            assert s.type == "RandomResize" and s.scale == ((1333, 480), (1333, 800)) and s.ratio_range is None
            # 321 short edges: 8000 draws miss one of them with probability 321 * (320 / 321) ** 8000 < 1e-8
            drawn = {s(np.random.RandomState(k)) for k in range(8000)}
            assert {w for w, _ in drawn} == {1333} and {h for _, h in drawn} == set(range(480, 801))
        else:
            assert s.type == "Resize" and s.scale == (1333, 800), f
            assert s(None) == (1333, 800)                      # a fixed scale makes no draw: it never touches the generator


@pytest.mark.parametrize("bad, name", [
    (dict(type="Resize", scale=(1333, 800), keep_ratio=False), "Resize"),
    (dict(type="Resize", scale=(1333, 800)), "Resize"),
    (dict(type="RandomResize", scale=[(1333, 480), (1333, 800)], keep_ratio=False), "RandomResize"),
    (dict(type="RandomResize", scale=[(1333, 480), (1333, 640), (1333, 800)], keep_ratio=True), "RandomResize"),
    (dict(type="RandomChoiceResize", scales=[], keep_ratio=True), "RandomChoiceResize"),
    (dict(type="RandomChoiceResize", scales=[(1333, 800)]), "RandomChoiceResize"),
    (dict(type="Resize", scale=(1333, 800), keep_ratio=True, interpolation="nearest"), "Resize"),
])
def test_unbuilt_resize_forms_raise(bad, name):
    from erd_amd.datasets import resolve_train_pipeline
    with pytest.raises(ValueError, match=name):
        resolve_train_pipeline(LOAD + [bad, dict(type="RandomFlip", prob=0.5)] + PACK)


@pytest.mark.parametrize("extra, name", [
    (dict(type="RandomFlip", prob=0.5, direction="vertical"), "RandomFlip"),
    (dict(type="RandomFlip", prob=0.5, direction="diagonal"), "RandomFlip"),
    (dict(type="RandomFlip", prob=[0.3, 0.3], direction=["horizontal", "vertical"]), "RandomFlip"),
    (dict(type="RandomFlip", prob=1.5), "RandomFlip"),
    (dict(type="RandomCrop", crop_size=(512, 512)), "RandomCrop"),
    (dict(type="PhotoMetricDistortion"), "PhotoMetricDistortion"),
    (dict(type="Pad", size_divisor=32), "Pad"),
    (dict(type="Resize", scale=(666, 400), keep_ratio=True), "second resize"),
    (dict(type="RandomChoiceResize", scales=[(666, 400)], keep_ratio=True), "second resize"),
    (dict(type="LoadAnnotations", with_bbox=True, with_mask=True), "LoadAnnotations"),
])
def test_unbuilt_transforms_raise_by_name(extra, name):
    from erd_amd.datasets import resolve_train_pipeline
    with pytest.raises(ValueError, match=name):
        resolve_train_pipeline(LOAD + [dict(type="Resize", scale=(1333, 800), keep_ratio=True), extra] + PACK)


def test_flip_forms_and_missing_resize():
    from erd_amd.datasets import resolve_train_pipeline
    rs = [dict(type="Resize", scale=(1333, 800), keep_ratio=True)]
    assert resolve_train_pipeline(LOAD + rs + PACK)["flip_prob"] == 0.0                                  # absent: no flip
    assert resolve_train_pipeline(LOAD + rs + [dict(type="RandomFlip", prob=None)] + PACK)["flip_prob"] == 0.0
    assert resolve_train_pipeline(LOAD + rs + [dict(type="RandomFlip", prob=0.25)] + PACK)["flip_prob"] == 0.25
    assert resolve_train_pipeline(LOAD + rs + [dict(type="RandomFlip", prob=1, direction="horizontal")] + PACK)["flip_prob"] == 1.0
    with pytest.raises(ValueError, match="RandomFlip"):
        resolve_train_pipeline(LOAD + rs + [dict(type="RandomFlip", prob=0.5), dict(type="RandomFlip", prob=0.5)] + PACK)
    with pytest.raises(ValueError, match="no resize stage"):
        resolve_train_pipeline(LOAD + PACK)


def test_random_resize_two_scales_covers_its_range_and_nothing_else():
    from erd_amd.datasets import resolve_train_pipeline
    s = resolve_train_pipeline(LOAD + [dict(type="RandomResize", scale=[(50, 10), (50, 14)], keep_ratio=True)] + PACK)["sampler"]
    p = _pipe(s)
    seen = []
    for seed in range(10):
        p.seed = seed
        for index in range(20):
            flip, scale = p.draw(index, epoch=0)
            # the rule, recomputed: flip = first draw; then randint per edge, first edge first
            rng = np.random.RandomState(_key(seed, 0, index))
            assert flip == bool(rng.rand() < 0.5)
            assert scale == (rng.randint(50, 51), rng.randint(10, 15))
            seen.append(scale)
    assert len(seen) == 200 and {w for w, _ in seen} == {50} and {h for _, h in seen} == {10, 11, 12, 13, 14}
    # the two scales may come in either order and differ in both edges: each edge is drawn on its own
    s2 = resolve_train_pipeline(LOAD + [dict(type="RandomResize", scale=[(52, 10), (50, 12)], keep_ratio=True)] + PACK)["sampler"]
    got = {s2(np.random.RandomState(k)) for k in range(400)}
    assert got == {(w, h) for w in (50, 51, 52) for h in (10, 11, 12)}


def test_ratio_range_and_choice_cover_their_values_and_nothing_else():
    from erd_amd.datasets import resolve_train_pipeline
    s = resolve_train_pipeline(LOAD + [dict(type="RandomResize", scale=(40, 20), ratio_range=(0.5, 1.0), keep_ratio=True)] + PACK)["sampler"]
    p = _pipe(s, flip_prob=0.3)
    seen = set()
    for seed in range(10):
        p.seed = seed
        for index in range(20):
            flip, scale = p.draw(index, epoch=3)
            rng = np.random.RandomState(_key(seed, 3, index))
            assert flip == bool(rng.rand() < 0.3)
            r = rng.random_sample() * (1.0 - 0.5) + 0.5
            assert scale == (int(40 * r), int(20 * r))
            seen.add(scale)
    assert {h for _, h in seen} == set(range(10, 20))            # int(20 * r), r in [0.5, 1): every value 10..19
    assert {w for w, _ in seen} <= set(range(20, 40)) and all(abs(h - w / 2) < 1 for w, h in seen)
    c = resolve_train_pipeline(LOAD + [dict(type="RandomChoiceResize", scales=[(50, 10), (48, 12), (30, 30)], keep_ratio=True)] + PACK)["sampler"]
    p = _pipe(c, flip_prob=1.0)
    seen = []
    for seed in range(10):
        p.seed = seed
        for index in range(20):
            flip, scale = p.draw(index, epoch=0)
            rng = np.random.RandomState(_key(seed, 0, index))
            rng.rand()
            assert flip is True and scale == [(50, 10), (48, 12), (30, 30)][rng.randint(3)]
            seen.append(scale)
    assert set(seen) == {(50, 10), (48, 12), (30, 30)}


def test_flip_is_the_first_draw_whatever_the_resize_stage():
    from erd_amd.datasets import ScaleSampler
    samplers = [None, ScaleSampler("RandomResize", scale=[(50, 10), (50, 14)]),
                ScaleSampler("RandomResize", scale=(40, 20), ratio_range=(0.5, 1.0)),
                ScaleSampler("RandomChoiceResize", scales=[(50, 10), (48, 12)])]
    for prob in (0.0, 0.5, 1.0):
        flips = []
        for s in samplers:
            p = _pipe(s, flip_prob=prob, seed=4)
            p.set_epoch(2)
            flips.append([p.draw(i)[0] for i in range(64)])
            assert flips[-1] == [bool(np.random.RandomState(_key(4, 2, i)).rand() < prob) for i in range(64)]
        assert flips[0] == flips[1] == flips[2] == flips[3]
        if prob == 0.0:
            assert not any(flips[0])
        elif prob == 1.0:
            assert all(flips[0])
        else:
            assert any(flips[0]) and not all(flips[0])
    assert _pipe(None).draw(5)[1] == (50, 12)                       # the fixed scale


def test_draws_depend_on_seed_epoch_index_only(monkeypatch):
    """the same (seed, epoch, index) gives the same scale and flip whichever batch the image falls into; another epoch changes some"""
    from erd_amd import datasets as D
    p = _pipe(D.ScaleSampler("RandomResize", scale=[(50, 10), (50, 14)]), seed=9)
    img = np.zeros((48, 64, 3), np.uint8)
    monkeypatch.setattr(D.torch.cuda, "is_available", lambda: False)          # (pack: plain host memory here)
    a = p.pack([3, 7, 11], [img] * 3)
    b = p.pack([11, 20], [img] * 2)
    c = p.pack([7], [img])
    assert a.metas[2] == b.metas[0] and a.metas[1] == c.metas[0]
    e0 = [p.draw(i, epoch=0) for i in range(64)]
    e1 = [p.draw(i, epoch=1) for i in range(64)]
    assert e0 == [p.draw(i) for i in range(64)] and e0 != e1
    assert any(x[0] != y[0] for x, y in zip(e0, e1)) and any(x[1] != y[1] for x, y in zip(e0, e1))
    p.set_epoch(1)
    assert p.pack([3, 7, 11], [img] * 3, epoch=0).metas == a.metas        # an explicit epoch wins over the pipeline's current one
    assert [p.draw(i) for i in range(64)] == e1


def test_packed_batch_layout(monkeypatch):
    """records at the head, images at 16-byte aligned offsets behind them, record fields = the C struct's"""
    import ctypes as C
    from erd_amd import _lib, datasets as D
    monkeypatch.setattr(D.torch.cuda, "is_available", lambda: False)
    assert D.RESIZE_ITEM.itemsize == C.sizeof(_lib.ResizeItem) == 32
    for name, _ in _lib.ResizeItem._fields_:
        assert D.RESIZE_ITEM.fields[name][1] == getattr(_lib.ResizeItem, name).offset, name
    rng = np.random.RandomState(0)
    imgs = [rng.randint(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((5, 7), (1, 3), (9, 2))]
    pb = D.pack_images(imgs, [(10, 14, True), (2, 6, False), (9, 2, True)])
    host = pb.buf.numpy()
    rec = host[:3 * 32].view(D.RESIZE_ITEM)
    end = 96
    for k, im in enumerate(imgs):
        o = int(rec["offset"][k])
        assert o % 16 == 0 and o >= end
        assert np.array_equal(host[o:o + im.size].reshape(im.shape), im)
        end = o + im.size
    assert end <= host.size
    assert rec["sh"].tolist() == [5, 1, 9] and rec["sw"].tolist() == [7, 3, 2] and rec["nh"].tolist() == [10, 2, 9]
    assert rec["nw"].tolist() == [14, 6, 2] and rec["flip"].tolist() == [1, 0, 1]
    assert pb.metas == [(5, 7, 10, 14, True), (1, 3, 2, 6, False), (9, 2, 9, 2, True)]
    with pytest.raises(ValueError):
        D.pack_images([np.zeros((4, 4), np.uint8)], [(4, 4, False)])


def test_train_data_from_cfg_reads_the_pipeline(tmp_path):
    from erd_amd import Config
    from erd_amd.runner import CocoTrainData
    ds = dict(images=[dict(id=i, file_name=f"{i}.png", width=64, height=48) for i in range(5)],
              annotations=[dict(id=i + 1, image_id=i, category_id=1, bbox=[1.0, 1.0, 20.0, 20.0], area=400.0, iscrowd=0) for i in range(5)],
              categories=[dict(id=1, name="a")])
    json.dump(ds, open(tmp_path / "ann.json", "w"))
    base = dict(data_root=str(tmp_path), ann_file="ann.json", data_prefix=dict(img=""), metainfo=dict(classes=("a",)),
                filter_cfg=dict(filter_empty_gt=True, min_size=0))
    ms = LOAD + [dict(type="RandomResize", scale=[(50, 10), (50, 14)], keep_ratio=True), dict(type="RandomFlip", prob=0.25)] + PACK
    d = CocoTrainData.from_cfg(dict(train_dataloader=dict(batch_size=3, num_workers=2, dataset=dict(base, pipeline=ms))), rank=0, world=1)
    assert d.bs == 3 and d.num_workers == 2 and d.pipe.flip_prob == 0.25 and d.pipe.scale_sampler.type == "RandomResize"
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "gfl_increment", "gfl_r50_fpn_1x_coco_first_40_incre_last_40_cats.py"))
    cfg.merge_from_dict({"train_dataloader.dataset.data_root": str(tmp_path) + "/", "train_dataloader.dataset.ann_file": "ann.json",
                         "train_dataloader.dataset.metainfo": dict(classes=("a",))})
    d = CocoTrainData.from_cfg(cfg)
    assert d.pipe.scale == (1333, 800) and d.pipe.scale_sampler is None and d.pipe.flip_prob == 0.5 and d.bs == 2
    with pytest.raises(ValueError, match="Pad"):
        CocoTrainData.from_cfg(dict(train_dataloader=dict(batch_size=2, dataset=dict(base, pipeline=ms + [dict(type="Pad", size=(8, 8))]))))


HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_batch_resize_kernel_rounds_product_and_difference_separately(tmp_path):
    """resize_normalize_batch_kernel computes datasets.linear_coeffs on the device: f = float((d + 0.5) * scale - 0.5) is TWO rounded
    double operations there (numpy evaluates them one array operation after the other).  A compiler that contracts them emits
    v_fma_f64 ..., -0.5, which is another function -- so the ISA is checked: per instantiation five multiply / add(-0.5) pairs
    (one y, four x), no fused form, no scratch, no LDS."""
    out = tmp_path / "elementwise.s"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-function", "-S", "--cuda-device-only",
                        "-o", str(out), "elementwise.hip"], cwd=os.path.join(ROOT, "erd_amd", "csrc"), capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    s = open(out).read()
    seen = 0
    for m in re.finditer(r"^(_Z\S+):[^\n]*\n(.*?)^\s*\.end_amdhsa_kernel", s, re.S | re.M):
        name, body = m.group(1), m.group(2)
        if "resize_normalize_batch_kernel" not in name:
            continue
        seen += 1
        f64 = [t.strip() for t in body.split("\n") if re.match(r"\s*v_\w*f64", t)]
        assert not [t for t in f64 if re.match(r"v_fma\w*_f64", t) and t.rstrip().endswith("-0.5")], name
        pairs = sum(1 for a, b in zip(f64, f64[1:]) if a.startswith("v_mul_f64") and b.startswith("v_add_f64") and b.endswith("-0.5"))
        assert pairs == 5, (name, pairs)
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)) == 0, name
        assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body).group(1)) == 0, name
    assert seen == 2, seen          # float4 rows / element-wise rows
