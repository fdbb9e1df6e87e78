"""Annotation side of the data pipeline: COCO json -> per-image records restricted to the
configured classes, the empty/min-size filter, aspect-ratio batching, category slicing for the 40+40 protocol.
Host-side integer / dictionary work only (the reference does this in Python too); pixels are decoded and resized
by `GpuDetPipeline` at the end of this file (decode on the host with PIL, everything else in ONE HIP kernel).

Reference: mmdet/datasets/coco.py:59-100 (load_data_list), :102-170 (parse_data_info), :172-212 (filter_data);
mmdet/datasets/samplers/batch_sampler.py:11-68; scripts/select_categories.py:21-64; pycocotools' COCO index
(getCatIds / getImgIds / getAnnIds semantics restated: dataset order everywhere).
"""
from __future__ import annotations

import json
import math
import os
import warnings
from collections import defaultdict
from typing import Dict, Iterable, Iterator, List, Optional, Sequence

import numpy as np
import torch

from .structures import DetDataSample, InstanceData


def select_categories(dataset: dict, start: int, end: int) -> dict:
    """scripts/select_categories.py:31-60: sort categories by id, keep those at positions [start, end), then the
    annotations of those categories and the images that still have at least one annotation (original order kept)."""
    cats = sorted(dataset["categories"], key=lambda c: c["id"])[start:end]
    ids = {c["id"] for c in cats}
    annos = [a for a in dataset["annotations"] if a["category_id"] in ids]
    img_ids = {a["image_id"] for a in annos}
    return dict(categories=cats, annotations=annos, images=[im for im in dataset["images"] if im["id"] in img_ids])


class CocoAnnotations:
    """what the reference keeps of a COCO annotation file after load_data_list + filter_data"""

    def __init__(self, ann_file, classes: Sequence[str], data_prefix: str = "", filter_empty_gt: bool = True,
                 min_size: int = 32, test_mode: bool = False):
        ds = json.load(open(ann_file)) if isinstance(ann_file, (str, os.PathLike)) else ann_file
        if classes is None:      # CocoDataset's default METAINFO lists all 80 names: every category of the file matches
            classes = [c["name"] for c in ds["categories"]]
        names = set(classes)
        # getCatIds(catNms=classes): ids in the FILE's category order, not in `classes` order (coco.py:69-72)
        self.cat_ids = [c["id"] for c in ds["categories"] if c["name"] in names]
        self.cat2label = {cid: i for i, cid in enumerate(self.cat_ids)}
        self.classes = tuple(classes)
        anns_of = defaultdict(list)
        cat_img_map = defaultdict(list)
        seen = set()
        for a in ds["annotations"]:
            if a["id"] in seen:
                raise AssertionError(f"Annotation ids in '{ann_file}' are not unique!")
            seen.add(a["id"])
            anns_of[a["image_id"]].append(a)
            cat_img_map[a["category_id"]].append(a["image_id"])
        self.data_list = [self._parse(im, anns_of.get(im["id"], []), data_prefix) for im in ds["images"]]
        if not test_mode:
            in_cat = set()
            for cid in self.cat_ids:
                in_cat |= set(cat_img_map.get(cid, []))
            self.data_list = [d for d in self.data_list
                              if not (filter_empty_gt and d["img_id"] not in in_cat) and
                              min(d["width"], d["height"]) >= min_size]

    def _parse(self, img: dict, anns: Iterable[dict], prefix: str) -> dict:
        W, H = img["width"], img["height"]
        inst = []
        for a in anns:
            if a.get("ignore", False):
                continue
            x1, y1, w, h = a["bbox"]
            iw = max(0, min(x1 + w, W) - max(x1, 0))
            ih = max(0, min(y1 + h, H) - max(y1, 0))
            if iw * ih == 0 or a["area"] <= 0 or w < 1 or h < 1 or a["category_id"] not in self.cat2label:
                continue
            inst.append(dict(bbox=[x1, y1, x1 + w, y1 + h], bbox_label=self.cat2label[a["category_id"]],
                             ignore_flag=1 if a.get("iscrowd", False) else 0))
        return dict(img_path=os.path.join(prefix, img["file_name"]), img_id=img["id"], height=H, width=W, instances=inst)

    def __len__(self):
        return len(self.data_list)

    def get_data_info(self, idx: int) -> dict:
        return self.data_list[idx]

    def data_sample(self, idx: int, scale_factor=(1.0, 1.0), flip: bool = False, img_shape=None, clip: bool = False) -> DetDataSample:
        """PackDetInputs for the annotation half: boxes of non-ignored instances scaled by (w_scale, h_scale) and
        optionally flipped horizontally inside img_shape (RandomFlip), ignored ones in `ignored_instances`."""
        d = self.data_list[idx]
        sw, sh = scale_factor
        shape = img_shape or (int(d["height"] * sh + 0.5), int(d["width"] * sw + 0.5))
        boxes = torch.tensor([i["bbox"] for i in d["instances"]], dtype=torch.float32).reshape(-1, 4)
        boxes = boxes * torch.tensor([sw, sh, sw, sh], dtype=torch.float32)
        if clip:           # Resize(clip_object_border=True): boxes clipped to the resized image
            boxes[:, 0::2].clamp_(0, shape[1])
            boxes[:, 1::2].clamp_(0, shape[0])
        if flip:
            x1 = shape[1] - boxes[:, 2]
            x2 = shape[1] - boxes[:, 0]
            boxes = torch.stack([x1, boxes[:, 1], x2, boxes[:, 3]], 1)
        labels = torch.tensor([i["bbox_label"] for i in d["instances"]], dtype=torch.int64)
        ign = torch.tensor([i["ignore_flag"] for i in d["instances"]], dtype=torch.bool)
        s = DetDataSample(metainfo=dict(img_id=d["img_id"], img_path=d["img_path"], ori_shape=(d["height"], d["width"]),
                                        img_shape=shape, scale_factor=(sw, sh), flip=flip))
        s.gt_instances = InstanceData(bboxes=boxes[~ign], labels=labels[~ign])
        s.ignored_instances = InstanceData(bboxes=boxes[ign], labels=labels[ign])
        return s


def rescale_size(old_wh, scale) -> tuple:
    """mmcv.image.rescale_size for a (long, short) target such as (1333, 800) with keep_ratio: the largest factor
    that keeps the long edge <= max(scale) and the short edge <= min(scale); new size = int(x * f + 0.5)."""
    w, h = old_wh
    f = min(max(scale) / max(h, w), min(scale) / min(h, w))
    return int(w * float(f) + 0.5), int(h * float(f) + 0.5)


class AspectRatioBatchSampler:
    """batch_sampler.py:11-68: indices from `sampler` are bucketed by (width < height); a bucket is emitted when it
    reaches batch_size; leftovers of both buckets are concatenated (portrait first) and chunked at the end."""

    def __init__(self, sampler: Iterable[int], dataset: CocoAnnotations, batch_size: int, drop_last: bool = False):
        if not isinstance(batch_size, int) or batch_size <= 0:
            raise ValueError(f"batch_size should be a positive integer value, but got batch_size={batch_size}")
        self.sampler, self.dataset, self.batch_size, self.drop_last = sampler, dataset, batch_size, drop_last

    def __iter__(self) -> Iterator[List[int]]:
        buckets = [[], []]
        for idx in self.sampler:
            d = self.dataset.get_data_info(idx)
            b = buckets[0 if d["width"] < d["height"] else 1]
            b.append(idx)
            if len(b) == self.batch_size:
                yield b[:]
                del b[:]
        left = buckets[0] + buckets[1]
        while left:
            if len(left) <= self.batch_size:
                if not self.drop_last:
                    yield left[:]
                left = []
            else:
                yield left[:self.batch_size]
                left = left[self.batch_size:]

    def __len__(self) -> int:
        n = len(self.sampler)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size


# ---------------------------------------------------------------------------------------------------------
# image side: LoadImageFromFile -> Resize(scale=(1333, 800), keep_ratio=True) -> RandomFlip(0.5) -> PackDetInputs ->
# DetDataPreprocessor (configs/gfl_increment/*:13-19, data_preprocessor.py:110-183).  Decode stays on the host (PIL; the
# reference decodes with cv2 on the host too); resize + flip + normalise + pad are one kernel over the padded batch
# (erd_resize_normalize_batch: one launch per training batch; erd_resize_normalize per image for test-time views).  cv2's 8-bit bilinear resize is restated (resize.cpp: half-pixel centres, 11-bit fixed-point
# weights, two-pass rounding) -- UNPINNED against cv2, which is not in this image.
# ---------------------------------------------------------------------------------------------------------
def linear_coeffs(src: int, dst: int):
    """per output index along one axis: source index (int32) and the two fixed-point weights (int16, sum 2048)"""
    scale = 1.0 / (float(dst) / float(src))
    f = ((np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int32)
    f = f - s.astype(np.float32)
    lo, hi = s < 0, s >= src - 1
    f[lo], s[lo] = 0.0, 0
    f[hi], s[hi] = 0.0, src - 1
    c1 = np.rint(f.astype(np.float64) * 2048.0)
    c0 = np.rint((1.0 - f).astype(np.float32).astype(np.float64) * 2048.0)
    return s, np.stack([c0, c1], 1).astype(np.int16)


def load_image_bgr(path: str) -> np.ndarray:
    """LoadImageFromFile: uint8 [h, w, 3] in BGR order (what cv2.imread hands the reference's pipeline)"""
    from PIL import Image
    with Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])


def prefetch_map(fn, items: Sequence, workers: int, depth: int):
    """yield fn(item) for every item IN ORDER while up to `depth` later items are already being computed on `workers`
    threads (the DataLoader's num_workers / prefetch_factor, as threads: image decoding releases the GIL).  workers <= 0:
    plain serial map.  An exception in fn surfaces at the position of its item."""
    if workers <= 0:
        for it in items:
            yield fn(it)
        return
    from collections import deque
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=workers, thread_name_prefix="erd-decode") as pool:
        pending = deque()
        it = iter(items)
        try:
            for _ in range(max(1, depth)):
                pending.append(pool.submit(fn, next(it)))
        except StopIteration:
            pass
        while pending:
            head = pending.popleft()
            try:
                pending.append(pool.submit(fn, next(it)))
            except StopIteration:
                pass
            try:
                yield head.result()
            except BaseException:
                for f in pending:
                    f.cancel()
                raise


def pinned(im: np.ndarray):
    """page-locked copy of a decoded image when a GPU is present (so that the H2D copy is asynchronous)"""
    t = torch.from_numpy(im)
    return t.pin_memory() if torch.cuda.is_available() else t


# one record of erd_resize_normalize_batch (include/erd_hip.h erd_resize_item, _lib.ResizeItem): 32 bytes
RESIZE_ITEM = np.dtype([("offset", "<i8"), ("sh", "<i4"), ("sw", "<i4"), ("nh", "<i4"), ("nw", "<i4"), ("flip", "<i4"),
                        ("reserved", "<i4")])


class PackedBatch:
    """host half of a batch as ONE buffer: the records {offset, sh, sw, nh, nw, flip} at its head, then the decoded uint8 HWC
    images back to back at 16-byte aligned offsets.  `buf` is page-locked when a GPU is present, so the single host-to-device
    copy of `assemble` is asynchronous.  `metas[k]` = (sh, sw, nh, nw, flip) of image k, as Python ints / bool."""

    def __init__(self, buf: torch.Tensor, metas: list):
        self.buf, self.metas = buf, metas

    def __len__(self):
        return len(self.metas)


def pack_images(imgs: Sequence, metas: Sequence[tuple]) -> PackedBatch:
    """imgs: decoded [h,w,3] uint8 arrays (or CPU tensors); metas: (nh, nw, flip) per image"""
    n = len(imgs)
    arrs = [(im.numpy() if isinstance(im, torch.Tensor) else np.asarray(im)) for im in imgs]
    offs, pos = [], -(-n * RESIZE_ITEM.itemsize // 16) * 16
    for a in arrs:
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
            raise ValueError(f"decoded images are uint8 [h, w, 3], got {a.dtype} {a.shape}")
        offs.append(pos)
        pos += -(-a.size // 16) * 16
    buf = torch.empty(pos, dtype=torch.uint8, pin_memory=torch.cuda.is_available())      # torch's pinned allocator, as pinned()
    host = buf.numpy()
    rec = host[:n * RESIZE_ITEM.itemsize].view(RESIZE_ITEM)
    full = []
    for k, (a, o, (nh, nw, flip)) in enumerate(zip(arrs, offs, metas)):
        host[o:o + a.size] = a.reshape(-1)
        rec[k] = (o, a.shape[0], a.shape[1], nh, nw, int(bool(flip)), 0)
        full.append((int(a.shape[0]), int(a.shape[1]), int(nh), int(nw), bool(flip)))
    return PackedBatch(buf, full)


class ScaleSampler:
    """the target scale of one image, drawn from that image's own generator AFTER its flip draw.  The rules restate mmcv 2.x
    transforms/processing.py (RandomResize._random_sample / _random_sample_ratio, RandomChoiceResize._random_select) --
    UNPINNED: mmcv is not part of this project's test oracle.
      Resize(scale):                              the scale, no draw
      RandomResize(scale=[(a, b), (c, d)]):       (randint(min(a, c), max(a, c) + 1), randint(min(b, d), max(b, d) + 1)), in that order
      RandomResize(scale=(a, b), ratio_range):    r = random_sample() * (hi - lo) + lo; (int(a * r), int(b * r))
      RandomChoiceResize(scales):                 scales[randint(len(scales))]"""

    def __init__(self, type: str = "Resize", scale=None, ratio_range=None, scales=None):
        self.type = type
        if type == "Resize":
            self.scale = _scale2(scale)
        elif type == "RandomResize" and ratio_range is not None:
            self.scale, self.ratio_range = _scale2(scale), (float(ratio_range[0]), float(ratio_range[1]))
            if not 0 < self.ratio_range[0] <= self.ratio_range[1]:
                raise ValueError(f"RandomResize: ratio_range {ratio_range} is not 0 < lo <= hi")
        elif type == "RandomResize":
            if not isinstance(scale, (list, tuple)) or len(scale) != 2:
                raise ValueError(f"RandomResize: scale is two (w, h) tuples or one with ratio_range, got {scale}")
            self.scale, self.ratio_range = (_scale2(scale[0]), _scale2(scale[1])), None
        elif type == "RandomChoiceResize":
            if not isinstance(scales, (list, tuple)) or not scales:
                raise ValueError(f"RandomChoiceResize: scales is a non-empty list of (w, h), got {scales}")
            self.scales = [_scale2(s) for s in scales]
        else:
            raise ValueError(f"resize stage {type!r} is not built")

    def __call__(self, rng: np.random.RandomState) -> tuple:
        if self.type == "Resize":
            return self.scale
        if self.type == "RandomChoiceResize":
            return self.scales[rng.randint(len(self.scales))]
        if self.ratio_range is not None:
            lo, hi = self.ratio_range
            r = rng.random_sample() * (hi - lo) + lo
            return int(self.scale[0] * r), int(self.scale[1] * r)
        (a, b), (c, d) = self.scale
        e0 = rng.randint(min(a, c), max(a, c) + 1)
        e1 = rng.randint(min(b, d), max(b, d) + 1)
        return int(e0), int(e1)

    def __repr__(self):
        return "ScaleSampler(%s)" % ", ".join(f"{k}={v!r}" for k, v in vars(self).items())


def _scale2(s) -> tuple:
    if not isinstance(s, (list, tuple)) or len(s) != 2 or not all(isinstance(v, (int, np.integer)) and v > 0 for v in s):
        raise ValueError(f"a scale is (w, h) in positive integers, got {s!r}")
    return int(s[0]), int(s[1])


class GpuDetPipeline:
    """one training batch from image indices: decoded images -> normalised, padded [N,3,H,W] fp32 on the GPU + data
    samples with resized / flipped / clipped boxes.  Deterministic given `seed`: image `index` of `epoch` has its own
    generator, whose first draw is the flip and whose later draws (if any) are the scale -- whichever batch it falls into."""

    def __init__(self, annotations: CocoAnnotations, scale=(1333, 800), flip_prob: float = 0.5, mean=(123.675, 116.28, 103.53),
                 std=(58.395, 57.12, 57.375), bgr_to_rgb: bool = True, pad_size_divisor: int = 32, pad_value: float = 0.0,
                 seed: int = 0, loader=load_image_bgr, device="cuda", scale_sampler: Optional[ScaleSampler] = None):
        """scale_sampler: a per-image scale (RandomResize / RandomChoiceResize); None = the fixed `scale`"""
        self.ann, self.scale, self.flip_prob = annotations, tuple(scale), flip_prob
        self.scale_sampler = scale_sampler
        self.mean = [float(np.float32(v)) for v in mean]
        self.std = [float(np.float32(v)) for v in std]
        self.swap, self.div, self.pad_value, self.seed = bgr_to_rgb, pad_size_divisor, pad_value, seed
        self.loader, self.device = loader, torch.device(device)
        self._tables: Dict[tuple, tuple] = {}
        self.epoch = 0

    def set_epoch(self, epoch: int) -> None:
        self.epoch = epoch

    def _table(self, sh, sw, nh, nw):
        key = (sh, sw, nh, nw)
        if key not in self._tables:
            xo, xc = linear_coeffs(sw, nw)
            yo, yc = linear_coeffs(sh, nh)
            self._tables[key] = tuple(torch.from_numpy(a).to(self.device) for a in (xo, xc, yo, yc))
        return self._tables[key]

    def decode(self, indices: Sequence[int]) -> List[np.ndarray]:
        """host half of a batch (LoadImageFromFile): safe to run on worker threads, PIL releases the GIL while decoding"""
        return [self.loader(self.ann.get_data_info(i)["img_path"]) for i in indices]

    def draw(self, index: int, epoch: Optional[int] = None) -> tuple:
        """(flip, scale) of image `index` in `epoch`: the flip is the generator's FIRST draw (so fixed-scale runs flip as they
        always did), the scale draws follow it"""
        epoch = self.epoch if epoch is None else epoch
        rng = np.random.RandomState((self.seed * 1000003 + epoch * 7919 + int(index)) % (2 ** 31 - 1))
        flip = bool(rng.rand() < self.flip_prob)
        return flip, (self.scale if self.scale_sampler is None else tuple(self.scale_sampler(rng)))

    def pack(self, indices: Sequence[int], imgs: Optional[Sequence[np.ndarray]] = None, epoch: Optional[int] = None) -> PackedBatch:
        """host half of a batch, ready for ONE copy and ONE launch: decode (unless `imgs` is given), draw flip and scale per
        image, pack pixels and records into one page-locked buffer.  Safe on worker threads."""
        imgs = self.decode(indices) if imgs is None else imgs
        metas = []
        for i, im in zip(indices, imgs):
            flip, scale = self.draw(i, epoch)
            nw, nh = rescale_size((im.shape[1], im.shape[0]), scale)
            metas.append((nh, nw, flip))
        return pack_images(imgs, metas)

    def batch(self, indices: Sequence[int]):
        return self.assemble(indices, self.decode(indices))

    def assemble(self, indices: Sequence[int], imgs):
        """device half: one host-to-device copy, one resize / flip / normalise / pad launch over the whole batch
        (erd_resize_normalize_batch: bit-identical to one erd_resize_normalize launch per image) + the data samples.
        imgs: what `pack` returned, or the decoded images themselves (packed here)."""
        from . import kernels as K
        packed = imgs if isinstance(imgs, PackedBatch) else self.pack(indices, imgs)
        if len(packed) != len(indices):
            raise ValueError(f"{len(indices)} indices for a packed batch of {len(packed)}")
        H = max(int(math.ceil(nh / self.div)) * self.div for _, _, nh, _, _ in packed.metas)
        W = max(int(math.ceil(nw / self.div)) * self.div for _, _, _, nw, _ in packed.metas)
        out = torch.empty((len(packed), 3, H, W), dtype=torch.float32, device=self.device)
        K.resize_normalize_batch(packed.buf.to(self.device, non_blocking=True), len(packed), out, self.mean, self.std, self.swap,
                                 self.pad_value)
        samples = []
        for i, (sh, sw, nh, nw, flip) in zip(indices, packed.metas):
            s = self.ann.data_sample(i, scale_factor=(nw / sw, nh / sh), flip=flip, img_shape=(nh, nw), clip=True)
            s.set_metainfo(dict(pad_shape=(H, W), batch_input_shape=(H, W)))
            samples.append(s)
        return out, samples

    def assemble_tta(self, indices: Sequence[int], imgs: Sequence[np.ndarray], scales, flips):
        """TestTimeAug of one decoded batch: the views (scale s, flip f) of the N images in product order, scale
        outermost -- the order DetTTAModel merges them in.  Each image goes to the device once; the views of one scale
        share one padded [len(flips)*N,3,H,W] batch, view f being rows f*N..(f+1)*N-1.
        Returns [(inputs [N,3,H,W], data samples)] per view."""
        from . import kernels as K
        N = len(imgs)
        srcs = [(im if isinstance(im, torch.Tensor) else torch.from_numpy(im)).to(self.device, non_blocking=True)
                for im in imgs]
        views = []
        for scale in scales:
            new = [rescale_size((im.shape[1], im.shape[0]), tuple(scale)) for im in imgs]          # (w, h)
            H = max(int(math.ceil(h / self.div)) * self.div for _, h in new)
            W = max(int(math.ceil(w / self.div)) * self.div for w, _ in new)
            out = torch.empty((len(flips) * N, 3, H, W), dtype=torch.float32, device=self.device)
            for f, flip in enumerate(flips):
                samples = []
                for k, (i, im, (nw, nh)) in enumerate(zip(indices, imgs, new)):
                    K.resize_normalize_into(srcs[k], self._table(im.shape[0], im.shape[1], nh, nw), (nh, nw), out[f * N + k],
                                            self.mean, self.std, bool(flip), self.swap, self.pad_value)
                    s = self.ann.data_sample(i, scale_factor=(nw / im.shape[1], nh / im.shape[0]), flip=bool(flip),
                                             img_shape=(nh, nw), clip=True)
                    s.set_metainfo(dict(pad_shape=(H, W), batch_input_shape=(H, W),
                                        flip_direction="horizontal" if flip else None))
                    samples.append(s)
                views.append((out[f * N:(f + 1) * N], samples))
        return views


DEFAULT_TTA_MODEL = dict(type="DetTTAModel", tta_cfg=dict(nms=dict(type="nms", iou_threshold=0.5), max_per_img=100))


def _test_dataset_cfg(cfg) -> dict:
    d = cfg["test_dataloader"]["dataset"]
    while "dataset" in d:
        d = d["dataset"]
    return d


def _resize_scale(t: dict) -> tuple:
    if not t.get("keep_ratio", False) or t.get("scale") is None or len(t["scale"]) != 2:
        raise ValueError(f"--tta: only Resize(scale=(w, h), keep_ratio=True) is built, got {dict(t)}")
    return tuple(int(v) for v in t["scale"])


def _flip_of(t: dict) -> bool:
    prob, direction = t.get("prob"), t.get("direction", "horizontal")
    if direction != "horizontal" or prob not in (0, 1):
        raise ValueError(f"--tta: only RandomFlip(prob=1.) / RandomFlip(prob=0.), horizontal, is built, got {dict(t)}")
    return bool(prob == 1)


def resolve_tta(cfg) -> dict:
    """tools/test.py --tta (reference tools/test.py:93-120): the config's `tta_model` / `tta_pipeline`, or the flip-only
    defaults (with the reference's warnings) at the scale of the test pipeline's Resize.  The pipeline is read, not run:
    a TestTimeAug whose lists are Resize(keep_ratio=True) scales and RandomFlip probs 1 / 0 (configs/retinanet/
    retinanet_tta.py's form), around LoadImageFromFile / LoadAnnotations / PackDetInputs.  Anything else raises.
    Returns dict(tta_model=..., scales=[(w, h), ...], flips=[bool, ...]); the views are their product, scale outermost."""
    tta_model = cfg.get("tta_model")
    if tta_model is None:
        warnings.warn("Cannot find ``tta_model`` in config, we will set it as default.")
        tta_model = DEFAULT_TTA_MODEL
    tta_model = json.loads(json.dumps(tta_model))                  # plain dicts, the config stays untouched
    if tta_model.get("type") != "DetTTAModel":
        raise ValueError(f"--tta: tta_model type {tta_model.get('type')!r} is not built (DetTTAModel is)")
    test_resize = [t for t in _test_dataset_cfg(cfg).get("pipeline", []) if t.get("type") == "Resize"]
    base = _resize_scale(test_resize[0]) if test_resize else (1333, 800)
    pipeline = cfg.get("tta_pipeline")
    if pipeline is None:
        warnings.warn("Cannot find ``tta_pipeline`` in config, we will set it as default.")
        return dict(tta_model=tta_model, scales=[base], flips=[True, False])
    scales, flips, outer, tta = None, None, None, False
    for t in pipeline:
        kind = t.get("type")
        if kind in ("LoadImageFromFile", "LoadAnnotations", "PackDetInputs"):
            continue
        if kind == "Resize" and not tta:
            outer = _resize_scale(t)
        elif kind == "TestTimeAug" and not tta:
            tta = True
            for group in t["transforms"]:
                kinds = {g.get("type") for g in group}
                if kinds == {"Resize"}:
                    if scales is not None or outer is not None:
                        raise ValueError("--tta: more than one Resize stage in tta_pipeline")
                    scales = [_resize_scale(g) for g in group]
                elif kinds == {"RandomFlip"}:
                    if flips is not None:
                        raise ValueError("--tta: more than one RandomFlip stage in tta_pipeline")
                    flips = [_flip_of(g) for g in group]
                elif not kinds or not kinds <= {"LoadAnnotations", "PackDetInputs"}:
                    raise ValueError(f"--tta: TestTimeAug transform list {sorted(map(str, kinds))} is not built "
                                     "(Resize(keep_ratio=True) scales and RandomFlip probs 1 / 0 are)")
        else:
            raise ValueError(f"--tta: tta_pipeline transform {kind!r} is not built")
    if not tta:
        raise ValueError("--tta: tta_pipeline has no TestTimeAug")
    return dict(tta_model=tta_model, scales=scales or [outer or base], flips=flips or [False])


# ---------------------------------------------------------------------------------------------------------
# the train pipeline of a config, read (not run) -- the training twin of resolve_tta
# ---------------------------------------------------------------------------------------------------------
_RESIZE_KINDS = ("Resize", "RandomResize", "RandomChoiceResize")
_RESIZE_KEYS = {"Resize": {"scale"}, "RandomResize": {"scale", "ratio_range"}, "RandomChoiceResize": {"scales"}}


def _plain(t) -> dict:
    return t.to_dict() if hasattr(t, "to_dict") else dict(t)


def _train_resize(t: dict) -> ScaleSampler:
    kind = t["type"]
    if t.get("keep_ratio", False) is not True:
        raise ValueError(f"train pipeline: {kind} is built with keep_ratio=True only, got {t}")
    if t.get("clip_object_border", True) is not True or t.get("interpolation", "bilinear") != "bilinear" \
            or t.get("backend", "cv2") != "cv2" or t.get("resize_type", "Resize") != "Resize":
        raise ValueError(f"train pipeline: {kind} is built with bilinear cv2 interpolation and clipped boxes only, got {t}")
    extra = set(t) - {"type", "keep_ratio", "clip_object_border", "interpolation", "backend", "resize_type"} - _RESIZE_KEYS[kind]
    if extra:
        raise ValueError(f"train pipeline: {kind} arguments {sorted(extra)} are not built")
    try:
        return ScaleSampler(kind, **{k: t[k] for k in _RESIZE_KEYS[kind] if t.get(k) is not None})
    except (ValueError, TypeError) as e:
        raise ValueError(f"train pipeline: {kind}: {e}") from None


def _train_flip(t: dict) -> float:
    prob, direction = t.get("prob"), t.get("direction", "horizontal")
    if direction != "horizontal":
        raise ValueError(f"train pipeline: RandomFlip is built for direction='horizontal' only, got {t}")
    if prob is None:
        return 0.0
    if isinstance(prob, bool) or not isinstance(prob, (int, float)) or not 0 <= prob <= 1:
        raise ValueError(f"train pipeline: RandomFlip prob is one number in [0, 1], got {t}")
    return float(prob)


def resolve_train_pipeline(pipeline) -> dict:
    """`train_dataloader.dataset.pipeline` -> dict(sampler=ScaleSampler, flip_prob=float): what GpuDetPipeline does for it.
    Accepted: LoadImageFromFile, LoadAnnotations(with_bbox=True), PackDetInputs, exactly ONE resize stage (Resize /
    RandomResize with two scales or a ratio_range / RandomChoiceResize, each keep_ratio=True) and at most one
    RandomFlip(prob=p, direction='horizontal') (absent or prob=None: no flip).  Anything else raises ValueError naming the
    transform -- a pipeline this path cannot perform must not train as something else."""
    sampler, flip = None, None
    for t in pipeline or []:
        t = _plain(t)
        kind = t.get("type")
        if kind in ("LoadImageFromFile", "PackDetInputs"):
            continue
        if kind == "LoadAnnotations":
            if t.get("with_bbox", True) is not True or any(t.get(k) for k in ("with_mask", "with_seg", "with_keypoints")):
                raise ValueError(f"train pipeline: LoadAnnotations is built for with_bbox=True alone, got {t}")
        elif kind in _RESIZE_KINDS:
            if sampler is not None:
                raise ValueError(f"train pipeline: a second resize stage ({kind}) is not built")
            sampler = _train_resize(t)
        elif kind == "RandomFlip":
            if flip is not None:
                raise ValueError("train pipeline: a second RandomFlip is not built")
            flip = _train_flip(t)
        else:
            raise ValueError(f"train pipeline: transform {kind!r} is not built")
    if sampler is None:
        raise ValueError("train pipeline: no resize stage (Resize, RandomResize or RandomChoiceResize with keep_ratio=True)")
    return dict(sampler=sampler, flip_prob=0.0 if flip is None else flip)
