"""Seeded synthetic COCO sets for the evaluator tests (tests/test_coco_eval_cpu.py, tests/test_gpu_coco_eval.py): ground truth with
crowd regions, `ignore` flags and annotation areas of exactly 32^2 and 96^2; detections near the ground truth and at random, with
scores on a coarse grid (ties within a pair and across images), zero-area and touching boxes, and pairs above 100 detections."""
import numpy as np


def make_gt(rng, n_img, cat_ids, gt_per_img=(1, 14), W=640, H=480, empty_cats=(), crowd_p=0.05, ignore_p=0.05):
    images = [dict(id=1000 + 7 * i, width=W, height=H, file_name=f"{i}.png") for i in range(n_img)]
    anns = []
    live = [c for c in cat_ids if c not in empty_cats]
    for im in images:
        for _ in range(rng.randint(gt_per_img[0], gt_per_img[1] + 1)):
            x, y = rng.uniform(0, W - 8), rng.uniform(0, H - 8)
            w, h = rng.uniform(2, min(300, W - x)), rng.uniform(2, min(300, H - y))
            area = float(w * h)
            u = rng.rand()
            if u < 0.05:
                area = 32.0 ** 2                                 # the inclusive bounds of the area ranges
            elif u < 0.10:
                area = 96.0 ** 2
            a = dict(id=len(anns) + 1, image_id=im["id"], category_id=int(live[rng.randint(len(live))]),
                     bbox=[float(x), float(y), float(w), float(h)], area=area, iscrowd=int(rng.rand() < crowd_p))
            if rng.rand() < ignore_p:
                a["ignore"] = 1
            anns.append(a)
    cats = [dict(id=int(c), name=f"c{c}") for c in sorted(cat_ids)]
    return dict(images=images, annotations=anns, categories=cats)


def make_dets(rng, gt, K, per_img=(0, 100), W=640, H=480, score_grid=50, no_det_cats=(), big_pair=False, cat_ids=None):
    """{image_id: (bboxes xyxy fp32 [n,4], scores fp32 [n], labels int64 [n])}; labels index cat_ids"""
    by_img = {}
    for a in gt["annotations"]:
        by_img.setdefault(a["image_id"], []).append(a)
    kpos = {c: k for k, c in enumerate(cat_ids)} if cat_ids is not None else None
    allowed = [k for k in range(K) if cat_ids is None or cat_ids[k] not in no_det_cats]
    out = {}
    for n, im in enumerate(gt["images"]):
        cnt = rng.randint(per_img[0], per_img[1] + 1)
        if n % 7 == 3:
            cnt = 0                                              # images with no detections
        boxes, labels = [], []
        for j in range(cnt):
            g = by_img.get(im["id"], [])
            if g and rng.rand() < 0.6:
                a = g[rng.randint(len(g))]
                x, y, w, h = a["bbox"]
                jit = rng.normal(0, 0.08, 4) * [w, h, w, h]
                b = [x + jit[0], y + jit[1], x + w + jit[2], y + h + jit[3]]
                k = kpos.get(a["category_id"], allowed[0]) if kpos is not None else rng.randint(K)
                if k not in allowed:
                    k = allowed[rng.randint(len(allowed))]
            else:
                x, y = rng.uniform(0, W - 4), rng.uniform(0, H - 4)
                b = [x, y, x + rng.uniform(1, 200), y + rng.uniform(1, 200)]
                k = allowed[rng.randint(len(allowed))]
            u = rng.rand()
            if u < 0.03:
                b[2], b[3] = b[0], b[1] + 5                      # zero area
            elif u < 0.06 and boxes:
                p = boxes[-1]
                b = [p[2], p[1], p[2] + 10, p[3]]                # touching the previous box
            boxes.append(b)
            labels.append(k)
        if big_pair and n == 1:
            for j in range(130):                                 # one pair above max(MAX_DETS)
                x, y = rng.uniform(0, W - 40), rng.uniform(0, H - 40)
                boxes.append([x, y, x + 30, y + 30])
                labels.append(allowed[0])
        m = len(boxes)
        scores = (rng.randint(1, score_grid + 1, m) / score_grid).astype(np.float32)
        out[im["id"]] = (np.asarray(boxes, dtype=np.float32).reshape(-1, 4), scores, np.asarray(labels, dtype=np.int64))
    return out
