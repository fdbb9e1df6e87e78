"""Test helper: the test-time-augmentation merge (DetTTAModel._merge_single_sample: bbox_flip + batched_nms, NMS restated
from mmcv's published algorithm, UNPINNED vs mmcv) on the host, in torch fp32 with the arithmetic erd_tta_merge uses, and
the seeded inputs of fixture F12 (tests/golden/f12_tta_merge_unpinned_nms.npz, written by tools/gen_tta_golden.py)."""
import numpy as np
import torch

F12_CASES = (
    # V views (flip flags), N images, P rows per view, original widths / heights, IoU, max_per_img
    dict(flips=(1, 0), N=3, P=20, ori=((120, 150), (90, 64), (200, 100)), iou=0.5, max_per_img=100),
    dict(flips=(1, 0, 1, 0, 1, 0), N=2, P=30, ori=((150, 117), (64, 201)), iou=0.6, max_per_img=10),
    dict(flips=(0, 1), N=2, P=8, ori=((80, 96), (100, 100)), iou=0.5, max_per_img=100, ties=True),
)


def f12_inputs(case: int, seed: int = 12):
    """(dets [V,N,P,5] f32, labels [V,N,P] i64, num [V,N] i32, flips, ori_w [N], iou, max_per_img) of one F12 case.
    Each view holds its rows score-descending (erd_predict_nms's order); boxes come from a few clusters per image so
    that rows of different views overlap; case 0: image 1 has an empty view 1 and image 2 has no detection at all;
    case 2: equal scores across views and mirrored copies of view 0's boxes in view 1."""
    c = F12_CASES[case]
    rng = np.random.RandomState(seed + case)
    V, N, P = len(c["flips"]), c["N"], c["P"]
    dets = np.zeros((V, N, P, 5), np.float32)
    labels = np.zeros((V, N, P), np.int64)
    num = np.zeros((V, N), np.int32)
    for n, (w, h) in enumerate(c["ori"]):
        centres = rng.uniform([8, 8], [w - 8, h - 8], (3, 2))
        for v in range(V):
            m = int(rng.randint(P // 2, P + 1))
            if case == 0 and (n == 2 or (n == 1 and v == 1)):
                m = 0
            k = rng.randint(0, 3, m)
            cx = centres[k, 0] + rng.uniform(-6, 6, m)
            cy = centres[k, 1] + rng.uniform(-6, 6, m)
            bw, bh = rng.uniform(6, 30, m), rng.uniform(6, 30, m)
            b = np.stack([np.clip(cx - bw / 2, 0, w), np.clip(cy - bh / 2, 0, h),
                          np.clip(cx + bw / 2, 0, w), np.clip(cy + bh / 2, 0, h)], 1).astype(np.float32)
            s = rng.uniform(0.05, 1.0, m).astype(np.float32)
            lab = rng.randint(0, 3, m)
            if c.get("ties"):
                s = rng.choice(np.array([0.25, 0.5, 0.75], np.float32), m)
                if v == 1:                       # view 0's boxes again, with the same labels and scores
                    m = num[0, n]
                    b, s, lab = dets[0, n, :m, :4].copy(), dets[0, n, :m, 4].copy(), labels[0, n, :m].copy()
            if c["flips"][v]:                    # the detections of a flipped view live in the mirrored frame
                b = np.stack([np.float32(w) - b[:, 2], b[:, 1], np.float32(w) - b[:, 0], b[:, 3]], 1)
            o = np.argsort(-s, kind="stable")
            dets[v, n, :m, :4], dets[v, n, :m, 4], labels[v, n, :m] = b[o], s[o], lab[o]
            num[v, n] = m
    ori_w = [float(w) for w, _ in c["ori"]]
    return dets, labels, num, [bool(f) for f in c["flips"]], ori_w, c["iou"], c["max_per_img"]


def f12_metas(case: int):
    c = F12_CASES[case]
    return [[dict(ori_shape=(h, w), flip=bool(f), flip_direction="horizontal" if f else None) for (w, h) in c["ori"]]
            for f in c["flips"]]


def merge_image(dets, labels, num, flips, W: float, iou_thr: float, max_per_img: int, n: int):
    """one image: (boxes [k,4], scores [k], labels [k]) after the merge, in keep order"""
    dets, labels, num = torch.as_tensor(dets), torch.as_tensor(labels), torch.as_tensor(num)
    bs, ss, ls = [], [], []
    Wt = torch.tensor(float(W), dtype=torch.float32)
    for v in range(dets.shape[0]):
        m = int(num[v, n])
        b = dets[v, n, :m, :4].float()
        if flips[v]:
            b = torch.stack([Wt - b[:, 2], b[:, 1], Wt - b[:, 0], b[:, 3]], 1)
        bs.append(b)
        ss.append(dets[v, n, :m, 4].float())
        ls.append(labels[v, n, :m].long())
    b, s, l = torch.cat(bs), torch.cat(ss), torch.cat(ls)
    if b.shape[0] == 0:
        return b.reshape(0, 4), s, l
    offs = b.max() + torch.tensor(1.0)
    bo = b + (l.float() * offs)[:, None]
    order = torch.sort(s, descending=True, stable=True).indices
    r = bo[order]
    x1, y1, x2, y2 = r.unbind(1)
    area = (x2 - x1) * (y2 - y1)
    supp = torch.zeros(len(order), dtype=torch.bool)
    keep = []
    for i in range(len(order)):
        if supp[i]:
            continue
        keep.append(i)
        if len(keep) == max_per_img:
            break
        w = (torch.minimum(x2[i], x2[i + 1:]) - torch.maximum(x1[i], x1[i + 1:])).clamp(min=0)
        h = (torch.minimum(y2[i], y2[i + 1:]) - torch.maximum(y1[i], y1[i + 1:])).clamp(min=0)
        inter = w * h
        supp[i + 1:] |= inter / (area[i] + area[i + 1:] - inter) > iou_thr
    k = order[torch.tensor(keep, dtype=torch.long)]
    return b[k], s[k], l[k]


def merge(dets, labels, num, flips, ori_w, iou_thr: float, max_per_img: int):
    return [merge_image(dets, labels, num, flips, ori_w[n], iou_thr, max_per_img, n) for n in range(len(ori_w))]
