"""Host references for the exact tests of erd_amd/csrc/predict.hip (tests/test_gpu_predict_exact.py, tests/test_predict_refs_cpu.py).

GPU expf differs from the host's, so a score-ordered selection on random logits cannot be compared exactly.  The inputs built here
remove that dependence instead of tolerating it:

* classification logits come from TABLE, fp32-exact values whose fp64 sigmoids are >= 128 fp32 ulps apart: the order of two
  entries cannot depend on the expf implementation, equal logits give equal keys, and the only rule left is the documented one --
  score descending, then (anchor, class) index ascending -- which is exact on the host too;
* box logits are one-hot (0 at one bin, -200 elsewhere): expf(-200) is 0 in fp32, the softmax is exactly (1, 0, ...), the Integral
  exactly the bin, and every distance and corner a small integer: decoded boxes are exact;
* the NMS runs in fp32 on both sides (predict.o is built without FMA contraction): O.nms_class_offset on fp32 tensors is the same
  IEEE sequence as pred_nms_kernel.

Nothing here reads the kernels' code: paths (`all`, `fit`, `tie`) follow from counts alone."""
import functools
from collections import namedtuple

import numpy as np
import torch

from oracle import erd_oracle as O

F32 = np.float32
INF = float("inf")
NAN = float("nan")

# ---------------------------------------------------------------------------------------------
# the score table
# ---------------------------------------------------------------------------------------------
TABLE = np.array(sorted([-6 + 0.5 * i for i in range(25)] + [i / 8 for i in range(1, 4)] +
                        [j * 2.0 ** -15 for j in range(1, 9)] + [-3 + j * 2.0 ** -12 for j in range(1, 9)]), np.float64)
P2_GROUP = [0.0] + [j * 2.0 ** -15 for j in range(1, 8)]          # share the top 22 key bits: told apart in radix pass 2
P1_GROUP = [-3.0] + [-3 + j * 2.0 ** -12 for j in range(1, 9)]    # share the top 11 key bits only: told apart in pass 1
P0_GROUP = [-2.0, -1.5, -1.0, -0.5]                               # four different top-11 buckets: told apart in pass 0
THR_MID = float(F32(0.05))                                               # between sigmoid(-3 + 8/4096) and sigmoid(-2.5)
THR_P2 = float(F32(0.5 + 2.0 ** -18))                             # 64 ulps above sigmoid(0), 64 below sigmoid(2^-15)
THRESHOLDS = (0.0, THR_MID, THR_P2)
SCORE_ULPS = 63                                                   # half the table's separation, minus one
BELOW_MID = [-6.0, -5.0, -4.0, -3.5, -3.0, -3 + 2.0 ** -12]       # fillers under THR_MID
NEVER = [-INF, NAN]                                               # fillers under every threshold, 0.0 included


def score64(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def score32(x):
    """the fp64 sigmoid rounded to fp32: what a correctly rounded fp32 sigmoid returns"""
    return score64(x).astype(F32)


def key_of(s):
    return np.asarray(s, F32).view(np.uint32).astype(np.int64)


def ulps(a, b):
    """distance of two non-negative fp32 values in units in the last place"""
    return np.abs(key_of(a) - key_of(b))


def table_separation_ulps():
    k = key_of(score32(TABLE))
    return int(np.diff(k).min())


def threshold_distance_ulps(thr):
    return int(np.abs(key_of(score32(TABLE)) - int(key_of(thr))).min())


# ---------------------------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------------------------
STRIDES = (8, 16, 32, 64, 128)
LV5 = ((9, 13), (5, 7), (3, 4), (2, 2), (1, 1))                   # 117 + 35 + 12 + 4 + 1 anchors
LV65 = ((5, 13), (9, 13), (3, 4), (2, 2), (1, 1))                 # a 65-anchor level: one full scan block plus one row


def _spec(spec, nel):
    if isinstance(spec, int):
        return [(spec, (0, nel))]
    if isinstance(spec, tuple):
        return [spec]
    return list(spec)


def build_level(rng, cnt, C, recipe, filler):
    """[cnt, C] fp32 logits: each recipe entry {logit: count | (count, (lo, hi)) | [(count, (lo, hi)), ...]} scattered at seeded
    free positions (of its flat-index range, ranged entries first), the rest drawn from `filler`."""
    nel = cnt * C
    out = np.empty(nel, F32)
    free = np.ones(nel, bool)
    items = [(lg, c, r) for lg, sp in recipe.items() for c, r in _spec(sp, nel)]
    for lg, c, (lo, hi) in sorted(items, key=lambda it: it[2][1] - it[2][0]):
        assert float(F32(lg)) == lg or lg == INF, lg
        pos = np.flatnonzero(free[lo:hi]) + lo
        assert len(pos) >= c, (lg, c, lo, hi, len(pos))
        pick = rng.choice(pos, c, replace=False) if c else pos[:0]
        out[pick] = lg
        free[pick] = False
    rest = np.flatnonzero(free)
    if len(rest):
        out[rest] = rng.choice(np.asarray(filler, F32), len(rest))
    return out.reshape(cnt, C)


def build_box_logits(bins):
    """[A, 4] integer bins -> [A, 68] one-hot logits (0 at the bin, -200 elsewhere)"""
    z = np.full(bins.shape + (17,), -200.0, F32)
    np.put_along_axis(z, bins[..., None], 0.0, -1)
    return z.reshape(bins.shape[0], 68)


def level_offsets(sizes):
    off = [0]
    for h, w in sizes:
        off.append(off[-1] + h * w)
    return off


def anchor_centres(sizes):
    return O.anchor_centers(torch.cat(O.grid_anchors(list(sizes), STRIDES[:len(sizes)]))).numpy().astype(np.float64)


def build_inputs(case):
    """a case -> cls [N, A, C], bbox [N, A, 68] (fp32 numpy, level-concatenated), bins [N, A, 4], img_hw [N, 2]"""
    sizes, C, N = case["sizes"], case["C"], len(case["recipes"])
    rng = np.random.RandomState(case["seed"])
    off = level_offsets(sizes)
    A = off[-1]
    cls = np.empty((N, A, C), F32)
    for n in range(N):
        for l, (h, w) in enumerate(sizes):
            cls[n, off[l]:off[l + 1]] = build_level(rng, h * w, C, case["recipes"][n][l], case["filler"])
    bins = rng.randint(0, 17, (N, A, 4))
    if case.get("no_clamp"):                                       # left / top distances never reach past the image origin
        ctr = anchor_centres(sizes)
        for l in range(len(sizes)):
            lim = (ctr[off[l]:off[l + 1]] / STRIDES[l]).astype(np.int64)
            bins[:, off[l]:off[l + 1], 0] = np.minimum(bins[:, off[l]:off[l + 1], 0], lim[None, :, 0])
            bins[:, off[l]:off[l + 1], 1] = np.minimum(bins[:, off[l]:off[l + 1], 1], lim[None, :, 1])
    bbox = np.stack([build_box_logits(bins[n]) for n in range(N)])
    return dict(cls=cls, bbox=bbox, bins=bins, img_hw=np.asarray(case["img_hw"], F32).reshape(N, 2))


# ---------------------------------------------------------------------------------------------
# top-k reference: filter_scores_and_topk + decode, per (image, level)
# ---------------------------------------------------------------------------------------------
LevelRef = namedtuple("LevelRef", "idx labels boxes scores logits path total need c_eq decided_pass tie_chunks clamped")


def topk_ref(cls, bbox, sizes, img_hw, score_thr, k):
    """-> [N][L] LevelRef: the selected flat (anchor * C + class) indices in output order, labels, fp64 boxes and scores, and the
    path the selection must take -- `all` (no more candidates than k), `fit` (the k-th key's equal keys all fit) or `tie` (they do
    not: `need` of the `c_eq` are wanted, lowest indices first) -- with the radix pass that isolates the k-th key (how many leading
    digits it shares with another candidate key) and, for `tie`, the 1024-element chunks of the first and the last wanted tie and
    the level's last chunk."""
    N, A, C = cls.shape
    off = level_offsets(sizes)
    ctr = anchor_centres(sizes)
    z = bbox.reshape(N, A, 4, 17)
    assert ((z == 0) | (z == -200)).all() and ((z == 0).sum(-1) == 1).all(), "box logits must be one-hot"
    dist_bins = z.argmax(-1).astype(np.float64)
    thr = F32(score_thr)
    out = []
    for n in range(N):
        H, W = float(img_hw[n][0]), float(img_hw[n][1])
        row = []
        for l in range(len(sizes)):
            x = cls[n, off[l]:off[l + 1]].reshape(-1)
            s64 = score64(x)
            with np.errstate(invalid="ignore"):
                cand = np.flatnonzero(s64.astype(F32) > thr)
            order = np.argsort(-s64[cand], kind="stable")
            sel = cand[order[:k]]
            total = len(cand)
            need = c_eq = 0
            dpass, tie_chunks = -1, None
            if total <= k:
                path = "all"
            else:
                T = s64[sel[-1]]
                c_gt, c_eq = int((s64[cand] > T).sum()), int((s64[cand] == T).sum())
                need = k - c_gt
                path = "fit" if need == c_eq else "tie"
                keys = np.unique(key_of(s64[cand].astype(F32)))
                kT = int(key_of(F32(T)))
                others = keys[keys != kT]
                dpass = 2 if ((others >> 10) == (kT >> 10)).any() else (1 if ((others >> 21) == (kT >> 21)).any() else 0)
                if path == "tie":
                    pos = cand[s64[cand] == T]
                    tie_chunks = (int(pos[0]) // 1024, int(pos[need - 1]) // 1024, (len(x) - 1) // 1024)
            a = off[l] + sel // C
            d = dist_bins[n, a] * STRIDES[l]
            raw = np.stack([ctr[a, 0] - d[:, 0], ctr[a, 1] - d[:, 1], ctr[a, 0] + d[:, 2], ctr[a, 1] + d[:, 3]], 1)
            boxes = raw.copy()
            boxes[:, 0::2] = np.clip(raw[:, 0::2], 0, W)
            boxes[:, 1::2] = np.clip(raw[:, 1::2], 0, H)
            row.append(LevelRef(sel, (sel % C).astype(np.int64), boxes, s64[sel], x[sel], path, total, need, c_eq, dpass,
                                tie_chunks, int((boxes != raw).sum())))
        out.append(row)
    return out


def concat_levels(row, score_fn=score32):
    """one image's LevelRefs -> erd_predict_topk's level-major rows: boxes [M, 4] fp32, scores [M] fp32, labels [M] int32"""
    boxes = np.concatenate([r.boxes for r in row]).astype(F32).reshape(-1, 4)
    assert (boxes.astype(np.float64) == np.concatenate([r.boxes for r in row]).reshape(-1, 4)).all()      # exact in fp32
    scores = np.concatenate([np.asarray(score_fn(r.logits), F32).reshape(-1) for r in row])
    return boxes, scores, np.concatenate([r.labels for r in row]).astype(np.int32)


# ---------------------------------------------------------------------------------------------
# NMS reference: fp32 on both sides
# ---------------------------------------------------------------------------------------------
def nms_ref(boxes, scores, labels, num, inv_scale, min_bbox_size, iou_thr, max_per_img):
    """boxes [N, cols, 4] fp32, scores [N, cols] fp32, labels [N, cols] int32, num [N], inv_scale [N, 2] fp32 (numpy) ->
    dets [N, max_per_img, 5] fp32, det_labels [N, max_per_img] int64, det_num [N] int32 (torch, rows past the count zero), and per
    image (rows that pass the size filter, rows the NMS keeps before the max_per_img cut)."""
    N = boxes.shape[0]
    dets = torch.zeros((N, max_per_img, 5), dtype=torch.float32)
    det_labels = torch.zeros((N, max_per_img), dtype=torch.int64)
    det_num = torch.zeros((N,), dtype=torch.int32)
    thr = float(F32(iou_thr))                                      # the kernel's argument is a float
    info = []
    for n in range(N):
        M = int(num[n])
        b = torch.from_numpy(np.ascontiguousarray(boxes[n, :M], F32))
        s = torch.from_numpy(np.ascontiguousarray(scores[n, :M], F32))
        lab = torch.from_numpy(np.ascontiguousarray(labels[n, :M]).astype(np.int64))
        sc = torch.from_numpy(np.asarray(inv_scale[n], F32))
        b = b * sc.repeat(2)[None]
        if min_bbox_size >= 0:
            ok = ((b[:, 2] - b[:, 0]) > float(F32(min_bbox_size))) & ((b[:, 3] - b[:, 1]) > float(F32(min_bbox_size)))
            b, s, lab = b[ok], s[ok], lab[ok]
        keep = O.nms_class_offset(b, s, lab, thr)
        info.append((int(b.shape[0]), int(keep.shape[0])))
        keep = keep[:max_per_img]
        c = int(keep.shape[0])
        dets[n, :c, :4], dets[n, :c, 4], det_labels[n, :c], det_num[n] = b[keep], s[keep], lab[keep], c
    return dets, det_labels, det_num, info


# ---------------------------------------------------------------------------------------------
# top-k and composition cases
# ---------------------------------------------------------------------------------------------
ABOVE_MID = [float(x) for x in TABLE if score32(x) > F32(THR_MID)]


def _distinct(total, seed):
    """`total` different entries above THR_MID, one score each"""
    rng = np.random.RandomState(seed)
    return {float(x): 1 for x in rng.choice(ABOVE_MID, total, replace=False)}


def _split(total, nel, seed, pool=None, classes=None):
    """`total` (capped at nel) scores over a few seeded tie classes"""
    rng = np.random.RandomState(seed)
    total = min(total, nel)
    if total == 0:
        return {}
    m = min(total, classes or int(rng.randint(1, 6)))
    cuts = np.sort(rng.choice(np.arange(1, total), m - 1, replace=False)) if m > 1 else np.array([], np.int64)
    sizes = np.diff(np.concatenate([[0], cuts, [total]]))
    return {float(x): int(c) for x, c in zip(rng.choice(pool or ABOVE_MID, m, replace=False), sizes)}


def _nel(sizes, C):
    return [h * w * C for h, w in sizes]


def _case(name, recipes, k, C=80, sizes=LV5, thr=THR_MID, filler=None, seed=0, img_hw=((70, 100),) * 3, **nms):
    cfg = dict(min_bbox_size=0, iou_thr=0.6, max_per_img=100, scale_factor=((1.0, 1.0),) * 3)
    cfg.update(nms)
    return dict(name=name, recipes=recipes, nms_pre=k, C=C, sizes=sizes, score_thr=thr,
                filler=filler if filler is not None else (NEVER if thr == 0.0 else BELOW_MID), seed=seed, img_hw=img_hw, **cfg)


def _sweep(name, k, C=80, sizes=LV5, thr=THR_MID, seed=0, **kw):
    """every (image, level) pair takes the next of: 0, 1, k-1, k, k+1, about 2k, every score of the level"""
    nel = _nel(sizes, C)
    recipes = []
    for n in range(3):
        row = []
        for l in range(5):
            totals = [0, 1, k - 1, k, k + 1, 2 * k + 3, nel[l]]
            t = max(totals[(n * 5 + l + seed) % 7], 0)
            row.append(_split(t, nel[l], 1000 * seed + 10 * n + l, pool=None if thr != THR_P2 else P2_GROUP[1:] + [0.125, 0.25, 2.0]))
        recipes.append(row)
    return _case(name, recipes, k, C=C, sizes=sizes, thr=thr, seed=seed, **kw)


def _cases():
    n80 = _nel(LV5, 80)                                            # 9360, 2800, 960, 320, 80
    cs = []
    # totals 0, 1, k-1, k, k+1 on every level, distinct scores (k = 7) and tie classes (k = 100; level 4 holds only 80 scores)
    tot = [[0, 1, 6, 7, 8], [8, 7, 6, 1, 0], [7, 8, 0, 6, 1]]
    cs.append(_case("totals_k7", [[_distinct(t, 31 * n + l) for l, t in enumerate(r)] for n, r in enumerate(tot)], 7, seed=1))
    tot = [[0, 1, 99, 100, 80], [101, 100, 99, 1, 0], [100, 101, 0, 99, 1]]
    cs.append(_case("totals_k100", [[_split(t, n80[l], 77 * n + l, classes=3) for l, t in enumerate(r)]
                                    for n, r in enumerate(tot)], 100, seed=2))
    # the cut on a class boundary (c_eq == need), and inside a class with need of 1, c_eq - 1 and mid-way; level 4 takes `all`
    cs.append(_case("cuts", [
        [{2.0: 40, 1.0: 60, 0.5: 50}, {2.0: 99, 1.0: 30}, {2.0: 71, 1.0: 30, 0.5: 9}, {2.0: 50, 1.0: 100}, {2.0: 80}],
        [{2.0: 99, 1.0: 2}, {2.0: 100, 1.0: 1}, {3.0: 1, 2.0: 99, 1.0: 7}, {2.0: 101}, {2.0: 3}],
        [{1.0: 100, 0.5: 1}, {2.0: 50, 1.0: 51}, {}, {2.0: 1, 1.0: 319}, {INF: 1, 2.0: 5}]], 100, seed=3))
    # one class fills the whole level (score_thr = 0: nothing is filler)
    cs.append(_case("giant", [
        [{1.0: e} for e in n80],
        [{1.0: e - 3, 2.0: 3} for e in n80],
        [{INF: 1}, {}, {INF: 2, 1.0: 958}, {0.0: 320}, {-6.0: 80}]], 100, thr=0.0, seed=4))
    # where the last wanted tie lies: all wanted in the first 1024 elements (early break), in the last partial chunk, across a chunk edge
    cs.append(_case("tie_positions", [
        [{3.0: 60, 1.0: [(40, (0, 1024)), (200, (2048, 9360))]}, {3.0: 10, 1.0: [(48, (2000, 2048)), (52, (2048, 2100))]},
         {1.0: (200, (0, 512))}, {1.0: 300}, {1.0: 50}],
        [{3.0: 60, 1.0: (70, (9216, 9360))}, {3.0: 99, 1.0: [(1, (0, 1)), (1, (2799, 2800))]},      # need 1 of 2: the first wins
         {2.0: 99, 1.0: [(1, (0, 1)), (1, (959, 960))]}, {1.0: 320}, {1.0: 80}],
        [{3.0: 60, 1.0: [(20, (1004, 1024)), (30, (1024, 1054))]}, {1.0: [(60, (964, 1024)), (60, (2048, 2108))]},
         {1.0: (120, (840, 960))}, {3.0: 99, 1.0: 200}, {}]], 100, seed=5))
    # the k-th key isolated in radix pass 0, 1 and 2 (score_thr = 0 so that the -3 + j/4096 group is above it)
    p0, p1, p2 = ({x: 3 for x in g} for g in (P0_GROUP, P1_GROUP, P2_GROUP))
    cs.append(_case("radix_passes", [[p2, p1, p0, {**p2, **p0}, {**p1, 2.0: 4}],
                                     [p1, p0, p2, {**p1, **p2}, p2],
                                     [p0, p2, p1, {x: 40 for x in P2_GROUP}, {x: 5 for x in P1_GROUP}]], 10, thr=0.0, seed=6))
    # a threshold between two entries that share 22 key bits
    cs.append(_sweep("thr_between_pass2_entries", 7, thr=THR_P2, seed=7, filler=[0.0, -1.0, -6.0, -INF]))
    # nms_pre values; image sizes that clamp and scale factors with sx != sy
    for i, k in enumerate((1, 2, 7, 100, 1000, 1024, 4096)):
        cs.append(_sweep(f"nms_pre_{k}", k, seed=10 + i, thr=0.0 if k in (2, 1024) else THR_MID,
                         scale_factor=((1.0, 1.0), (1.333, 1.2), (0.5, 0.8)), img_hw=((70, 100), (64, 90), (33, 47)),
                         min_bbox_size=(-1 if k == 100 else 0)))
    # class counts; a 65-anchor level
    for i, (C, sizes) in enumerate(((70, LV5), (3, LV5), (1, LV5), (3, LV65), (80, LV65))):
        cs.append(_sweep(f"C{C}_{'lv65' if sizes is LV65 else 'lv5'}", 7 if C < 70 else 100, C=C, sizes=sizes, seed=20 + i,
                         scale_factor=((2.0, 2.0), (1.0, 1.0), (0.75, 1.5))))
    # composition: the real configuration's shape of parameters; one case in which no clamp triggers
    cs.append(_sweep("compose_c80", 1000, seed=30, scale_factor=((1.333, 1.333), (1.0, 1.0), (0.6, 0.7)), iou_thr=0.6,
                     img_hw=((70, 100), (72, 104), (50, 60)), max_per_img=100))
    cs.append(_sweep("compose_c70_noclamp", 100, C=70, seed=31, scale_factor=((1.25, 1.5), (1.0, 1.0), (0.6, 0.7)), iou_thr=0.5,
                     img_hw=((4096, 4096),) * 3, max_per_img=20, no_clamp=True))
    return cs


CASES = {c["name"]: c for c in _cases()}
MIXED_CASE = "cuts"                                                # one launch whose 15 pairs take all three paths


@functools.lru_cache(maxsize=None)
def case_data(name):
    """(inputs, [N][L] LevelRef) of a case, computed once and shared; callers must not modify it"""
    case = CASES[name]
    inp = build_inputs(case)
    ref = topk_ref(inp["cls"], inp["bbox"], case["sizes"], inp["img_hw"], case["score_thr"], case["nms_pre"])
    return inp, ref


def inv_scale_of(case):
    return np.array([[1 / f[0], 1 / f[1]] for f in case["scale_factor"]], F32)


def topk_rows(case, ref, score_fn=score32):
    """the padded [N, L * nms_pre] tensors erd_predict_topk would write, from the reference (zeros past the counts)"""
    N, cols = len(ref), len(case["sizes"]) * case["nms_pre"]
    boxes, scores = np.zeros((N, cols, 4), F32), np.zeros((N, cols), F32)
    labels, num = np.zeros((N, cols), np.int32), np.zeros((N,), np.int32)
    for n, row in enumerate(ref):
        b, s, lab = concat_levels(row, score_fn)
        num[n] = len(s)
        boxes[n, :num[n]], scores[n, :num[n]], labels[n, :num[n]] = b, s, lab
    return boxes, scores, labels, num


def case_nms_ref(case, boxes, scores, labels, num):
    return nms_ref(boxes, scores, labels, num, inv_scale_of(case), case["min_bbox_size"], case["iou_thr"], case["max_per_img"])


def oracle_single(case, inp, n):
    """O.predict_single on image n of a case"""
    off = level_offsets(case["sizes"])
    cm = [torch.from_numpy(inp["cls"][n, off[l]:off[l + 1]].reshape(h, w, -1)).permute(2, 0, 1)
          for l, (h, w) in enumerate(case["sizes"])]
    bm = [torch.from_numpy(inp["bbox"][n, off[l]:off[l + 1]].reshape(h, w, 68)).permute(2, 0, 1)
          for l, (h, w) in enumerate(case["sizes"])]
    hw = inp["img_hw"][n]
    return O.predict_single(cm, bm, (float(hw[0]), float(hw[1])), tuple(case["scale_factor"][n]), score_thr=case["score_thr"],
                            nms_pre=case["nms_pre"], min_bbox_size=case["min_bbox_size"], iou_thr=float(F32(case["iou_thr"])),
                            max_per_img=case["max_per_img"], strides=STRIDES[:len(case["sizes"])])


def census(names=None):
    """what the cases reach, from the reference's path report alone: a set of tags"""
    tags = set()
    for name in (names or CASES):
        case = CASES[name]
        _, ref = case_data(name)
        k = case["nms_pre"]
        paths = set()
        for row in ref:
            for l, r in enumerate(row):
                paths.add(r.path)
                tags.add("path:" + r.path)
                for d, t in ((0, "0"), (1, "1"), (k - 1, "k-1"), (k, "k"), (k + 1, "k+1")):
                    if r.total == d:
                        tags.add("total:" + t)
                if r.path != "all":
                    tags.add(f"pass:{r.decided_pass}")
                if r.path == "fit" and r.c_eq > 1:
                    tags.add("fit:class_boundary")
                if r.path == "tie":
                    tags.add("need:1" if r.need == 1 else ("need:c_eq-1" if r.need == r.c_eq - 1 else "need:mid"))
                    nel = case["sizes"][l][0] * case["sizes"][l][1] * case["C"]
                    if r.c_eq == nel:
                        tags.add("tie:giant")
                    first, last, end = r.tie_chunks
                    if last == 0 and end > 0:
                        tags.add("tie:early_break")
                    if first == end and end > 0 and nel % 1024:
                        tags.add("tie:last_partial_chunk")
                    if first != last:
                        tags.add("tie:straddle")
                    if last > 1:
                        tags.add("tie:running_count")
                if r.clamped:
                    tags.add("clamp:some")
                cnt = case["sizes"][l][0] * case["sizes"][l][1]
                if cnt == 1:
                    tags.add("level:1")
                elif cnt < 64:
                    tags.add("level:<64")
                elif cnt == 65:
                    tags.add("level:65")
                if any(np.isposinf(r.logits)):
                    tags.add("score:1.0")
        if paths == {"all", "fit", "tie"}:
            tags.add("mixed_launch")
        if not any(r.clamped for row in ref for r in row):
            tags.add("clamp:none")
        tags.add(f"C:{case['C']}")
        tags.add(f"nms_pre:{k}")
        tags.add(f"thr:{case['score_thr']:.6g}")
    return tags


CENSUS_WANTED = {
    "path:all", "path:fit", "path:tie", "total:0", "total:1", "total:k-1", "total:k", "total:k+1", "pass:0", "pass:1", "pass:2",
    "fit:class_boundary", "need:1", "need:c_eq-1", "need:mid", "tie:giant", "tie:early_break", "tie:last_partial_chunk",
    "tie:straddle", "tie:running_count", "clamp:some", "clamp:none", "level:1", "level:<64", "level:65", "score:1.0", "mixed_launch",
    "C:80", "C:70", "C:3", "C:1", "nms_pre:1", "nms_pre:2", "nms_pre:7", "nms_pre:100", "nms_pre:1000", "nms_pre:1024",
    "nms_pre:4096", "thr:0", "thr:0.05", f"thr:{THR_P2:.6g}"}


# ---------------------------------------------------------------------------------------------
# NMS cases: inputs of erd_predict_nms built on the host
# ---------------------------------------------------------------------------------------------
def _pad(rows, cols):
    """[(boxes [M, 4], scores [M], labels [M])] per image -> padded arrays + num; rows past M carry junk the kernel must ignore"""
    N = len(rows)
    boxes, scores = np.full((N, cols, 4), 1e9, F32), np.full((N, cols), 9.0, F32)
    labels, num = np.full((N, cols), 5, np.int32), np.zeros((N,), np.int32)
    for n, (b, s, lab) in enumerate(rows):
        M = len(s)
        assert M <= cols
        boxes[n, :M], scores[n, :M], labels[n, :M], num[n] = b, s, lab, M
    return boxes, scores, labels, num


def _empty():
    return np.zeros((0, 4), F32), np.zeros((0,), F32), np.zeros((0,), np.int32)


def _random_rows(rng, M, canvas=(1333, 800), n_labels=80, tie_levels=64):
    """integer boxes, many overlapping; scores k / tie_levels: ties everywhere"""
    cx, cy = rng.randint(0, canvas[0], M), rng.randint(0, canvas[1], M)
    w, h = rng.randint(0, 200, M), rng.randint(0, 200, M)
    b = np.stack([np.maximum(cx - w // 2, 0), np.maximum(cy - h // 2, 0), np.minimum(cx + w - w // 2, canvas[0]),
                  np.minimum(cy + h - h // 2, canvas[1])], 1).astype(F32)
    return b, (rng.randint(1, tie_levels + 1, M) / tie_levels).astype(F32), rng.randint(0, n_labels, M).astype(np.int32)


def _grid_rows(rng, survivors, min_size):
    """disjoint integer boxes, one per 40 x 40 cell, so that the NMS keeps every row the size filter keeps and the output shows the
    compaction's order.  Rows 64m - 1 and 64m (both sides of every wave edge, hence of every 1024 block edge) have w or h ==
    min_size exactly and are dropped; rows 64m - 2 and 64m + 1 are one unit above it and stay.  M is chosen so that exactly
    `survivors` rows pass."""
    M = passed = 0
    while passed < survivors:
        passed += M % 64 not in (0, 63)
        M += 1
    i = np.arange(M)
    w, h = rng.randint(min_size + 2, 36, M), rng.randint(min_size + 2, 36, M)
    w[i % 64 == 63] = min_size
    h[i % 64 == 0] = min_size
    w[i % 64 == 62] = min_size + 1
    h[i % 64 == 1] = min_size + 1
    x0, y0 = (i % 50) * 40, (i // 50) * 40
    b = np.stack([x0, y0, x0 + w, y0 + h], 1).astype(F32)
    return b, (rng.randint(1, 17, M) / 16).astype(F32), rng.randint(0, 80, M).astype(np.int32)


def _near_threshold_rows(rng, pairs, iou_thr):
    """pairs of same-label boxes near coordinate 2700 whose IoU is within about 2e-3 of the threshold, labels up to 79: whether
    the second is suppressed depends on how the fp32 class offset (up to 79 * 2701) rounds the corners"""
    x = rng.uniform(100, 2600, pairs)
    y = rng.uniform(100, 2600, pairs)
    w = rng.uniform(30, 60, pairs)
    h = rng.uniform(30, 60, pairs)
    dx = w * (1 - iou_thr) / (1 + iou_thr) * (1 + rng.uniform(-4e-3, 4e-3, pairs))      # IoU = (w - dx) / (w + dx)
    a = np.stack([x, y, x + w, y + h], 1)
    b = a + np.stack([dx, 0 * dx, dx, 0 * dx], 1)
    lab = rng.randint(0, 80, pairs)
    lab[:4] = 79
    boxes = np.concatenate([a, b]).astype(F32)
    boxes[0] = [2650, 2660, 2700, 2700]                             # the largest coordinate: the offset is 2701 per label
    order = rng.permutation(2 * pairs)
    return boxes[order], rng.uniform(0.1, 1, 2 * pairs).astype(F32)[order], np.concatenate([lab, lab]).astype(np.int32)[order]


def _nms_case(name, rows, cols=None, inv_scale=None, min_bbox_size=0.0, iou_thr=0.6, max_per_img=100):
    cols = cols or max(1, max(len(r[1]) for r in rows))
    boxes, scores, labels, num = _pad(rows, cols)
    inv = np.asarray(inv_scale if inv_scale is not None else [[1.0, 1.0]] * len(rows), F32)
    return dict(name=name, boxes=boxes, scores=scores, labels=labels, num=num, inv_scale=inv, min_bbox_size=min_bbox_size,
                iou_thr=float(F32(iou_thr)), max_per_img=max_per_img)


HALF_DOWN = float(np.nextafter(F32(0.5), F32(0)))


def _iou_half_rows():
    """integer boxes with IoU exactly 0.5 (inter 50, union 100), per label; a second pair one label further"""
    b = np.array([[0, 0, 10, 10], [0, 0, 10, 5], [20, 20, 30, 30], [20, 25, 30, 30], [0, 0, 10, 10], [0, 0, 5, 10]], F32)
    return b, np.array([0.9, 0.8, 0.7, 0.7, 0.6, 0.5], F32), np.array([0, 0, 3, 3, 7, 7], np.int32)


def _tie_rows():
    """equal scores at positions of different levels: the earlier position wins and suppresses the later"""
    b = np.array([[10, 10, 50, 50], [100, 100, 140, 140], [11, 10, 51, 50], [101, 100, 141, 140], [12, 10, 52, 50]], F32)
    return b, np.array([0.5, 0.75, 0.5, 0.75, 0.5], F32), np.array([2, 2, 2, 2, 2], np.int32)


def _label_rows():
    """identical boxes: different labels are kept, the same label is suppressed"""
    b = np.tile(np.array([[5, 6, 45, 66]], F32), (6, 1))
    return b, np.array([0.9, 0.8, 0.7, 0.6, 0.5, 0.4], F32), np.array([0, 79, 0, 40, 79, 1], np.int32)


def _degenerate_rows():
    """zero-width, zero-height and zero-area boxes, some identical (IoU 0 / 0), among ordinary ones"""
    b = np.array([[5, 5, 5, 20], [5, 5, 5, 20], [7, 7, 30, 7], [9, 9, 9, 9], [9, 9, 9, 9], [0, 0, 10, 10], [0, 0, 10, 9],
                  [5, 5, 5, 20]], F32)
    return b, np.array([0.9, 0.9, 0.8, 0.7, 0.7, 0.6, 0.5, 0.4], F32), np.array([1, 1, 1, 2, 2, 1, 1, 1], np.int32)


NMS_CASE_NAMES = (
    "batch_5000_0_1", "batch_5000_keep_all", "survivors_1_1023_1024", "survivors_1025_2049_0", "min_size_0_degenerate",
    "min_size_minus1_degenerate", "iou_exactly_thr_kept", "iou_just_above_thr_suppressed", "labels_identical_boxes",
    "labels_79_near_2700_thr0.6", "labels_79_near_2700_thr0.5", "score_ties", "max_per_img_equal", "max_per_img_one_below",
    "max_per_img_one", "max_per_img_smallest_image")


@functools.lru_cache(maxsize=None)
def nms_cases():
    """name -> case, built on first use (NMS_CASE_NAMES lists the names for parametrising without building)"""
    rng = np.random.RandomState(4242)
    cs = [_nms_case("batch_5000_0_1", [_random_rows(rng, 5000, canvas=(500, 400)), _empty(), _random_rows(rng, 1)], cols=5000,
                    inv_scale=[[1 / 1.333, 1 / 1.2], [1.0, 1.0], [2.0, 0.5]]),
          _nms_case("batch_5000_keep_all", [_random_rows(rng, 5000), _random_rows(rng, 300), _empty()], cols=5000,
                    inv_scale=[[0.75, 1.5], [1 / 3, 1 / 7], [1.0, 1.0]], max_per_img=5000, iou_thr=0.45)]
    for name, counts in (("survivors_1_1023_1024", (1, 1023, 1024)), ("survivors_1025_2049_0", (1025, 2049, 0))):
        cs.append(_nms_case(name, [_grid_rows(rng, c, 4) if c else _empty() for c in counts], min_bbox_size=4.0,
                            max_per_img=3000, inv_scale=[[1.0, 1.0], [0.5, 0.5], [1.0, 1.0]]))
        cs[-1]["boxes"][1] *= 2                                    # image 1: everything doubled, then halved by inv_scale
    cs.append(_nms_case("min_size_0_degenerate", [_degenerate_rows()] * 3, min_bbox_size=0.0))
    cs.append(_nms_case("min_size_minus1_degenerate", [_degenerate_rows()] * 3, min_bbox_size=-1.0))
    cs.append(_nms_case("iou_exactly_thr_kept", [_iou_half_rows()] * 3, iou_thr=0.5))
    cs.append(_nms_case("iou_just_above_thr_suppressed", [_iou_half_rows()] * 3, iou_thr=HALF_DOWN))
    cs.append(_nms_case("labels_identical_boxes", [_label_rows(), _tie_rows(), _empty()]))
    for thr in (0.6, 0.5):
        cs.append(_nms_case(f"labels_79_near_2700_thr{thr}", [_near_threshold_rows(rng, 400, thr) for _ in range(3)], iou_thr=thr,
                            max_per_img=1000, inv_scale=[[1.0, 1.0], [1 / 1.333, 1 / 1.333], [0.9, 1.1]]))
    cs.append(_nms_case("score_ties", [_tie_rows(), _random_rows(rng, 700, tie_levels=3, n_labels=2),
                                       _random_rows(rng, 64, canvas=(90, 70), tie_levels=1, n_labels=1)], max_per_img=700))
    base = [_random_rows(rng, 300, canvas=(400, 300), n_labels=3, tie_levels=8) for _ in range(3)]
    probe = _nms_case("probe", base, max_per_img=300)
    kept = nms_ref(probe["boxes"], probe["scores"], probe["labels"], probe["num"], probe["inv_scale"], 0.0, 0.6, 300)[3]
    kmin = min(k for _, k in kept)
    assert kmin > 2
    for nm, mpi in (("equal", kept[0][1]), ("one_below", kept[0][1] - 1), ("one", 1), ("smallest_image", kmin)):
        cs.append(_nms_case(f"max_per_img_{nm}", base, max_per_img=mpi))
    return {c["name"]: c for c in cs}


@functools.lru_cache(maxsize=None)
def nms_case_ref(name):
    c = nms_cases()[name]
    return nms_ref(c["boxes"], c["scores"], c["labels"], c["num"], c["inv_scale"], c["min_bbox_size"], c["iou_thr"],
                   c["max_per_img"])
