"""GPU: erd_predict_topk and erd_predict_nms pinned exactly at the C ABI, against the host references of tests/predict_refs.py.

tests/test_gpu_predict.py reaches these kernels through GFLHead.predict_by_feat on Gaussian logits and has to tolerate the GPU's
expf.  Here the classification logits come from a table whose sigmoids are >= 128 fp32 ulps apart and the box logits are one-hot,
so the selection (`num`, order, labels), the decoded boxes and everything the NMS writes must match bit for bit; a score must lie
within 63 ulps of its table entry (half the table's separation: it maps back to one entry) and all scores of one entry must be
bit-equal.  Every output of the raw top-k call is pre-filled with a sentinel and the workspaces with 0xFF bytes (`same_ws` asserts that
the launch ran in the buffer that was filled).  Which path each
(image, level) pair takes is reported by the reference from counts alone; tests/test_predict_refs_cpu.py holds the census.

Largest sigmoid error seen on the MI355X over all cases: 1 ulp ("What pins predict.hip")."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import predict_refs as R
from oracle import erd_oracle as O

SENT_F = 0x7FC0BEEF            # a NaN with a payload
SENT_L, SENT_N = -12345, -7


@pytest.fixture(scope="module")
def K():
    from erd_amd import kernels
    assert torch.cuda.is_available()
    return kernels


def device():
    """the device as the tensors name it ("cuda:0"): kernels.workspace keys its cache on that string"""
    return torch.device("cuda", torch.cuda.current_device())


def dirty(K, name, nbytes):
    """fill the cached workspace `name` with 0xFF bytes; callers check with `same_ws` that the launch ran in this buffer"""
    ws = K.workspace(name, nbytes, device())
    ws.fill_(0xFF)
    return ws


def same_ws(K, name, nbytes, ws, like):
    """the workspace a wrapper fetches for a tensor on `like`'s device is the buffer `ws` that was dirtied"""
    assert like.device == device() and K.workspace(name, nbytes, like.device).data_ptr() == ws.data_ptr(), (name, like.device)


def anchors_of(sizes):
    return torch.cat(O.grid_anchors(list(sizes), R.STRIDES[:len(sizes)])).cuda()


def raw_topk(K, case, inp, fill_ws=True):
    """erd_predict_topk into sentinel-filled outputs -> (boxes, scores, labels, num) on the host, floats as int32 bit patterns"""
    k, thr = case["nms_pre"], case["score_thr"]
    sizes = case["sizes"]
    N, A, Cc = inp["cls"].shape
    cols = len(sizes) * k
    cls, bbox, hw, anchors = (torch.from_numpy(inp["cls"]).cuda(), torch.from_numpy(inp["bbox"]).cuda(),
                              torch.from_numpy(inp["img_hw"]).cuda(), anchors_of(sizes))
    boxes = torch.full((N, cols, 4), SENT_F, dtype=torch.int32, device="cuda")
    scores = torch.full((N, cols), SENT_F, dtype=torch.int32, device="cuda")
    labels = torch.full((N, cols), SENT_L, dtype=torch.int32, device="cuda")
    num = torch.full((N,), SENT_N, dtype=torch.int32, device="cuda")
    need = int(K._lib.load().erd_predict_ws_bytes(N, len(sizes), k))
    ws = dirty(K, "predict", need) if fill_ws else K.workspace("predict", need, cls.device)
    same_ws(K, "predict", need, ws, cls)
    lv = K.make_levels(sizes)
    K.call("erd_predict_topk", K._p(cls), K._p(bbox), K._p(anchors), N, A, Cc, C.byref(lv),
           K._iarr(R.STRIDES[:len(sizes)]), K._p(hw), float(thr), int(k), K._p(boxes), K._p(scores), K._p(labels), K._p(num),
           K._p(ws), C.c_size_t(need), K._stream())
    torch.cuda.synchronize()
    return boxes.cpu().numpy(), scores.cpu().numpy(), labels.cpu().numpy(), num.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def check_topk(case, ref, got, by_entry=None):
    """every assertion of the module docstring, per (image, level); returns the largest ulp error of a score"""
    boxes, scores, labels, num = got
    by_entry = {} if by_entry is None else by_entry
    worst = 0
    for n, row in enumerate(ref):
        assert int(num[n]) == sum(len(r.idx) for r in row), (case["name"], n, int(num[n]), [len(r.idx) for r in row])
        at = 0
        for l, r in enumerate(row):
            c = len(r.idx)
            what = (case["name"], n, l, r.path, r.total, r.need, r.c_eq)
            assert np.array_equal(labels[n, at:at + c], r.labels), what                        # exact and in order
            assert np.array_equal(boxes[n, at:at + c], bits(r.boxes.astype(np.float32))), what  # bit-equal, clamps included
            s = scores[n, at:at + c].view(np.float32)
            want = R.score32(r.logits)
            if c:
                err = R.ulps(s, want)
                worst = max(worst, int(err.max()))
                assert int(err.max()) <= R.SCORE_ULPS, what + (int(err.max()),)
                assert float(np.abs(s.astype(np.float64) - r.scores).max()) <= 1e-6, what
            for lg, b in zip(r.logits.tolist(), scores[n, at:at + c].tolist()):
                assert by_entry.setdefault(lg, b) == b, what + (lg,)                           # one entry, one bit pattern
            at += c
        assert (boxes[n, at:] == np.int32(SENT_F)).all() and (scores[n, at:] == np.int32(SENT_F)).all(), (case["name"], n)
        assert (labels[n, at:] == SENT_L).all(), (case["name"], n)
    return worst


# ---------------------------------------------------------------------------------------------
# top-k
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_topk_exact(K, name):
    case = R.CASES[name]
    inp, ref = R.case_data(name)
    worst = check_topk(case, ref, raw_topk(K, case, inp))
    print(f"[predict_exact] {name}: paths {sorted({r.path for row in ref for r in row})}, max sigmoid error {worst} ulp")


def test_topk_mixed_launch_takes_all_three_paths(K):
    """one launch whose 15 (image, level) pairs are spread over `all`, `fit` and `tie`"""
    case = R.CASES[R.MIXED_CASE]
    inp, ref = R.case_data(R.MIXED_CASE)
    paths = [r.path for row in ref for r in row]
    assert len(paths) == 15 and set(paths) == {"all", "fit", "tie"}
    check_topk(case, ref, raw_topk(K, case, inp))


def test_topk_workspace_reuse(K):
    """two calls in a row are bit-identical; a small launch after a large one, in the workspace the large one left, is correct"""
    big, small = R.CASES["nms_pre_4096"], R.CASES["totals_k7"]
    (ib, rb), (ism, rs) = R.case_data("nms_pre_4096"), R.case_data("totals_k7")
    a = raw_topk(K, big, ib)
    b = raw_topk(K, big, ib, fill_ws=False)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    check_topk(big, rb, b)
    check_topk(small, rs, raw_topk(K, small, ism, fill_ws=False))
    check_topk(big, rb, raw_topk(K, big, ib, fill_ws=False))


def test_topk_refusals_leave_the_outputs_untouched(K):
    """nms_pre of 0, 4097 and -3, score_thr < 0 and a workspace one byte short: the argument checks return before anything is
    launched, so each call raises and every output element still holds its sentinel"""
    case = R.CASES["totals_k7"]
    inp, _ = R.case_data("totals_k7")
    N, A, Cc = inp["cls"].shape
    cls, bbox, hw, anchors = (torch.from_numpy(inp["cls"]).cuda(), torch.from_numpy(inp["bbox"]).cuda(),
                              torch.from_numpy(inp["img_hw"]).cuda(), anchors_of(case["sizes"]))
    cols = 5 * 7
    boxes = torch.full((N, cols, 4), SENT_F, dtype=torch.int32, device="cuda")
    scores = torch.full((N, cols), SENT_F, dtype=torch.int32, device="cuda")
    labels = torch.full((N, cols), SENT_L, dtype=torch.int32, device="cuda")
    num = torch.full((N,), SENT_N, dtype=torch.int32, device="cuda")
    ws = torch.empty(1 << 22, dtype=torch.uint8, device="cuda")
    need = int(K._lib.load().erd_predict_ws_bytes(N, 5, 7))
    lv = K.make_levels(case["sizes"])
    for k, thr, nbytes in ((0, 0.05, need), (4097, 0.05, 1 << 22), (7, -1e-3, need), (7, 0.05, need - 1), (-3, 0.05, need)):
        with pytest.raises(K._lib.ErdHipError):
            K.call("erd_predict_topk", K._p(cls), K._p(bbox), K._p(anchors), N, A, Cc, C.byref(lv), K._iarr(R.STRIDES),
                   K._p(hw), float(thr), int(k), K._p(boxes), K._p(scores), K._p(labels), K._p(num), K._p(ws),
                   C.c_size_t(nbytes), K._stream())
    torch.cuda.synchronize()
    assert (boxes == SENT_F).all() and (scores == SENT_F).all() and (labels == SENT_L).all() and (num == SENT_N).all()


# ---------------------------------------------------------------------------------------------
# NMS
# ---------------------------------------------------------------------------------------------
def run_nms(K, c):
    boxes, scores, labels, num, inv = (torch.from_numpy(c[k]).cuda() for k in ("boxes", "scores", "labels", "num", "inv_scale"))
    nbytes = boxes.shape[0] * boxes.shape[1] * 48
    ws = dirty(K, "predict_nms", nbytes)
    d, l, n = K.predict_nms(boxes, scores, labels, num, inv, c["min_bbox_size"], c["iou_thr"], c["max_per_img"])
    torch.cuda.synchronize()
    same_ws(K, "predict_nms", nbytes, ws, boxes)                    # the launch ran in the dirtied buffer
    return d.cpu(), l.cpu(), n.cpu()


def assert_nms_equal(got, want, what):
    (d, l, n), (wd, wl, wn) = got, want[:3]
    assert torch.equal(n, wn), (what, n.tolist(), wn.tolist())
    assert l.dtype == torch.int64 and torch.equal(l, wl), what                                # labels, and zeros past the count
    if not torch.equal(d.view(torch.int32), wd.view(torch.int32)):                           # bit-equal, and zeros past the count
        bad = (d.view(torch.int32) != wd.view(torch.int32)).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} elements differ; first at {i}: got {float(d[i])!r}, want {float(wd[i])!r}")


@pytest.mark.parametrize("name", R.NMS_CASE_NAMES)
def test_nms_exact(K, name):
    c = R.nms_cases()[name]
    want = R.nms_case_ref(name)
    got = run_nms(K, c)
    assert_nms_equal(got, want, name)
    for n in range(len(c["num"])):
        k = int(got[2][n])
        assert (got[0][n, k:] == 0).all() and (got[1][n, k:] == 0).all()
        assert k == min(want[3][n][1], c["max_per_img"])


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_nms_on_the_reference_rows_of_every_topk_case(K, name):
    """erd_predict_nms on exactly the rows the top-k reference says erd_predict_topk writes (fp64-rounded scores)"""
    case = R.CASES[name]
    _, ref = R.case_data(name)
    boxes, scores, labels, num = R.topk_rows(case, ref)
    c = dict(boxes=boxes, scores=scores, labels=labels, num=num, inv_scale=R.inv_scale_of(case),
             min_bbox_size=case["min_bbox_size"], iou_thr=case["iou_thr"], max_per_img=case["max_per_img"])
    assert_nms_equal(run_nms(K, c), R.case_nms_ref(case, boxes, scores, labels, num), name)


# ---------------------------------------------------------------------------------------------
# composition
# ---------------------------------------------------------------------------------------------
def assert_detections(case, inp, ref, dets, det_labels, det_num, what):
    """against O.predict_single per image: labels exact, boxes bit-equal; scores within the table bound of the fp64-rounded ones"""
    wd, wl, wn, _ = R.case_nms_ref(case, *R.topk_rows(case, ref))
    for n in range(len(ref)):
        ob, os_, ol = R.oracle_single(case, inp, n)
        c = int(det_num[n])
        assert c == len(os_) == int(wn[n]), (what, n, c, len(os_))
        assert torch.equal(det_labels[n, :c], ol), (what, n)
        assert torch.equal(dets[n, :c, :4].view(torch.int32), ob.view(torch.int32)), (what, n)
        if c:
            err = R.ulps(dets[n, :c, 4].numpy(), wd[n, :c, 4].numpy())
            assert int(err.max()) <= R.SCORE_ULPS, (what, n, int(err.max()))
            assert float((dets[n, :c, 4] - os_).abs().max()) <= 1e-6
        assert (dets[n, c:] == 0).all() and (det_labels[n, c:] == 0).all()


@pytest.mark.parametrize("name", ["compose_c80", "compose_c70_noclamp", "nms_pre_100", "nms_pre_1024", "C3_lv65"])
def test_topk_then_nms_equals_oracle(K, name):
    case = R.CASES[name]
    inp, ref = R.case_data(name)
    tb = int(K._lib.load().erd_predict_ws_bytes(3, 5, case["nms_pre"]))
    tws = dirty(K, "predict", tb)
    boxes, scores, labels, num = K.predict_topk(torch.from_numpy(inp["cls"]).cuda(), torch.from_numpy(inp["bbox"]).cuda(),
                                                anchors_of(case["sizes"]), list(case["sizes"]), list(R.STRIDES),
                                                torch.from_numpy(inp["img_hw"]).cuda(), case["score_thr"], case["nms_pre"])
    same_ws(K, "predict", tb, tws, boxes)
    nws = dirty(K, "predict_nms", 3 * 5 * case["nms_pre"] * 48)
    d, l, n = K.predict_nms(boxes, scores, labels, num, torch.from_numpy(R.inv_scale_of(case)).cuda(), case["min_bbox_size"],
                            case["iou_thr"], case["max_per_img"])
    same_ws(K, "predict_nms", 3 * 5 * case["nms_pre"] * 48, nws, boxes)
    assert_detections(case, inp, ref, d.cpu(), l.cpu(), n.cpu(), name)


def test_head_predict_by_feat_equals_oracle_c70():
    """the same through GFLHead.predict_by_feat (its own anchors, inverse scale factors and level concatenation), C = 70"""
    from erd_amd import MODELS
    name = "compose_c70_noclamp"
    case = R.CASES[name]
    inp, ref = R.case_data(name)
    cfg = dict(nms_pre=case["nms_pre"], min_bbox_size=case["min_bbox_size"], score_thr=case["score_thr"],
               nms=dict(type="nms", iou_threshold=case["iou_thr"]), max_per_img=case["max_per_img"])
    head = MODELS.build(dict(type="GFLHead", num_classes=case["C"], in_channels=256, test_cfg=cfg)).cuda()
    off = R.level_offsets(case["sizes"])
    maps = lambda x: [torch.from_numpy(x[:, off[l]:off[l + 1]].reshape(3, h, w, -1)).permute(0, 3, 1, 2).contiguous().cuda()
                      for l, (h, w) in enumerate(case["sizes"])]
    metas = [dict(img_shape=tuple(float(v) for v in inp["img_hw"][n]), scale_factor=tuple(case["scale_factor"][n]))
             for n in range(3)]
    res = head.predict_by_feat(maps(inp["cls"]), maps(inp["bbox"]), batch_img_metas=metas, rescale=True)
    P = case["max_per_img"]
    d, l, num = torch.zeros(3, P, 5), torch.zeros(3, P, dtype=torch.int64), torch.zeros(3, dtype=torch.int32)
    for n, r in enumerate(res):
        c = len(r.scores)
        d[n, :c, :4], d[n, :c, 4], l[n, :c], num[n] = r.bboxes.cpu(), r.scores.cpu(), r.labels.cpu(), c
    assert_detections(case, inp, ref, d, l, num, name)
