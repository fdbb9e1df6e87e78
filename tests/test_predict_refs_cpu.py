"""CPU: the references of tests/test_gpu_predict_exact.py (tests/predict_refs.py) are what they claim to be.

The score table keeps its 128-ulp separation and every threshold its 64-ulp distance, every logit is fp32-exact and the one-hot box
logits decode exactly in O.integral; topk_ref followed by nms_ref equals O.predict_single (the restatement fixture F8 pins to the
reference project) on every top-k and composition case; and a census computed from the reference's path report alone shows that the
case list still reaches every path and edge the GPU file is there for."""
import numpy as np
import pytest
import torch

import predict_refs as R
from oracle import erd_oracle as O


def test_table_separation_and_thresholds():
    assert len(R.TABLE) == 44 and len(set(R.TABLE.tolist())) == 44
    assert (R.TABLE.astype(np.float32).astype(np.float64) == R.TABLE).all()              # fp32-exact logits
    assert R.table_separation_ulps() >= 128
    assert R.SCORE_ULPS < R.table_separation_ulps() / 2                                   # a score maps back to one entry
    assert (R.score32(R.TABLE) < 1.0).all() and R.score32(R.INF) == 1.0                   # only +inf scores 1.0
    assert R.score32(-R.INF) == 0.0 and not (R.score32(R.NAN) > 0.0)                      # never selected, even at score_thr 0
    for thr in R.THRESHOLDS:
        assert float(np.float32(thr)) == thr and R.threshold_distance_ulps(thr) >= 64, thr
    assert {c["score_thr"] for c in R.CASES.values()} <= set(R.THRESHOLDS)
    t = torch.from_numpy(R.TABLE.astype(np.float32))
    assert int(R.ulps(t.sigmoid().numpy(), R.score32(R.TABLE)).max()) <= 1                # torch's fp32 sigmoid: within 1 ulp


def test_table_groups_share_the_key_bits_they_are_named_for():
    k2, k1, k0 = (R.key_of(R.score32(g)) for g in (R.P2_GROUP, R.P1_GROUP, R.P0_GROUP))
    assert len(set(k2 >> 10)) == 1 and len(set(k2)) == 8
    assert len(set(k1 >> 21)) == 1 and len(set(k1 >> 10)) == 9
    assert len(set(k0 >> 21)) == 4


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_case_logits_come_from_the_table_and_boxes_decode_exactly(name):
    inp, _ = R.case_data(name)
    allowed = np.concatenate([R.TABLE, [R.INF, -R.INF]])
    cls = inp["cls"].astype(np.float64)
    assert (np.isin(cls, allowed) | np.isnan(cls)).all()
    d = O.integral(torch.from_numpy(inp["bbox"].reshape(-1, 68)))
    assert torch.equal(d, torch.from_numpy(inp["bins"].reshape(-1, 4)).float())           # softmax exactly (1, 0, ...)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_topk_ref_then_nms_ref_equals_oracle(name):
    case = R.CASES[name]
    inp, ref = R.case_data(name)
    off = R.level_offsets(case["sizes"])
    sig = lambda x: torch.from_numpy(np.asarray(x, np.float32)).sigmoid().numpy()         # the oracle's fp32 sigmoid
    for n, row in enumerate(ref):
        for l, r in enumerate(row):                                                      # the selection, index by index
            scores = torch.from_numpy(inp["cls"][n, off[l]:off[l + 1]]).sigmoid()
            s, labels, keep = O.filter_scores_and_topk(scores, case["score_thr"], case["nms_pre"])
            assert np.array_equal((keep * case["C"] + labels).numpy(), r.idx) and np.array_equal(labels.numpy(), r.labels)
            assert len(r.idx) == min(r.total, case["nms_pre"])
            assert int(R.ulps(s.numpy(), r.scores.astype(np.float32)).max(initial=0)) <= 1
    boxes, scores, labels, num = R.topk_rows(case, ref, sig)
    dets, det_labels, det_num, _ = R.case_nms_ref(case, boxes, scores, labels, num)
    for n in range(len(ref)):
        wb, ws, wl = R.oracle_single(case, inp, n)
        c = int(det_num[n])
        assert c == len(ws), (n, c, len(ws))
        assert torch.equal(det_labels[n, :c], wl)
        assert torch.equal(dets[n, :c, :4], wb)                                          # bit-equal boxes
        assert torch.equal(dets[n, :c, 4], ws)                                           # the oracle's own scores


def test_census_of_paths_and_edges():
    tags = R.census()
    assert R.CENSUS_WANTED <= tags, sorted(R.CENSUS_WANTED - tags)
    assert "mixed_launch" in R.census([R.MIXED_CASE])
    sizes = {tuple(c["sizes"]) for c in R.CASES.values()}
    assert sizes == {R.LV5, R.LV65} and all(len(c["recipes"]) == 3 for c in R.CASES.values())


def test_census_of_nms_cases():
    cs = R.nms_cases()
    assert tuple(cs) == R.NMS_CASE_NAMES
    info = {name: R.nms_case_ref(name) for name in cs}
    passed = {k for r in info.values() for k, _ in r[3]}
    assert {0, 1, 1023, 1024, 1025, 2049} <= passed                                      # rows that pass the size filter
    assert cs["batch_5000_0_1"]["num"].tolist() == [5000, 0, 1]
    for name in ("survivors_1_1023_1024", "survivors_1025_2049_0"):                       # the filter drops rows at every wave edge
        c, (dets, _, num, inf) = cs[name], info[name]
        for n in range(3):
            M = int(c["num"][n])
            b = c["boxes"][n, :M] * np.tile(c["inv_scale"][n], 2)
            w, h = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
            i = np.arange(M)
            assert (w[i % 64 == 63] == 4).all() and (h[i % 64 == 0] == 4).all()
            assert (w[i % 64 == 62] == 5).all() and (h[i % 64 == 1] == 5).all()
            assert inf[n][0] == inf[n][1] == int(num[n])                                 # disjoint boxes: the NMS keeps them all
    assert [k for _, k in info["iou_exactly_thr_kept"][3]] == [6, 6, 6]
    assert [k for _, k in info["iou_just_above_thr_suppressed"][3]] == [3, 3, 3]
    assert [k for _, k in info["min_size_minus1_degenerate"][3]] == [7, 7, 7]            # 0 / 0 suppresses nothing
    kept0 = info["max_per_img_equal"][3][0][1]
    assert cs["max_per_img_equal"]["max_per_img"] == kept0 and cs["max_per_img_one_below"]["max_per_img"] == kept0 - 1
    assert info["max_per_img_one"][2].tolist() == [1, 1, 1]
    flips = 0
    for thr in (0.6, 0.5):                                                                # the fp32 class offset decides some pairs
        c = cs[f"labels_79_near_2700_thr{thr}"]
        assert int(c["labels"].max()) == 79 and float(c["boxes"][:, :800].max()) == 2700.0
        for n in range(3):                                                               # the same NMS class by class, no offset
            b = torch.from_numpy(c["boxes"][n, :800]) * torch.from_numpy(np.tile(c["inv_scale"][n], 2))
            s, lab = torch.from_numpy(c["scores"][n, :800]), torch.from_numpy(c["labels"][n, :800]).long()
            alone = sum(len(O.nms_class_offset(b[lab == k], s[lab == k], lab[lab == k] * 0, c["iou_thr"])) for k in lab.unique())
            flips += alone != info[c["name"]][3][n][1]
    assert flips > 0
