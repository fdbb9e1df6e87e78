"""CPU: test-time augmentation (tools/test.py --tta) -- the host restatement of the merge against the reference's own
DetTTAModel (fixture F12, UNPINNED vs mmcv's NMS), the resolution of tta_model / tta_pipeline from a config, the registry
entry and the static resources of erd_tta_merge's kernel.  The kernel itself is checked on the GPU (test_gpu_tta.py)."""
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest

from erd_amd import Config, MODELS
import tta_util as T
from e2e_util import CFG_INCRE, ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CFG_TTA = os.path.join(ROOT, "configs", "gfl_increment", "gfl_r50_fpn_1x_coco_first_40_incre_last_40_cats_tta.py")
F12 = os.path.join(ROOT, "tests", "golden", "f12_tta_merge_unpinned_nms.npz")


@pytest.mark.parametrize("case", range(len(T.F12_CASES)))
def test_restated_merge_equals_reference_fixture(case):
    g = np.load(F12)
    dets, labels, num, flips, ori_w, iou, mpi = T.f12_inputs(case)
    assert np.array_equal(g[f"c{case}_dets"], dets) and np.array_equal(g[f"c{case}_num"], num)   # inputs from the seeds
    for n, (b, s, l) in enumerate(T.merge(dets, labels, num, flips, ori_w, iou, mpi)):
        assert np.array_equal(b.numpy(), g[f"c{case}_i{n}_bboxes"]), (case, n)        # same set, same order, bit-equal
        assert np.array_equal(s.numpy(), g[f"c{case}_i{n}_scores"]) and np.array_equal(l.numpy(), g[f"c{case}_i{n}_labels"])


def test_fixture_covers_the_issue_cases():
    g = np.load(F12)
    flips = [g[f"c{c}_flips"] for c in range(3)]
    assert sorted(len(f) for f in flips) == [2, 2, 6] and all(f.any() and not f.all() for f in flips)
    assert (g["c0_num"] == 0).any() and (g["c0_num"][:, 2] == 0).all() and len(g["c0_i2_scores"]) == 0   # empty view / image
    assert {float(g[f"c{c}_iou_max"][0]) for c in range(3)} == {0.5, 0.6}
    assert len(g["c1_i0_scores"]) == int(g["c1_iou_max"][1]) < g["c1_num"][:, 0].sum()              # the max_per_img cut
    s = np.concatenate([g["c2_dets"][v, 0, :g["c2_num"][v, 0], 4] for v in range(2)])
    assert len(np.unique(s)) < len(s)                                                              # ties across views
    assert len(g["c2_i0_scores"]) < g["c2_num"][:, 0].sum()                                        # cross-view suppression


def _cfg(path=CFG_INCRE):
    return Config.fromfile(path)


def test_resolve_defaults_to_flip_only_at_the_test_scale():
    from erd_amd.datasets import resolve_tta
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        r = resolve_tta(_cfg())
    msgs = [str(x.message) for x in w]
    assert "Cannot find ``tta_model`` in config, we will set it as default." in msgs
    assert "Cannot find ``tta_pipeline`` in config, we will set it as default." in msgs
    assert r["tta_model"] == dict(type="DetTTAModel", tta_cfg=dict(nms=dict(type="nms", iou_threshold=0.5), max_per_img=100))
    assert r["scales"] == [(1333, 800)] and r["flips"] == [True, False]
    c = _cfg()
    c.test_dataloader.dataset.pipeline[1]["scale"] = (666, 400)
    assert resolve_tta(c)["scales"] == [(666, 400)]


def test_resolve_tta_config_gives_three_scales_by_two_flips():
    from erd_amd.datasets import resolve_tta
    with warnings.catch_warnings():
        warnings.simplefilter("error")                     # the config has both: no warning
        r = resolve_tta(_cfg(CFG_TTA))
    assert r["scales"] == [(1333, 800), (666, 400), (2000, 1200)] and r["flips"] == [True, False]
    views = [(s, f) for s in r["scales"] for f in r["flips"]]     # TestTimeAug's product order, scale outermost
    assert views[:3] == [((1333, 800), True), ((1333, 800), False), ((666, 400), True)] and len(views) == 6
    assert r["tta_model"]["tta_cfg"]["nms"]["iou_threshold"] == 0.5


@pytest.mark.parametrize("bad", [
    dict(type="Resize", scale=(1333, 800), keep_ratio=False),
    dict(type="RandomFlip", prob=0.5),
    dict(type="RandomFlip", prob=1.0, direction="vertical"),
    dict(type="PhotoMetricDistortion"),
])
def test_resolve_rejects_unsupported_transforms(bad):
    from erd_amd.datasets import resolve_tta
    c = _cfg(CFG_TTA)
    tta = c.tta_pipeline[1]
    if bad["type"] == "Resize":
        tta["transforms"][0] = [bad]
    elif bad["type"] == "RandomFlip":
        tta["transforms"][1] = [dict(type="RandomFlip", prob=1.0), bad]
    else:
        tta["transforms"].insert(0, [bad])
    with pytest.raises(ValueError, match="--tta"):
        resolve_tta(c)
    c2 = _cfg(CFG_TTA)
    c2.tta_pipeline.insert(1, dict(type="PhotoMetricDistortion"))
    with pytest.raises(ValueError, match="PhotoMetricDistortion"):
        resolve_tta(c2)
    c3 = _cfg(CFG_TTA)
    c3.tta_model = dict(type="OtherTTAModel")
    with pytest.raises(ValueError):
        resolve_tta(c3)


def test_det_tta_model_is_registered_and_rejects_unbuilt_nms():
    assert "DetTTAModel" in MODELS
    teacher_cfg = Config.fromfile(os.path.join(ROOT, "configs", "gfl_increment", "gfl_r50_fpn_1x_coco_first_40_cats.py")).model
    m = MODELS.build(dict(type="DetTTAModel", module=teacher_cfg,
                          tta_cfg=dict(nms=dict(type="nms", iou_threshold=0.5), max_per_img=100)))
    assert type(m.module).__name__ == "GFL" and set(m.state_dict()) == {"module." + k for k in m.module.state_dict()}
    for nms in (dict(type="soft_nms", iou_threshold=0.5), dict(type="nms", iou_threshold=0.5, class_agnostic=True)):
        with pytest.raises(NotImplementedError):
            MODELS.build(dict(type="DetTTAModel", module=teacher_cfg, tta_cfg=dict(nms=nms, max_per_img=100)))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_tta_merge_kernel_fits_static_lds_and_uses_no_scratch(tmp_path):
    """`tta_merge_kernel` keeps up to TTA_LDS_K rank-ordered offset boxes, their scores, merged positions and suppression
    flags in STATIC LDS: within the 64 KB a kernel gets without the dynamic-LDS attribute, no scratch."""
    out = tmp_path / "predict.s"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-function", "-ffp-contract=off", "-S",
                        "--cuda-device-only", "-o", str(out), "predict.hip"], cwd=os.path.join(ROOT, "erd_amd", "csrc"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    m = re.search(r"\.amdhsa_kernel \S*tta_merge_kernel\S*\n(.*?)\.end_amdhsa_kernel", open(out).read(), re.S)
    assert m, "tta_merge_kernel not found"
    lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", m.group(1)).group(1))
    scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(1)).group(1))
    cap = int(re.search(r"constexpr int TTA_LDS_K = (\d+);",
                        open(os.path.join(ROOT, "erd_amd", "csrc", "predict.hip")).read()).group(1))
    assert cap >= 20 * 100 and cap * (16 + 4 + 4 + 1) <= lds <= 65536, (cap, lds)
    assert scratch == 0
