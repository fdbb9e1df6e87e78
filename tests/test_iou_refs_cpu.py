"""CPU: IoULoss / DIoULoss / CIoULoss -- the restatement of tests/iou_refs.py against the reference's own values (fixture F14,
tools/gen_iou_loss_golden.py; the live reference where its tree is present), E32 per kind, the exclusion condition, the planted
mistakes, the registry / config surface and the static resources of the kernels that carry the box term.  The kernels themselves
are checked on the GPU (tests/test_gpu_iou_loss.py)."""
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest
import torch

import iou_refs as IR
import leaf_refs as R
from e2e_util import ROOT
from oracle import ref_stub

F14 = os.path.join(ROOT, "tests", "golden", "f14_iou_losses.npz")
CFG_CIOU = os.path.join(ROOT, "configs", "gfl_increment", "gfl_r50_fpn_1x_coco_first_40_incre_last_40_cats_ciou.py")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
LOSS_WEIGHT = 2.0


def _same(a, b):
    """bit-equal, NaN where the other is NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.array_equal(a, b, equal_nan=True))


def _restated_values(kind, c):
    rows, grad = IR.restate(kind, c, R.F32)
    out = {"rows": rows.numpy(), "grad": grad.numpy()}
    for i, (reduction, avg_factor, form) in enumerate(IR.MODULE_RUNS):
        out[f"run{i}"] = IR.module_forward(kind, c.pred, c.target, IR.module_weight(c, form), avg_factor, reduction, LOSS_WEIGHT).numpy()
    return out


@pytest.mark.parametrize("kind", IR.KINDS)
def test_restatement_equals_the_reference_fixture(kind):
    g = np.load(F14)
    for c in IR.cases():
        for k, v in _restated_values(kind, c).items():
            assert _same(v, g[f"{kind}.{c.name}.{k}"]), (kind, c.name, k)


@pytest.mark.skipif(not ref_stub.available(), reason="reference tree not present")
@pytest.mark.parametrize("kind", IR.KINDS)
def test_restatement_equals_the_live_reference(kind):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_iou_loss_golden as G
    ref = ref_stub.load_reference()
    assert G.IR_LOSS_WEIGHT == LOSS_WEIGHT
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for c in IR.cases():
            live = G.reference_values(ref, kind, c)
            for k, v in _restated_values(kind, c).items():
                assert _same(v, live[k]), (kind, c.name, k)


def test_swap_box_loss_drives_the_oracle_and_restores_it():
    from oracle import erd_oracle as O
    c = IR.cases()[3]
    w = torch.rand(c.n, generator=R._gen(1))
    before = O.giou_loss_module
    want_giou = before(c.pred, c.target, w, 3.0)
    for kind in IR.KINDS:
        with IR.swap_box_loss(kind):
            got = O.giou_loss_module(c.pred, c.target, w, 3.0)
        assert torch.equal(got, IR.module_forward(kind, c.pred, c.target, w, 3.0, "mean", 2.0)) and not torch.equal(got, want_giou)
    with IR.swap_box_loss("iou", mode="square"):
        assert torch.equal(O.giou_loss_module(c.pred, c.target, w, 3.0), IR.module_forward("iou_square", c.pred, c.target, w, 3.0, "mean", 2.0))
        assert float(O.giou_loss_module(c.pred, c.target, torch.zeros(c.n), 3.0)) == 0.0
    assert O.giou_loss_module is before and torch.equal(before(c.pred, c.target, w, 3.0), want_giou)


def test_compose_under_a_kind_changes_the_box_term_only():
    import loss_refs as LR
    names = [c.name for c in LR.cases()]
    c = LR.cases()[names.index("one_pos")]
    base = LR.compose(c, R.F64)
    L = c.nlvl
    for kind in IR.KINDS:
        r = IR.compose(c, R.F64, kind, want_scales=True)
        assert torch.equal(r.score, base.score) and torch.equal(r.wt, base.wt) and torch.equal(r.qfl, base.qfl) and torch.equal(r.dfl, base.dfl)
        assert torch.equal(r.dcls, base.dcls) and torch.equal(r.sums[:, [0, 2, 3]], base.sums[:, [0, 2, 3]])
        keep = [i for i in range(len(base.losses)) if not L <= i < 2 * L]
        assert torch.equal(r.losses[keep], base.losses[keep])
        assert not torch.equal(r.giou, base.giou) and not torch.equal(r.dbbox, base.dbbox)
        # the rows are the kind's, and the whole functions of the oracle agree with the composition under the swap
        lv = r.lv[1]
        assert torch.equal(lv.giou[lv.pos], IR.rows_fn(kind, lv.dec, lv.tgt))
    from oracle import erd_oracle as O
    assert O.bbox_overlaps is LR.O.bbox_overlaps and LR._giou_scales is R._giou_scales


def test_chain_cases_reach_every_branch_of_the_box_term():
    """the fused-chain cases hold positives with IoU above AND below 0.5 and v > 0, so CIoU's alpha term is live (its rows differ
    from DIoU's there and only there), every row of every kind is finite in fp32, and the no-positive case has none"""
    cs = IR.chain_cases()
    assert [int(c.num_pos.sum()) for c in cs] == [5, 0, 5] and [c.distill for c in cs] == [True, True, False]
    assert cs[0].A == 84 and cs[0].cls_shift == 1
    for i in (0, 2):
        d, ci = IR.compose(cs[i], R.F32, "diou"), IR.compose(cs[i], R.F32, "ciou")
        pos = cs[i].labels != cs[i].c_all
        live = (ci.giou != d.giou) & pos
        assert bool((ci.score[live] > 0.5).all()) and int(live.sum()) == 2 and bool((ci.score[pos & ~live] < 0.5).all())
        for kind in IR.KINDS:
            r = IR.compose(cs[i], R.F32, kind)
            assert bool(torch.isfinite(r.giou).all()) and bool(torch.isfinite(r.dbbox).all()), kind


def test_e32_and_the_exclusion_condition():
    """E32 per kind (printed); a row is excluded only where the CPU fp32 evaluation is not finite: exactly every copy of
    BOX_FAMILY[0] (two identical boxes) under CIoU, no row under DIoU or IoU, none in the random table.  At most 1 row in 17."""
    for kind in IR.KINDS:
        er, eg = IR.e32(kind)
        print(f"\n[iou] {kind:11s} E32 rows {er:.3e}  gradient {eg:.3e}")
        assert 0.0 < er < 1e-5 and 0.0 < eg < 1e-5          # fp32: a handful of roundings of the row's magnitude
        for c, rows, grad, rs, gs, excl in IR.ref64(kind):
            want = IR.family_row0(c) if kind == "ciou" else torch.zeros(c.n, dtype=torch.bool)
            assert torch.equal(excl, want), (kind, c.name)
            assert int(excl.sum()) * 17 <= c.n + 16
            assert bool(torch.isfinite(rows).all()) and bool(torch.isfinite(grad).all())       # the fp64 evaluation is finite everywhere
            r32, g32 = IR.restate(kind, c, R.F32)
            assert bool(torch.isnan(r32[excl]).all()) and bool(torch.isnan(g32[excl]).all())


@pytest.mark.parametrize("mut,kind", [(m, k) for m, ks in IR.MUTATIONS.items() for k in ks])
def test_planted_mistakes_break_the_rule(mut, kind):
    er, eg = IR.e32(kind)
    fr, fg = IR.figures(kind, lambda c: IR.restate(kind, c, R.F32, mut=mut))
    assert fr > R.FACTOR * er or fg > R.FACTOR * eg, (mut, kind, fr / er, fg / eg)


def test_the_unmutated_restatement_passes_the_rule_it_defines():
    for kind in IR.KINDS:
        er, eg = IR.e32(kind)
        fr, fg = IR.figures(kind, lambda c: IR.restate(kind, c, R.F32))
        assert fr <= er and fg <= eg


# ---- registry and config ------------------------------------------------------------------------------------------------
def test_registry_builds_the_three_losses_with_reference_defaults():
    from erd_amd import MODELS
    m = MODELS.build(dict(type="IoULoss"))
    assert (m.mode, m.linear, m.eps, m.reduction, m.loss_weight) == ("log", False, 1e-6, "mean", 1.0)
    for t in ("DIoULoss", "CIoULoss"):
        m = MODELS.build(dict(type=t))
        assert (m.eps, m.reduction, m.loss_weight) == (1e-6, "mean", 1.0)
        assert list(m.state_dict()) == []
    m = MODELS.build(dict(type="IoULoss", mode="square", eps=1e-3, loss_weight=2.5, reduction="sum"))
    assert (m.mode, m.eps, m.loss_weight, m.reduction) == ("square", 1e-3, 2.5, "sum")
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        m = MODELS.build(dict(type="IoULoss", linear=True))
    assert m.mode == "linear" and m.linear is True and any("deprecated" in str(x.message) for x in w)
    with pytest.raises(AssertionError):
        MODELS.build(dict(type="IoULoss", mode="cubic"))
    for t in ("BoundedIoULoss", "EIoULoss"):               # out of scope: they keep failing as before
        with pytest.raises(KeyError):
            MODELS.build(dict(type=t))


def _head_cfg(loss_bbox):
    return dict(type="GFLHead", num_classes=4, in_channels=256, loss_bbox=loss_bbox,
                train_cfg=dict(assigner=dict(type="ATSSAssigner", topk=9), allowed_border=-1, pos_weight=-1, debug=False))


def test_heads_resolve_loss_bbox_to_kind_and_eps():
    from erd_amd import MODELS
    from erd_amd import kernels as K
    want = [(dict(type="GIoULoss", loss_weight=2.0), (IR.KIND_ID["giou"], 1e-6)),
            (dict(type="IoULoss", loss_weight=2.0), (IR.KIND_ID["iou_log"], 1e-6)),
            (dict(type="IoULoss", mode="linear", eps=1e-4), (IR.KIND_ID["iou_linear"], 1e-4)),
            (dict(type="IoULoss", mode="square"), (IR.KIND_ID["iou_square"], 1e-6)),
            (dict(type="DIoULoss", eps=1e-7), (IR.KIND_ID["diou"], 1e-7)),
            (dict(type="CIoULoss", loss_weight=2.0), (IR.KIND_ID["ciou"], 1e-6))]
    for cfg, kind in want:
        head = MODELS.build(_head_cfg(cfg))
        assert tuple(head._box_loss) == kind, cfg
    assert K.BOX_LOSS_GIOU == (IR.KIND_ID["giou"], 1e-6)
    assert (K.BOX_IOU_LOG, K.BOX_IOU_LINEAR, K.BOX_IOU_SQUARE, K.BOX_DIOU, K.BOX_CIOU) == tuple(IR.KIND_ID[k] for k in IR.KINDS)
    for t in ("DIoULoss", "CIoULoss", "IoULoss", "GIoULoss"):
        with pytest.raises(NotImplementedError, match="reduction"):
            MODELS.build(_head_cfg(dict(type=t, reduction="sum")))
    with pytest.raises(NotImplementedError, match="eps"):                    # the GIoU refusal stays
        MODELS.build(_head_cfg(dict(type="GIoULoss", eps=1e-7)))


def test_header_enum_matches_the_bindings():
    header = open(os.path.join(ROOT, "include", "erd_hip.h")).read()
    for name, kind in (("ERD_BOX_GIOU", "giou"), ("ERD_BOX_IOU_LOG", "iou_log"), ("ERD_BOX_IOU_LINEAR", "iou_linear"),
                       ("ERD_BOX_IOU_SQUARE", "iou_square"), ("ERD_BOX_DIOU", "diou"), ("ERD_BOX_CIOU", "ciou")):
        assert int(re.search(name + r" = (\d+)", header).group(1)) == IR.KIND_ID[kind]


def test_ciou_config_loads_and_its_model_builds():
    from erd_amd import Config, MODELS
    from e2e_util import CFG_INCRE
    cfg = Config.fromfile(CFG_CIOU)
    assert cfg.model.bbox_head.loss_bbox == dict(type="CIoULoss", loss_weight=2.0)
    base = Config.fromfile(CFG_INCRE).to_dict()
    ours = cfg.to_dict()
    ours["model"]["bbox_head"]["loss_bbox"] = base["model"]["bbox_head"]["loss_bbox"]
    ours.pop("filename"), base.pop("filename")
    assert ours == base                                                    # only loss_bbox is overridden
    cfg.model.latest_model_flag = False
    model = MODELS.build(cfg.model)
    assert type(model.bbox_head.loss_bbox).__name__ == "CIoULoss" and model.bbox_head._box_loss == (IR.KIND_ID["ciou"], 1e-6)
    cfg0 = Config.fromfile(CFG_INCRE)
    cfg0.model.latest_model_flag = False
    assert list(model.state_dict()) == list(MODELS.build(cfg0.model).state_dict())       # loss modules hold no parameters


# ---- static resources ----------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.isfile(HIPCC), reason="hipcc not present")
@pytest.mark.parametrize("src,pattern,count", [("losses.hip", "gfl_losses_kernel", 12), ("leaf_ops.hip", "iou_loss_kernel", 5)])
def test_box_loss_kernels_use_no_scratch(tmp_path, src, pattern, count):
    """every instantiation of gfl_losses_kernel (forward / backward x six kinds) and of the stand-alone iou_loss_kernel (five kinds)
    keeps its state in registers: no scratch"""
    out = tmp_path / (src + ".s")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-function", "-ffp-contract=off", "-S",
                        "--cuda-device-only", "-o", str(out), src], cwd=os.path.join(ROOT, "erd_amd", "csrc"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    found = re.findall(r"\.amdhsa_kernel (\S*" + pattern + r"\S*)\n(.*?)\.end_amdhsa_kernel", open(out).read(), re.S)
    assert len(found) == count, [n for n, _ in found]
    for name, body in found:
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1))
        print(f"\n[iou] {name}: {vgpr} VGPRs, scratch {scratch}")
        assert scratch == 0, name
