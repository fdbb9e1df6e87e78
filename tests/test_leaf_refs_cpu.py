"""CPU: the references of tests/leaf_refs.py are right and its rule bites (no GPU, no erd_amd).

  * the fp64 references reproduce every value and gradient the REAL reference produced for fixture F1 (f1_leaf.npz)
  * the case tables contain what they claim
  * the restatements of the kernels are the same formulas (fp64: equal to the oracle under autograd to 1e-9 of the row scale;
    fp32: inside the 4 x E32 rule, or bit-equal to the oracle's fp32 where equality is the rule)
  * negative controls: every planted mistake breaks the rule on at least one case of its operator"""
from types import SimpleNamespace as NS

import pytest
import torch

import golden_inputs as G
import leaf_refs as R
from oracle import erd_oracle as O

F32, F64 = R.F32, R.F64
HALF_ULP = 2.0 ** -24


def _t(a):
    return torch.from_numpy(a)


# ---- fixture F1 ------------------------------------------------------------------------------------------------------
def _f1_rule_cases():
    d = G.f1_inputs()
    e = R.EPS32
    return d, {
        "qfl": NS(n=300, C=40, pred=d["qfl_pred"], label=d["qfl_label"], score=d["qfl_score"], coef=d["qfl_weight"] / (37.0 + e)),
        "dfl": NS(m=384, nb=17, pred=d["dfl_pred"], target=d["dfl_label"], coef=0.25 * d["dfl_weight"] / (4.0 + e)),
        "kd": NS(m=256, nb=17, T=10.0, pred=d["kd_pred"], soft=d["kd_soft"], coef=0.25 * d["kd_weight"] / (4.0 + e)),
        "giou": NS(n=128, pred=d["box_a"], target=d["box_b"], coef=2.0 * d["box_w"] / (1.0 + e), eps=1e-6),
        "integral": NS(m=384, nb=17, x=d["dfl_pred"], dy=d["dist"][:96].reshape(-1)),
    }


def test_fp64_references_reproduce_fixture_f1(golden):
    """the fixture holds what the reference computed in fp32: each row within 4 x E32 of its scale (the rule itself) plus the
    half ulp of its storage; a reduced loss within the same share of sum_i |coef_i| scale_i"""
    g = golden("f1_leaf.npz")
    d, cases = _f1_rule_cases()
    keys = {"qfl": ("qfl_rows", "qfl_grad", "qfl_loss"), "dfl": (None, "dfl_grad", "dfl_loss"), "kd": (None, "kd_grad", "kd_loss"),
            "giou": (None, "giou_grad", "giou_loss"), "integral": ("integral", "integral_grad", None)}
    for op, c in cases.items():
        _, oracle, scales, _ = R.RULE_OPS[op]
        rows, grad = oracle(c, F64)
        rs, gs = scales(c)
        er, eg = R.e32(op)
        kr, kg, kl = keys[op]
        if kr:
            assert R.nerr(_t(g[kr]).reshape(rows.shape), rows, rs) <= R.FACTOR * er + HALF_ULP, op
        assert R.nerr(_t(g[kg]).reshape(grad.shape), grad, gs) <= R.FACTOR * eg + HALF_ULP, op
        if kl:
            coef = c.coef.double()
            loss = float((rows * coef).sum())
            tol = (R.FACTOR * er + HALF_ULP) * float((rs * coef.abs()).sum()) + HALF_ULP * abs(loss)
            assert abs(float(g[kl]) - loss) <= tol, (op, float(g[kl]), loss, tol)
    a, b = d["box_a"].double(), d["box_b"].double()
    # iou = overlap / union of valid boxes: at most 8 roundings of half an ulp each on a value <= 1
    assert (_t(g["iou_aligned"]) - O.bbox_overlaps(a, b, is_aligned=True)).abs().max() <= 8 * HALF_ULP
    assert (_t(g["iou_pair"]) - O.bbox_overlaps(a[:16], b[:8])).abs().max() <= 8 * HALF_ULP
    assert R.nerr(_t(g["giou_aligned"]), O.bbox_overlaps(a, b, mode="giou", is_aligned=True), torch.full((128,), 3.0)) <= 8 * HALF_ULP
    assert float(g["giou_zero_weight"]) == 0.0
    # one rounded subtraction each (the clamp bound 16 - 0.1 is one more rounded number)
    ref = O.distance2bbox(d["pts"].double(), d["dist"].double())
    assert bool(((_t(g["distance2bbox"]) - ref).abs() <= HALF_ULP * ref.abs()).all())
    ref = O.bbox2distance(d["pts"].double(), d["box_a"].double(), 16, 0.1)
    assert bool(((_t(g["bbox2distance"]) - ref).abs() <= HALF_ULP * ref.abs().clamp(min=1.0)).all())


# ---- the tables hold what they claim -----------------------------------------------------------------------------------
def test_case_tables_contain_their_edges():
    q = R.qfl_cases()
    assert [(c.n, c.C) for c in q[:len(R.QFL_SHAPES)]] == R.QFL_SHAPES
    assert any(c.C > 64 and bool(((c.label >= 64) & (c.label < c.C)).any()) for c in q)
    big = [c for c in q if c.C >= 40 and c.n >= 5]
    for c in big:
        for v in (0, c.C - 1, c.C, c.C + 5, -1):
            assert bool((c.label == v).any()) or c.name.endswith("bg"), (c.name, v)
        assert bool((c.score == 0).any()) and bool((c.score == 1).any())
    assert any(bool((c.label == c.C).all()) for c in q)
    c = q[-2]
    for v in (0.0, 30.0, -30.0, 90.0, -90.0):
        assert bool((c.pred == v).any())
    assert bool((c.coef == 0).any()) and c.n % 4 != 0 and c.n > 1024
    for c in R.dfl_cases():
        ts = set(c.target.tolist())
        want = {0.0, float(c.nb - 2), float(torch.tensor(c.nb - 1.1, dtype=F32))} if c.m >= 8 else {0.0}
        assert want <= ts, (c.name, want - ts)
        assert float(c.target.max()) <= c.nb - 1.1 + 1e-6 and float(c.target.min()) >= 0
        if c.m >= 8:
            assert bool((c.pred == -80).all(1).any()) and bool((c.pred > 30).any()) and bool((c.pred == 0.75).all(1).any())
    assert any(bool((c.target == float(torch.tensor(15.9, dtype=F32))).any()) for c in R.dfl_cases() if c.nb == 17)
    kd = R.kd_cases()
    assert {c.T for c in kd} == {1.0, 10.0}
    assert any(bool((c.pred == c.soft).all(1).any()) for c in kd) and any(bool((c.coef == 0).any()) for c in kd)
    # at least one teacher probability that is exactly 0.0 in fp32
    assert any(bool((torch.softmax(c.soft / c.T, 1) == 0).any()) for c in kd if c.T == 1.0)
    for c in R.integral_cases():
        assert bool((c.x == 0.75).all(1).any()) and bool((c.x[:, 0] > 30).any()) and bool((c.x[:, -1] > 30).any())
    # boxes: a tie on every coordinate somewhere, w == 0, containment, union < eps, inverted
    a, b = R.family_boxes(len(R.BOX_FAMILY))
    for k in range(4):
        assert bool(((a[:, k] == b[:, k]) & (a != b).any(1)).any()), k
    assert bool((a == b).all(1).any())
    w = torch.minimum(a[:, 2], b[:, 2]) - torch.maximum(a[:, 0], b[:, 0])
    h = torch.minimum(a[:, 3], b[:, 3]) - torch.maximum(a[:, 1], b[:, 1])
    assert bool(((w == 0) & (h > 0)).any()) and bool(((h == 0) & (w > 0)).any()) and bool((w < 0).any())
    assert bool((a[:, 2] < a[:, 0]).any()) and bool(((a[:, 2] == a[:, 0]) & (a[:, 3] == a[:, 1])).any())
    aa, bb = R.family_boxes(2 * len(R.BOX_FAMILY), affine=True)
    assert bool((aa != aa.round()).any()) and bool((aa[len(R.BOX_FAMILY)] == bb[len(R.BOX_FAMILY)]).all())
    # coder: decoded coordinates exactly 0, exactly on the border, outside both ways
    c = R.d2b_case(257)
    box = O.distance2bbox(c.pts, c.dist)
    assert torch.equal(box, c.want)
    H, W = R.MAX_SHAPE
    for k, lim in enumerate((W, H, W, H)):
        col = box[:, k]
        assert bool((col == 0).any()) and bool((col == lim).any()) and bool((col < 0).any()) and bool((col > lim).any())
    for max_dis, eps in R.B2D_PARAMS[1:]:
        c = R.b2d_case(257, max_dis, eps)
        raw = R.b2d_oracle(NS(pts=c.pts, box=c.box, max_dis=None, eps=eps), F32)
        assert bool((raw == c.hi).any()) and bool((raw == 0).any()) and bool((raw < 0).any()) and bool((raw > c.hi).any())
        # the kernel's bound max_dis - eps in fp32 arithmetic is the fp32 value of the reference's double max_dis - eps
        assert c.hi == float(torch.tensor(max_dis - eps, dtype=F32))


# ---- the restatements are the operators ---------------------------------------------------------------------------------
@pytest.mark.parametrize("op", sorted(R.RULE_OPS))
def test_restatement_is_the_oracle(op):
    """in fp64 the kernel-order restatement equals the oracle under autograd (hand-written gradient rules included: ties, clamps
    at equality, the gated enclosing-area term); in fp32 it is inside the rule the kernel is held to"""
    restate = R.RULE_OPS[op][3]
    r64 = R.figures(op, lambda c: restate(c, dtype=F64))
    assert max(r64) <= 1e-9, (op, r64)
    er, eg = R.e32(op)
    fr, fg = R.figures(op, restate)
    print(f"\n[{op}] E32 rows {er:.3e} grad {eg:.3e} | fp32 restatement rows {fr:.3e} grad {fg:.3e}")
    assert 0 < er < 1e-5 and 0 < eg < 1e-5, "E32 out of the range of fp32 rounding: a scale or a case is wrong"
    if op == "giou":
        for c in R.giou_cases():        # rows: equality rule
            assert torch.equal(restate(c)[0], R.giou_oracle(c, F32)[0])
    else:
        assert fr <= R.FACTOR * er, (op, fr, er)
    assert fg <= R.FACTOR * eg, (op, fg, eg)


@pytest.mark.parametrize("op,mut", [(op, m) for op in sorted(R.MUTATIONS) for m in R.MUTATIONS[op]])
def test_negative_controls_break_the_rule(op, mut):
    restate = R.RULE_OPS[op][3]
    er, eg = R.e32(op)
    fr, fg = R.figures(op, lambda c: restate(c, mut))
    print(f"\n[{op}/{mut}] rows {fr:.3e} (bound {R.FACTOR * er:.3e}) grad {fg:.3e} (bound {R.FACTOR * eg:.3e})")
    if op == "giou":                    # the planted mistakes are in the gradient rules
        assert fg > R.FACTOR * eg
    elif mut in ("right_bin_dl", "b_not_b_minus_e"):
        assert fg > R.FACTOR * eg and fr <= R.FACTOR * er
    elif mut == "t_log_t":              # only the row value takes the log of the teacher's probability
        assert fr > R.FACTOR * er and fg <= R.FACTOR * eg
    else:
        assert fr > R.FACTOR * er and fg > R.FACTOR * eg


def test_kd_equal_rows_have_an_exactly_zero_restated_gradient():
    for c in R.kd_cases():
        rows, grad = R.kd_restate(c)
        same = (c.pred == c.soft).all(1)
        assert bool((grad[same] == 0).all()) and bool((rows[same] == 0).all())


# ---- equality rule --------------------------------------------------------------------------------------------------------
def test_equality_restatements_are_the_oracle_in_fp32():
    for n in (1, 255, 257):
        a, b = R.family_boxes(n, affine=True)
        for mode in ("iou", "giou"):
            assert torch.equal(R.overlaps_restate(a, b, mode, True), O.bbox_overlaps(a, b, mode=mode, is_aligned=True))
    a, b = R.random_boxes(300, 5300)
    assert torch.equal(R.overlaps_restate(a, b, "giou", True), O.bbox_overlaps(a, b, mode="giou", is_aligned=True))
    for m, n in R.PAIR_SHAPES:
        a, b = R.pair_boxes(m, n)
        for mode in ("iou", "giou"):
            got = R.overlaps_restate(a, b, mode, False)
            assert got.shape == (m, n) and torch.equal(got, O.bbox_overlaps(a, b, mode=mode))
    for n in R.CODER_N:
        c = R.d2b_case(n)
        for ms in (None, R.MAX_SHAPE):
            b32, g32 = R.d2b_oracle(c, ms, F32)
            b64, g64 = R.d2b_oracle(c, ms, F64)
            assert torch.equal(b32.double(), b64) and torch.equal(g32.double(), g64)      # exact at these values
            if ms is not None and n > 1:
                assert not torch.equal(R.d2b_oracle(c, ms, F32, mut="zero_at_border")[1], g32)
                H, W = ms
                lim = torch.tensor([W, H, W, H])
                at = (c.want == 0) | (c.want == lim)
                sign = torch.tensor([-1.0, -1.0, 1.0, 1.0])
                assert torch.equal(g32[at], (c.dout * sign)[at])                            # the gradient passes at equality
    for n in R.SMALL_N:
        for weighted in (False, True):
            c = R.small_case(n, weighted)
            w = 1.0 if c.weight is None else c.weight.double()
            ref = c.rows.double() * c.scale * w
            assert bool(((R.rows_mul_restate(c) - ref).abs() <= 2 * HALF_ULP * ref.abs()).all())
            ref = float(c.upstream) * c.scale * w * torch.ones(n, dtype=F64)
            assert bool(((R.loss_coef_restate(c) - ref).abs() <= 2 * HALF_ULP * ref.abs()).all())


def test_weighted_sum_cases_and_negative_control():
    differs = 0
    for n in R.WSUM_N:
        for weighted in (False, True):
            c = R.wsum_case(n, weighted)
            assert float(R.wsum_restate(c)) == c.want
            differs += weighted and float(R.wsum_restate(c, "weight_ignored")) != c.want
    assert differs >= 4
    c = R.wsum_real_case()
    assert abs(float(R.wsum_restate(c)) - c.want) <= HALF_ULP * abs(c.want)
    assert abs(float(R.wsum_restate(c, "weight_ignored")) - c.want) > 0.1 * abs(c.want)


def test_reduction_rules_follow_the_reference_order():
    rows, w = torch.tensor([1.0, 2.0, 4.0], dtype=F64), torch.tensor([0.5, 0.0, 2.0], dtype=F64)
    assert torch.equal(R.reduce_ref(rows, w, "none", None, 2.0), 2.0 * rows * w)
    assert torch.equal(R.reduce_ref(rows, w, "none", 5.0), rows * w)                 # utils.py:60-61: 'none' ignores avg_factor
    assert float(R.reduce_ref(rows, w, "sum", None)) == 8.5
    assert float(R.reduce_ref(rows, None, "mean", None)) == pytest.approx(7.0 / 3.0)
    assert float(R.reduce_ref(rows, w, "mean", 4.0, 3.0)) == pytest.approx(3.0 * 8.5 / (4.0 + R.EPS32))
    with pytest.raises(ValueError):
        R.reduce_ref(rows, w, "sum", 4.0)
    for red, af in (("sum", None), ("mean", None), ("mean", 4.0)):
        assert float(R.reduce_ref(rows, w, red, af, 3.0)) == pytest.approx(R.reduce_scale(red, af, 3, 3.0) * 8.5)


def test_atss_keys_decode_to_their_table():
    c = R.atss_case(257)
    assert bool((c.keys == 0).any()) and bool((c.gt_inds == 1).any()) and bool((c.gt_inds == len(R.ATSS_GT_LABELS)).any())
    k = c.keys[0].item() & ((1 << 64) - 1)
    assert 0xffffffff - (k & 0xffffffff) == 0 and torch.tensor(k >> 32, dtype=torch.int64).to(torch.int32).view(F32).item() == c.max_ov[0].item()
