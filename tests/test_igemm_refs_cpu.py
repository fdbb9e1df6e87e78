"""CPU: the references, case table and census of tests/igemm_refs.py -- that the inputs make every kernel's arithmetic exact, that the
reference agrees with a plain matrix product, and that at 256 CUs the cases reach every instantiation erd_conv_igemm's defaults choose
and every work-decomposition, tile-shape, K-axis and epilogue path tests/test_gpu_igemm_exact.py claims to pin."""
import pytest
import torch

import igemm_refs as R


def test_every_value_and_every_sum_is_exact():
    """one bf16 limb holds every multiplicand, no partial sum can leave the integers fp32 holds exactly, and the epilogue's operands
    keep every result a multiple of 1/4 below 2^22 (expected() asserts the latter two on the values themselves)"""
    for case in R.CASES:
        d = R.inputs(case.name)
        for x in d["x"]:
            assert set(x.unique().tolist()) == {-1.0, 0.0, 1.0}
        assert set(d["w"].unique().tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0}
        for t in d["x"] + [d["w"]] + [t for key in ("res", "base", "mask") for t in d.get(key, []) if t is not None]:
            assert torch.equal(t.bfloat16().float(), t)                    # limb 0 is the value, limbs 1 and 2 are zero; bf16 storage is exact
        if "scale" in d:
            assert set(d["scale"].tolist()) <= {0.5, 1.0, 2.0} and torch.equal(d["shift"], d["shift"].round())
        if "alpha" in d:
            assert [float(a) for a in d["alpha"]] == [0.5, 2.0][:len(d["alpha"])]
        assert R.acc_bound(case) * 2 * 2 + 3 * 2 + 4 < 2 ** 22              # (|acc| * scale + |shift|) * alpha + |residual|
        outs, cs = R.expected(case.name)
        assert all(o.dtype == (torch.bfloat16 if case.ob else torch.float32) for o in outs)
        assert cs is None or torch.equal(cs, cs.round())


def test_the_reference_of_a_1x1_case_is_a_matrix_product():
    for name in ("x3-dgrad-264to136-plain", "f32-fwd-264to136"):
        case, d = R.BY_NAME[name], R.inputs(name)
        outs, _ = R.expected(name)
        for i, x in enumerate(d["x"]):
            W = d["w"].reshape(case.C, case.K).t() if case.form == "fwd" else d["w"].reshape(case.K, case.C)
            y = x.reshape(-1, case.K).double() @ W.double()
            if case.form == "fwd":
                y = (y * d["scale"].double() + d["shift"].double() + d["res"][i].reshape(-1, case.C).double()).clamp_min(0.0)
            assert torch.equal(outs[i].reshape(-1, case.C).double(), y)


def _name(i):
    t = lambda b: "true" if b else "false"
    return f"<{i.BM}, {i.BN}, {i.WM}, {i.WN}, {i.BKT}, {i.MINW}, " + ", ".join(t(b) for b in i[6:]) + ">"


def test_the_cases_reach_every_instantiation_the_defaults_choose():
    got = {}
    for case in R.CASES:
        for gl in R.glds_values(case):
            got.setdefault(R.instantiation(R.desc(case), gl, R.CUS, R.reserve_of(case)), []).append(case.name)
    f32 = lambda bn, bkt, minw, st=False: R.Inst(128, bn, 2, 2, bkt, minw, False, st, False, False, False, False, False, False)
    want = {f32(128, 32, 2), f32(128, 16, 3), f32(128, 16, 4), f32(64, 32, 2), f32(128, 32, 2, True)}
    want |= {R.Inst(128, bn, 2, 2, 32, 2, True, st, ab, ob, False, False, False, False)
             for bn, st in ((128, False), (64, False), (128, True)) for ab in (False, True) for ob in (False, True)}
    want |= {R.Inst(128, bn, 4, 1, 32, 2, False, st, False, False, True, res, msk, gl)
             for bn, st in ((128, False), (64, False), (128, True)) for res in (False, True) for msk in (False, True) for gl in (False, True)}
    assert len(want) == 5 + 12 + 24
    assert set(got) == want, sorted(_name(i) for i in set(got) ^ want)
    assert got[f32(128, 16, 3)] == ["f32-fwd-40to840-few-cus"] and got[f32(128, 16, 4)] == ["f32-fwd-40to1100-few-cus"]
    # Cout % 4 != 0 goes to the fp32 kernel in every mode that has fp32 maps: its scalar-store tail on both tile widths
    assert "f32-fwd-264to70-scalar-tail" in got[f32(128, 32, 2)] and "f32-fwd-264to2-scalar-tail" in got[f32(64, 32, 2)]


def test_the_cases_reach_every_work_decomposition_path():
    got = {}
    for case in R.CASES:
        for p in R.paths(case):
            got.setdefault(p, []).append(case.name)
    assert set(got) == {"tile-parallel", "tiny", "stream-k", "pair", "three-or-more", "slots-0-and-1", "several-tiles-per-workgroup"}
    pl = lambda name: R.plan(R.desc(R.BY_NAME[name]), R.instantiation(R.desc(R.BY_NAME[name]), 1, R.CUS, R.reserve_of(R.BY_NAME[name])),
                             R.CUS, R.reserve_of(R.BY_NAME[name]))
    p = pl("x3-fwd-520to128-streamk-pair")
    assert (p.tiles, p.nkt, p.G) == (3, 17, 6) and R.paths(R.BY_NAME["x3-fwd-520to128-streamk-pair"]) == {"tiny", "pair"}
    assert all(R.contributors(p, t)[1] - R.contributors(p, t)[0] == 1 for t in range(3))      # exactly two contributors per tile
    p = pl("x3-fwd-3x3s2-72to136")
    assert (p.tiles, p.nkt, p.G) == (6, 27, 20) and {"three-or-more", "slots-0-and-1"} <= R.paths(R.BY_NAME["x3-fwd-3x3s2-72to136"])
    p = pl("x3-fwd-520to768-few-cus")
    assert (p.tiles, p.nkt, p.G) == (18, 17, 16) and "several-tiles-per-workgroup" in R.paths(R.BY_NAME["x3-fwd-520to768-few-cus"])
    assert got["stream-k"] == ["x3-fwd-520to768-few-cus"]
    assert R.paths(R.BY_NAME["f32-fwd-3x3s2-72to136"]) >= {"tiny", "three-or-more"}
    # every unit of every plan belongs to exactly one workgroup, and the XCD order is a permutation of the positions
    for case in R.CASES:
        d = R.desc(case)
        p = R.plan(d, R.instantiation(d, 1, R.CUS, R.reserve_of(case)), R.CUS, R.reserve_of(case))
        assert p.ranges[0][0] == 0 and p.ranges[-1][1] == p.tiles * p.nkt and all(a[1] == b[0] for a, b in zip(p.ranges, p.ranges[1:]))
        assert sorted(R.xcd_contiguous(b, p.G) for b in range(p.G)) == list(range(p.G))


def test_the_cases_reach_the_tile_k_axis_and_epilogue_paths():
    rows = [R.N * h * w for h, w in R.SIZES]
    assert rows == [154, 48] and rows[0] % 128 and len(rows) == 2                      # a ragged last M-tile of the first segment; a second segment
    by = lambda f: [c for c in R.CASES if f(c)]
    x3 = by(lambda c: c.mode == "f32x3")
    assert by(lambda c: c.C % 128 and c.C > 128)                                       # a ragged N-tile
    assert {c.C for c in by(lambda c: c.C % 4)} == {70, 2} and all(c.mode == "f32" for c in by(lambda c: c.C % 4))
    assert by(lambda c: c.K % 32) and [c for c in x3 if c.K % 8 == 4]                  # partial last K-slice; a weight chunk that straddles Cin
    assert [c for c in x3 if c.k == 3 and c.stride == 2 and c.form == "fwd"]           # padding taps, stride 2
    for mode in ("f32", "f32x3", "bf16"):
        assert by(lambda c: c.mode == mode and c.form == "dgrad_s2")                   # merged stride-2 input gradient, per-segment tap sets
    assert R.desc(R.BY_NAME["x3-dgrad-s2-136to72-plain"]).seg_taps == (4, 2, 2, 1)
    assert by(lambda c: "a" in c.epi) and by(lambda c: "A" in c.epi)                   # per-segment alpha; accumulate
    assert [c for c in x3 if "P" in c.epi] and R.desc(R.BY_NAME["x3-fwd-520to128-streamk-pair"]).res == (True, False)
    assert by(lambda c: "c" in c.epi) and by(lambda c: "C" in c.epi)                   # column sums: one row, replicated rows


@pytest.mark.parametrize("reserve,usable", [(0, 256), (248, 8), (250, 8), (100, 156)])
def test_usable_cus_follows_the_library(reserve, usable):
    assert R.usable_cus(256, reserve) == usable
