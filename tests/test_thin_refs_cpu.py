"""CPU: the references, case table and census of tests/thin_refs.py -- that the inputs make both thin kernels' arithmetic exact, that
every (pixel tile, 32-channel block) work unit has an expected block no mistake in the work decode can reproduce, that at 8 usable CUs
every case reaches the paths that run only when a workgroup owns several units, that at 256 CUs every workgroup owns one, and what the
dispatch predicates answer for every case tests/test_gpu_thin_exact.py launches."""
import pytest
import torch

import igemm_refs as R
import thin_refs as T

SERVED = [c for c in T.CASES if c.served]
REDUCED = [c for c in SERVED if c.few]
FULL = [c for c in SERVED if not c.few]


def test_every_value_and_every_sum_is_exact():
    """one bf16 limb holds every multiplicand; four times every expected value and four times every column sum is an integer below
    2^24 -- for the bf16-stored cases the column sums are those of the exact values, which the kernels sum before they round"""
    for case in T.CASES:
        d = T.inputs(case.name)
        for x in d["x"]:
            assert set(x.unique().tolist()) == {-1.0, 0.0, 1.0}
        assert set(d["w"].unique().tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0}
        for t in d["x"] + [d["w"]] + [t for key in ("res", "base", "mask") for t in d.get(key, []) if t is not None]:
            assert torch.equal(t.bfloat16().float(), t)
        if "scale" in d:
            assert set(d["scale"].tolist()) <= {0.5, 1.0, 2.0} and torch.equal(d["shift"], d["shift"].round())
        if "alpha" in d:
            assert [float(a) for a in d["alpha"]] == list(T.ALPHAS) and len(set(T.ALPHAS)) == 3 and 1.0 not in T.ALPHAS
            assert all(torch.frexp(torch.tensor(a))[0] == 0.5 for a in T.ALPHAS)          # powers of two
        assert R.acc_bound(case) * 2 * 4 + 3 * 4 + 4 < 2 ** 22                            # (|acc| * scale + |shift|) * alpha + |residual|
        outs, cs = T.expected(case.name)
        for o in outs:
            assert o.dtype == (torch.bfloat16 if case.ob else torch.float32)
            q = o.double() * 4
            assert torch.equal(q, q.round()) and float(q.abs().max()) < 2 ** 24
        assert (cs is not None) == ("c" in case.epi or "C" in case.epi)
        if cs is not None:
            assert cs.dtype == torch.float32 and torch.equal(cs, cs.round()) and float(cs.abs().max()) * 4 < 2 ** 24
            # ... and every partial sum of them: no more than |rows| values of at most this magnitude each
            rows = sum(T.desc(case).rows)
            assert rows * (R.acc_bound(case) + 4) * 4 < 2 ** 24


def test_bf16_column_sums_are_those_of_the_fp32_values():
    """the reference's convention: a bf16 launch's column sums add the exact values, not the stored ones -- they are the column sums
    of the same case on fp32 maps.  (The input gradients that carry column sums here are integers of magnitude <= 256, which bf16
    holds: the stored values add up to the same sums, so these cases pin the sums under either convention.)"""
    for case in (c for c in T.CASES if c.ob and "C" in c.epi):
        outs, cs = T.expected(case.name)
        wide, wide_cs = T.exact(case._replace(ab=False, ob=False), T.inputs(case.name))
        assert torch.equal(wide_cs, cs) and torch.equal(sum(o.double().sum((0, 1, 2)) for o in wide).float(), cs)
        assert all(float(o.abs().max()) <= 256 and torch.equal(o, o.round()) for o in wide)
        assert all(torch.equal(o.float(), wo) for o, wo in zip(outs, wide))


def test_the_reference_of_a_case_is_a_matrix_product():
    for name in ("x3-fwd-128to352-srR", "x3-dgrad-64to352-plain"):
        case, d = T.BY_NAME[name], T.inputs(name)
        outs, _ = T.expected(name)
        for i, x in enumerate(d["x"]):
            W = d["w"].reshape(case.C, case.K).t() if case.form == "fwd" else d["w"].reshape(case.K, case.C)
            y = x.reshape(-1, case.K).double() @ W.double()
            if case.form == "fwd":
                y = (y * d["scale"].double() + d["shift"].double() + d["res"][i].reshape(-1, case.C).double()).clamp_min(0.0)
            assert torch.equal(outs[i].reshape(-1, case.C).double(), y)


def test_the_geometry_is_the_smallest_that_crosses_tiles_and_segments():
    rows = [T.N * h * w for h, w in T.SIZES]
    assert rows == [270, 48, 8] and [T.cdiv(r, T.TILE) for r in rows] == [3, 1, 1]
    assert rows[0] - 2 * T.TILE == 14                                  # wave 0 partly filled, waves 1-3 empty
    for (ih, iw), (oh, ow) in zip(T.S2_IN, T.SIZES):
        assert ((ih - 1) // 2 + 1, (iw - 1) // 2 + 1) == (oh, ow)
    assert T.S2_IN[0][0] % 2 == 0                                      # a last input row no output pixel reads
    assert [T.tile_segment(rows, mt) for mt in range(5)] == [0, 0, 0, 1, 2]
    # with four tiles no range would cross a tile boundary on any of the three reduced grids
    for G, nb in ((16, 11), (24, 11), (32, 19)):
        assert all(lo // nb == (hi - 1) // nb for lo, hi in T.work_ranges(4 * nb, G))


@pytest.mark.parametrize("name", [c.name for c in SERVED])
def test_every_unit_has_a_block_nothing_else_produces(name):
    """per (pixel tile, channel block): the expected block is not all zero, differs from every other channel block on the same rows,
    and differs from what results if alpha, the residual (or the accumulate base) or the mask is left out -- a unit dropped (outputs
    start as NaN, accumulating ones from their base), computed twice into an accumulating output or stored under another block's
    index changes at least one element"""
    case = T.BY_NAME[name]
    tiles = T.unit_blocks(T.expected(name)[0])
    assert len(tiles) == 5 and all(len(t) == case.C // T.BLOCK for t in tiles)
    variants = {key: T.without(name, key) for key in ("alpha", "res", "mask")}
    assert (variants["alpha"] is not None) == ("a" in case.epi) and (variants["mask"] is not None) == ("m" in case.epi)
    assert (variants["res"] is not None) == any(f in case.epi for f in "RPA")
    variants = {k: T.unit_blocks(v) for k, v in variants.items() if v is not None}
    live = None
    if "A" in case.epi:     # a unit computed twice adds its GEMM block a second time: a non-zero product where the mask lets it through
        d = T.inputs(name)
        gemm = T.exact(case._replace(epi="", ab=False, ob=False), dict(x=d["x"], w=d["w"]))[0]
        live = T.unit_blocks([(g != 0) & (d["mask"][i] > 0 if "mask" in d else True) for i, g in enumerate(gemm)])
    for mt, blocks in enumerate(tiles):
        for cb, blk in enumerate(blocks):
            assert bool((blk != 0).any()), (mt, cb)
            for other in range(cb + 1, len(blocks)):
                assert not torch.equal(blk, blocks[other]), (mt, cb, other)
            for key, var in variants.items():
                assert not torch.equal(blk, var[mt][cb]), (mt, cb, key)
            assert live is None or bool(live[mt][cb].any()), (mt, cb)


# the counts of the issue this census answers, computed independently from the T wg / G formula: (a), (b), (c), workgroups with >= 3 units
WANT = {(16, 352): (14, 3, 1, 16), (24, 352): (21, 2, 2, 7), (32, 608): (30, 3, 2, 31)}


@pytest.mark.parametrize("name", [c.name for c in REDUCED])
def test_census_at_8_cus_reaches_every_multi_unit_path(name):
    case = T.BY_NAME[name]
    assert T.usable_cus(T.CUS, T.reserve_of(case)) == T.FEW
    c = T.census(case)
    assert (c.mtiles, c.T) == (5, 5 * case.C // 32) and c.G == T.per_cu(c.kind, T.desc(case)) * T.FEW
    assert (c.mid_starts, c.tile_crossings, c.seg_crossings, c.units3) == WANT[(c.G, case.C)]
    assert c.mid_starts >= 1 and c.tile_crossings >= 1 and c.seg_crossings >= 1          # (a), (b), (c)
    if case.K == 512:
        assert c.units2 >= 1 and c.ring_steps >= 4                                        # (d): two K-halves per unit
    else:
        assert c.units3 >= 1 and c.ring_steps >= 3                                        # (d): ring buffer 0 is refilled
    # every unit belongs to exactly one workgroup, and the XCD order is a permutation of the positions
    assert c.ranges[0][0] == 0 and c.ranges[-1][1] == c.T and all(a[1] == b[0] for a, b in zip(c.ranges, c.ranges[1:]))
    assert sorted(T.xcd_contiguous(b, c.G) for b in range(c.G)) == list(range(c.G))


def test_the_reduced_grids_are_the_three_the_shapes_were_chosen_for():
    grids = {}
    for case in REDUCED:
        c = T.census(case)
        grids.setdefault((c.G, case.C), set()).add((c.kind, case.K, c.inst.split("<")[1]))
    assert set(grids) == set(WANT)
    assert {(k, K) for k, K, _ in grids[(16, 352)]} == {("x3", 128), ("bf16", 512), ("bf16", 256)}
    assert {(k, K) for k, K, _ in grids[(24, 352)]} == {("x3", 64), ("bf16", 256)}
    assert {(k, K) for k, K, _ in grids[(32, 608)]} == {("bf16", 64), ("bf16", 128)}
    # K = 256 on bf16 maps: 16 workgroups only with residual AND mask rows
    assert T.census(T.BY_NAME["bf16-dgrad-256to352-AmC"]).G == 16 and T.census(T.BY_NAME["bf16-dgrad-256to352-plain"]).G == 24
    assert T.census(T.BY_NAME["bf16-fwd-256to352-srR"]).G == 24
    # all four (residual, mask) instantiations of the three-limb kernel at both K, of the bf16 kernel at K = 256
    x3 = {c.name: T.census(c).inst for c in REDUCED if c.mode == "f32x3"}
    assert set(x3.values()) == {f"conv_thin_x3_kernel<{ks}, 1, {r}, {m}>" for ks in (4, 8) for r in ("false", "true") for m in ("false", "true")}
    bf = {T.census(c).inst for c in REDUCED if c.mode == "bf16"}
    assert bf >= {f"conv_thin_bf16_kernel<{ks}, {rm}>" for ks in (4, 8, 16, 32) for rm in ("false, false", "true, false", "true, true")}


@pytest.mark.parametrize("name", [c.name for c in REDUCED if "c" in c.epi or "C" in c.epi])
def test_a_pending_column_sum_is_carried_across_a_tile_boundary(name):
    """the column sums of a block wait in LDS for the next block's barrier: a workgroup whose range spans a tile boundary carries them
    past the next tile's row table and activation loads, and every workgroup's last block leaves them to the final flush"""
    c = T.census(T.BY_NAME[name])
    carried = [(lo, hi) for lo, hi in c.ranges if lo // c.nb != (hi - 1) // c.nb]
    assert len(carried) == c.tile_crossings >= 2
    assert any(T.tile_segment(T.desc(T.BY_NAME[name]).rows, lo // c.nb) != T.tile_segment(T.desc(T.BY_NAME[name]).rows, (hi - 1) // c.nb)
               for lo, hi in carried)


def test_the_column_sum_cases_by_name():
    names = {c.name for c in REDUCED if "c" in c.epi or "C" in c.epi}
    assert names == ({f"x3-dgrad-{K}to352-{e}" for K in (64, 128) for e in ("mc", "AmC")} |
                     {f"bf16-dgrad-{K}to{T.BF_C[K]}-AmC" for K in (64, 128, 256, 512)} |
                     {"x3-dgrad-128to352-views", "bf16-dgrad-256to352-views"})


@pytest.mark.parametrize("name", [c.name for c in FULL])
def test_census_at_256_cus_is_one_unit_per_workgroup(name):
    case = T.BY_NAME[name]
    c = T.census(case)
    assert T.reserve_of(case) == 0 and c.G == c.T and all(hi - lo == 1 for lo, hi in c.ranges)
    assert c.G % 8 != 0                                                # the remainder branch of xcd_contiguous
    assert sorted(T.xcd_contiguous(b, c.G) for b in range(c.G)) == list(range(c.G))


def test_the_full_chip_cases_cover_both_kernels_and_both_forms():
    assert {(c.mode, c.form) for c in FULL} == {("f32x3", "fwd"), ("f32x3", "dgrad"), ("bf16", "fwd"), ("bf16", "dgrad")}


def test_the_predicates_answer_for_every_case():
    for case in T.CASES:
        kind = T.thin_kind(T.desc(case))
        assert (kind is not None) == case.served, case.name
        if case.served:
            assert kind == ("x3" if case.mode == "f32x3" else "bf16"), case.name
    refused = {c.name: c for c in T.CASES if not c.served}
    assert len(refused) == 6
    # each is refused for ONE reason: mending that field alone makes the launch a thin one
    mend = {"refused-K96": dict(K=128), "refused-C136": dict(C=352), "refused-3x3": dict(k=1), "refused-residual-on-one-segment": dict(epi="srR"),
            "refused-fp32-mode": dict(mode="f32x3"), "refused-bf16-mode-fp32-maps": dict(ab=True, ob=True)}
    assert set(mend) == set(refused)
    for name, fix in mend.items():
        assert T.thin_kind(T.desc(refused[name]._replace(**fix))) is not None, name
    assert T.desc(refused["refused-residual-on-one-segment"]).res == (True, False, False)


def test_the_cases_the_gpu_test_must_hold():
    by = lambda f: [c for c in SERVED if f(c)]
    for K in (64, 128):
        x3 = by(lambda c: c.mode == "f32x3" and c.K == K and c.few and not c.views)
        assert {(c.form, c.epi, c.stride, c.alias) for c in x3} == (
            {("fwd", "", 1, False), ("fwd", "srR", 1, False), ("fwd", "sa", 1, False), ("fwd", "sr", 2, False), ("fwd", "R", 1, True)} |
            {("dgrad", e, 1, False) for e in ("", "A", "m", "Am", "mc", "AmC")})
    for K in (64, 128, 256, 512):
        bf = by(lambda c: c.mode == "bf16" and c.K == K and c.few and not c.views)
        assert all(c.ab and c.ob for c in bf)
        assert {(c.form, c.epi) for c in bf if c.stride == 1} == {("fwd", "srR"), ("dgrad", ""), ("dgrad", "AmC")}
    assert len(by(lambda c: c.mode == "bf16" and c.stride == 2)) == 1
    assert sorted(c.mode for c in by(lambda c: c.views)) == ["bf16", "f32x3"]
    for c in by(lambda c: c.views):       # inputs, outputs, residual and mask on views whose image stride is not h w C
        assert "R" in c.epi and "m" in c.epi and c.form == "dgrad"
        d = T.desc(c)
        assert all(e != r * c.K for e, r in zip(d.in_elems, d.rows)) and all(e != r * c.C for e, r in zip(d.out_elems, d.rows))
