"""CPU: the references, data and case tables of tests/prep_refs.py -- that the limb split is the exact one and that the data fills
the lower limbs, that the fp32 Winograd transform is the fp64 one to within its four roundings, that the image references hold
U[co, ci, i, j] at the flat index the layout comments of the sources give, that every reference moves at least one bit under each
mistake a layout kernel can make, and that the case tables of tests/test_gpu_prep_exact.py cover what they claim."""
import numpy as np
import pytest
import torch

import prep_refs as P
import reduce_refs as R
import wino_refs as W

F32 = torch.float32


def f32(bits):
    return torch.from_numpy(np.array(bits, dtype=np.uint32).view(np.float32).copy())


# ---------------------------------------------------------------------------------------------
# limbs
# ---------------------------------------------------------------------------------------------
def test_limbs_are_an_exact_split_with_bounded_remainders():
    x = torch.cat([P.weights24(1, 1 << 16, edges=False), P.edge_values()])
    hi, mid, lo = P.limbs_value(P.limbs_ref(x))
    assert torch.equal((hi + mid) + lo, x)
    assert torch.equal(hi.double() + mid.double() + lo.double(), x.double())
    assert bool((mid.abs() <= hi.abs() * 2.0 ** -8).all()) and bool((lo.abs() <= hi.abs() * 2.0 ** -16).all())


def test_the_data_fills_the_lower_limbs_and_the_integer_weights_do_not():
    for x in (P.weights24(2, 1 << 16, edges=False), P.split3_inputs(70001), P.transpose_inputs(P.T_CASES[-1])[0],
              P.wino_U_f32(P.wino_inputs(P.WCase(128, 80, 1), "w24"), 1)):
        _, mid, lo = P.limbs_ref(x.reshape(-1))
        fm, fl = float((mid & 0x7FFF != 0).float().mean()), float((lo & 0x7FFF != 0).float().mean())
        print("non-zero mid / lo limbs:", fm, fl)
        assert fm >= 0.9 and fl >= 0.9
    wi = P.wino_inputs(P.WCase(128, 80, 0), "int")
    assert set(wi.unique().tolist()) == {-4.0, 0.0, 4.0}
    for x in (wi, P.wino_U_f32(wi, 0)):          # the convolution tests' weights: nothing below the first limb, image included
        _, mid, lo = P.limbs_ref(x.reshape(-1))
        assert not bool((mid & 0x7FFF).any()) and not bool((lo & 0x7FFF).any())


def test_limbs_at_the_edge_values():
    """hand-written limbs: signed zeros, exact bf16 values, ties at the first and at the second limb in both to-even directions"""
    want = {
        0x00000000: (0x0000, 0x0000, 0x0000),
        0x80000000: (0x8000, 0x0000, 0x0000),       # -0 - (-0) = +0: the remainders of a negative zero are positive zeros
        0x3F800000: (0x3F80, 0x0000, 0x0000),
        0xBFC00000: (0xBFC0, 0x0000, 0x0000),
        0x3F808000: (0x3F80, 0x3B80, 0x0000),       # 1 + 2^-8 -> 1 (even), remainder +2^-8
        0x3F818000: (0x3F82, 0xBB80, 0x0000),       # 1 + 2^-7 + 2^-8 -> 1 + 2^-6 (even), remainder -2^-8
        0xBF808000: (0xBF80, 0xBB80, 0x0000),
        0xBF818000: (0xBF82, 0x3B80, 0x0000),
        0x3F802020: (0x3F80, 0x3A80, 0x3680),       # remainder 2^-10 (1 + 2^-8) -> 2^-10 (even), then +2^-18
        0x3F802060: (0x3F80, 0x3A82, 0xB680),       # remainder 2^-10 (1 + 2^-7 + 2^-8) -> 2^-10 (1 + 2^-6), then -2^-18
        0xBF802020: (0xBF80, 0xBA80, 0xB680),
        0xBF802060: (0xBF80, 0xBA82, 0x3680),
    }
    assert set(want) <= set(P.EDGE_BITS)
    got = P.limbs_ref(f32(list(want))).to(torch.int32)
    for j, (b, limbs) in enumerate(want.items()):
        assert tuple(int(v) for v in got[:, j]) == limbs, hex(b)
    # the generators plant the list: first values of every weight tensor that is long enough
    w, _ = P.transpose_inputs(P.T_CASES[-1])
    assert R.same_bits(w.reshape(-1)[:len(P.EDGE_BITS)], P.edge_values())


def test_split3_ref_is_limbs_by_plane():
    x = P.split3_inputs(257)
    s = P.split3_ref(x)
    assert s.shape == (3, 257) and s.dtype == torch.uint16
    assert torch.equal(P.limbs_value(s).double().sum(0), x.double())


# ---------------------------------------------------------------------------------------------
# the Winograd transform
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flip", [0, 1])
def test_wino_U_f32_is_the_fp64_transform_to_four_roundings(flip):
    """|U32 - U64| <= gamma_4 (|G| |g| |G|^T): two additions per stage on the longest path, the halvings exact"""
    u = 2.0 ** -24
    gamma4 = 4 * u / (1 - 4 * u)
    w = P.wino_inputs(P.WCase(70, 48, flip), "w24")
    ohwi = (w.flip(1) if flip else w).reshape(70, 3, 3, 48)
    U64 = W.wino_U(ohwi)
    A = W.G_MAT.abs()
    bound = gamma4 * torch.einsum("ij,ocjk,lk->ocil", A, ohwi.permute(0, 3, 1, 2).double().abs(), A)
    U32 = P.wino_U_f32(w, flip)
    assert U32.shape == (70, 48, 4, 4) and U32.dtype == F32
    err = (U32.double() - U64).abs()
    share = float((err / bound.clamp_min(1e-300)).max()) * gamma4 / u
    print("largest share of the bound, in u:", share)
    assert bool((err <= bound).all())
    assert share > 0.25                   # ... and the bound is not idle: the fp32 roundings are there
    wi = P.wino_inputs(P.WCase(70, 48, flip), "int")
    ohwi = (wi.flip(1) if flip else wi).reshape(70, 3, 3, 48)
    assert torch.equal(P.wino_U_f32(wi, flip).double(), W.wino_U(ohwi))


def test_wino_U_f32_operation_order_is_the_kernels():
    """one (co, ci) by hand, scalar by scalar in numpy float32, in the order the kernels write"""
    w = P.wino_inputs(P.WCase(17, 16, 1), "w24")
    U = P.wino_U_f32(w, 1)
    h = np.float32(0.5)
    for co, ci in ((0, 0), (16, 15), (5, 9)):
        g = np.array([[w[co, 8 - (3 * a + b), ci].item() for b in range(3)] for a in range(3)], dtype=np.float32)
        t = np.zeros((4, 3), dtype=np.float32)
        for b in range(3):
            t[0][b], t[3][b] = g[0][b], g[2][b]
            t[1][b] = h * np.float32(np.float32(g[0][b] + g[1][b]) + g[2][b])
            t[2][b] = h * np.float32(np.float32(g[0][b] - g[1][b]) + g[2][b])
        for i in range(4):
            u = [t[i][0], h * np.float32(np.float32(t[i][0] + t[i][1]) + t[i][2]), h * np.float32(np.float32(t[i][0] - t[i][1]) + t[i][2]),
                 t[i][2]]
            assert R.same_bits(U[co, ci, i], torch.tensor(np.array(u, dtype=np.float32)))


# ---------------------------------------------------------------------------------------------
# layouts: the flat index of the source comments, once more, as a loop
# ---------------------------------------------------------------------------------------------
def test_image_references_hold_U_at_the_flat_index_of_the_layout_comment():
    """winograd.hip: U[xi][cout/16][cin/16][kq][cout%16][4]; erd_common.h: U3[xi][limb][co / 32][ci / 16][lane = (ci % 16 / 8) * 32 +
    co % 32][ci % 8].  Every element of both images is either gathered here or a zero of the padding rows."""
    Cout, Cin, flip = 33, 32, 1
    w = P.wino_inputs(P.WCase(Cout, Cin, flip), "w24")
    U = P.wino_U_f32(w, flip)
    L = P.limbs_ref(U)
    img = P.wino_image_ref(w, flip)
    img3 = P.wino_image_x3_ref(w, flip)
    nks, cop16, cop32 = Cin // 16, 48, 64
    assert tuple(img.shape) == (16, cop16 // 16, nks, 4, 16, 4) and img.dtype == F32
    assert tuple(img3.shape) == (16, 3, cop32 // 32, nks, 64, 8) and img3.dtype == torch.uint16
    assert img.numel() == P.wino_image_elems(Cout, Cin) and img3.numel() == P.wino_image_x3_elems(Cout, Cin)
    flat, flat3 = R.bits(img).reshape(-1).tolist(), img3.reshape(-1).to(torch.int32).tolist()
    Ub, Lb = R.bits(U).tolist(), L.to(torch.int32).tolist()
    seen, seen3 = set(), set()
    per_xi, per_xl = (cop16 // 16) * nks * 256, (cop32 // 32) * nks * 512
    for co in range(Cout):
        for ci in range(Cin):
            base = (((co // 16) * nks + ci // 16) * 4 + (ci % 16) // 4) * 64 + (co % 16) * 4 + ci % 4
            base3 = (((co // 32) * nks + ci // 16) * 64 + ((ci % 16) // 8) * 32 + co % 32) * 8 + ci % 8
            for i in range(4):
                for j in range(4):
                    xi = 4 * i + j
                    o = xi * per_xi + base
                    assert flat[o] == Ub[co][ci][i][j], (co, ci, i, j)
                    seen.add(o)
                    for limb in range(3):
                        o3 = (xi * 3 + limb) * per_xl + base3
                        assert flat3[o3] == Lb[limb][co][ci][i][j], (limb, co, ci, i, j)
                        seen3.add(o3)
    assert len(seen) == 16 * Cout * Cin and len(seen3) == 48 * Cout * Cin
    assert all(flat[o] == 0 for o in range(len(flat)) if o not in seen)
    assert all(flat3[o] == 0 for o in range(len(flat3)) if o not in seen3)


@pytest.mark.parametrize("out", P.T_OUTS)
def test_transpose_reference_at_the_flat_index_of_the_kernel_comment(out):
    """conv_mfma.hip: dst[plane][ci][t'][co] = limb `plane` of rowscale[co] * w[co][t][ci]"""
    Cout, ntaps, Cin = 3, 9, 5
    w, rs = P.weights24(11, Cout, ntaps, Cin), P.rowscale24(12, Cout)
    for flip in (0, 1):
        ref = P.transpose_ref(w, rs, flip, out)
        flat = R.bits(ref).reshape(-1).to(torch.int32) & (0xFFFF if out != "f32" else -1)
        n = Cout * ntaps * Cin
        assert ref.numel() == (3 * n if out == "x3" else n)
        for co in range(Cout):
            for t in range(ntaps):
                for ci in range(Cin):
                    v = (w[co, t, ci] * rs[co]).reshape(1)
                    td = ntaps - 1 - t if flip else t
                    o = (ci * ntaps + td) * Cout + co
                    if out == "f32":
                        assert int(flat[o]) == int(R.bits(v)), (co, t, ci)
                    elif out == "bf16":
                        assert int(flat[o]) == int(P.bits16(v.bfloat16()).to(torch.int32)), (co, t, ci)
                    else:
                        assert [int(flat[p * n + o]) for p in range(3)] == P.limbs_ref(v).to(torch.int32).reshape(-1).tolist(), (co, t, ci)


def test_a_difference_is_named_by_plane_position_and_channels():
    w = P.wino_inputs(P.WCase(33, 32, 0), "w24")
    want = P.wino_image_x3_ref(w, 0)
    assert P.explain(want.clone(), want, None) is None
    got = want.clone()
    # limb 2 of U[co = 32, ci = 25] at xi = 7: cout block 1, slice 1, lane (25 % 16 / 8) * 32 + 0, element 25 % 8
    got[7, 2, 1, 1, 32, 1] ^= 1
    got[9, 0, 0, 0, 0, 0] ^= 1
    f = P.first_diff(got, want)
    assert P.where_image_x3(f, 33, 32) == dict(plane=2, position=7, co=32, ci=25)
    assert "first of 2 differing" in P.explain(got, want, lambda f: P.where_image_x3(f, 33, 32))
    img = P.wino_image_ref(w, 0)
    got = img.clone()
    got[5, 2, 1, 3, 0, 2] = 0.0               # co = 32, ci = 16 + 12 + 2
    assert P.where_image(P.first_diff(got, img), 33, 32) == dict(plane=0, position=5, co=32, ci=30)
    t = P.transpose_ref(w, None, 0, "x3")    # [3][Cin = 32][9][Cout = 33]
    got = t.clone()
    got[1, 31, 4, 20] ^= 0x8000
    assert P.where_transposed(P.first_diff(got, t), 33, 9, 32) == dict(plane=1, position=4, co=20, ci=31)
    assert P.where_planes(2 * 257 + 5, 257) == dict(plane=2, position=5, co=None, ci=None)


# ---------------------------------------------------------------------------------------------
# sensitivity: on the data of the GPU cases, each mistake moves at least one bit
# ---------------------------------------------------------------------------------------------
def differ(a, b):
    return not R.same_bits(a, b)


def test_transpose_references_move_under_each_mistake():
    for case in P.T_CASES:
        w, rs = P.transpose_inputs(case)
        n = case.Cout * case.ntaps * case.Cin
        x3 = P.transpose_ref(w, rs, case.flip, "x3")
        assert differ(x3, x3[[0, 2, 1]]), case                      # mid and lo planes swapped
        for out in P.T_OUTS:
            ref = P.transpose_ref(w, rs, case.flip, out)
            if case.flip and case.ntaps > 1:                        # t' not reversed (one tap has nothing to reverse)
                assert differ(ref, P.transpose_ref(w, rs, case.flip, out, _reverse=False)), (case, out)
            if case.rs and case.Cout > 1 and n > 1:                 # the row scale taken by ci (one row has nothing to exchange)
                assert differ(ref, P.transpose_ref(w, rs, case.flip, out, _scale_by="ci")), (case, out)
            if case.rs:                                             # the row scale left out
                assert differ(ref, P.transpose_ref(w, None, case.flip, out)), (case, out)


@pytest.mark.parametrize("data", ["w24", "int"])
def test_image_references_move_under_each_mistake(data):
    for case in P.W_CASES:
        w = P.wino_inputs(case, data)
        img, img3 = P.wino_image_ref(w, case.flip), P.wino_image_x3_ref(w, case.flip)
        if data == "w24" or case.Cout * case.Cin >= 256:            # (a 1 x 16 integer weight may be symmetric, or all zero)
            assert differ(img, P.wino_image_ref(w, 1 - case.flip)), case                        # flip ignored
            assert differ(img3, P.wino_image_x3_ref(w, 1 - case.flip)), case
        if case.Cout % 16:                                          # padding rows left non-zero
            assert differ(img, P.wino_image_ref(w, case.flip, _pad_value=1.0)), case
        if case.Cout % 32:
            assert differ(img3, P.wino_image_x3_ref(w, case.flip, _pad_value=1.0)), case
        if data == "w24":
            assert differ(img3, img3[:, [0, 2, 1]]), case                                       # mid and lo planes swapped
            assert differ(img3, P.wino_image_x3_ref(w, case.flip, _lane_major="co")), case      # lane = (co % 32) * 2 + ci % 16 / 8
        else:       # what the issue is about: on the integer weights the lower planes are zero, swapped or not
            assert not differ(img3, img3[:, [0, 2, 1]]), case


def test_split3_reference_moves_when_planes_are_swapped():
    for n in P.SPLIT3_NS:
        s = P.split3_ref(P.split3_inputs(n))
        assert differ(s, s[[0, 2, 1]]) and differ(s, s[[1, 0, 2]]), n
    s = P.split3_ref(P.edge_values())
    assert differ(s, s[[0, 2, 1]])


# ---------------------------------------------------------------------------------------------
# block counts and case tables
# ---------------------------------------------------------------------------------------------
def test_prep_blocks_by_hand():
    assert P.prep_blocks(0, 1, 1, 1) == 1 and P.prep_blocks(1, 32, 1, 32) == 1
    assert P.prep_blocks(0, 33, 1, 32) == 2 and P.prep_blocks(0, 32, 1, 33) == 2
    assert P.prep_blocks(0, 100, 49, 65) == 4 * 3 * 49 and P.prep_blocks(1, 65, 9, 100) == 3 * 4 * 9
    assert P.prep_blocks(2, 16, 9, 16) == 1 and P.prep_blocks(2, 15, 9, 16) == 1 and P.prep_blocks(2, 17, 9, 16) == 2
    assert P.prep_blocks(2, 70, 9, 48) == 15 and P.prep_blocks(2, 128, 9, 80) == 40             # 80 x 48, 128 x 80 threads
    assert P.prep_blocks(3, 16, 1, 16) == 1 and P.prep_blocks(3, 257, 1, 1) == 2 and P.prep_blocks(3, 65, 9, 100) == 229
    assert P.prep_blocks(4, 1, 9, 16) == 2 and P.prep_blocks(4, 33, 9, 48) == 12 and P.prep_blocks(4, 70, 9, 64) == 24


def test_transpose_cases_cover_every_size_with_every_tap_count_flip_and_row_scale():
    for nt in P.T_NTAPS:
        for flip in (0, 1):
            for rs in (0, 1):
                cs = [c for c in P.T_CASES if (c.ntaps, c.flip, c.rs) == (nt, flip, rs)]
                assert sorted(c.Cout for c in cs) == sorted(P.T_SIZES) and sorted(c.Cin for c in cs) == sorted(P.T_SIZES)
    assert len(set(P.T_CASES)) == len(P.T_CASES) == 96
    assert any(c.Cout % 32 and c.Cin % 32 and c.Cout > 32 and c.Cin > 32 for c in P.T_CASES)     # ragged last tile on both sides


def test_the_mixed_table_puts_every_pair_of_kinds_and_both_block_extremes_side_by_side():
    tour = P.kind_tour()
    assert len(tour) == 26 and {(a, b) for a, b in zip(tour, tour[1:])} == {(a, b) for a in P.KINDS for b in P.KINDS}
    t = P.TABLES["mixed"]
    assert len(t) == 40
    assert {(a.kind, b.kind) for a, b in zip(t, t[1:])} == {(a, b) for a in P.KINDS for b in P.KINDS}
    nb = [P.item_blocks(it) for it in t]
    assert any(a == 1 and b >= 100 for a, b in zip(nb, nb[1:])) and any(a >= 100 and b == 1 for a, b in zip(nb, nb[1:]))
    assert any(a == 1 and b == 1 for a, b in zip(nb, nb[1:]))
    assert sum(1 for b in nb if 200 <= b <= 999) >= 4 and nb.count(1) >= 8
    assert all(it.Cin % 16 == 0 and it.ntaps == 9 for it in t if it.kind in (2, 4))
    assert any(it.Cout % 16 for it in t if it.kind == 2) and any(it.Cout % 32 for it in t if it.kind == 4)
    assert any(it.flip for it in t if it.kind < 2) and any(it.rs for it in t if it.kind < 2) and any(not it.rs for it in t if it.kind < 2)
    assert P.item_blocks(P.TABLES["first-has-one-block"][0]) == 1 and P.item_blocks(P.TABLES["last-has-one-block"][-1]) == 1
    assert all(P.item_blocks(it) == 1 for it in P.TABLES["one-block-items-only"])
    assert [P.TABLES[f"alone-{k}"][0].kind for k in P.KINDS] == list(P.KINDS)
    for name, items in P.TABLES.items():
        for it, (w, rs) in zip(items, P.table_inputs(name)):
            ref = P.item_ref(it, w, rs)
            assert ref.numel() == P.item_out(it)[0] and ref.element_size() == P.item_out(it)[1], (name, it)


# ---------------------------------------------------------------------------------------------
# BN fold
# ---------------------------------------------------------------------------------------------
def test_bn_fold_reference_in_fp32_sits_inside_the_bound_of_the_fp64_one():
    for j, eps in enumerate(P.BN_EPS):
        g, b, m, v = P.bn_inputs(j)
        assert g.numel() == P.BN_NS[j] and float(v.min()) >= 0.5
        (s32, h32), (s64, h64) = P.bn_fold_ref(g, b, m, v, eps), P.bn_fold_ref(g, b, m, v, eps, double=True)
        assert s32.dtype == F32 and s64.dtype == torch.float64
        assert R.relerr(s64, g.double() / torch.sqrt(v.double() + float(np.float32(eps)))) < 1e-15      # test_bn_fold_sizes' own formula
        # a quarter of the bound is left to the roundings themselves: the rest is the kernel's for sqrtf, the division and a contraction
        assert R.relerr(s32.double(), s64) < P.BN_BOUND / 4 and R.relerr(h32.double(), h64) < P.BN_BOUND / 4
    # a different eps is visible at the bound: the items of the batched launch cannot trade theirs
    g, b, m, v = P.bn_inputs(4)
    for e0 in P.BN_EPS:
        for e1 in P.BN_EPS:
            if e0 != e1:
                assert R.relerr(P.bn_fold_ref(g, b, m, v, e0, double=True)[0], P.bn_fold_ref(g, b, m, v, e1, double=True)[0]) > P.BN_BOUND


# ---------------------------------------------------------------------------------------------
# ParamPrep refuses what the batched kernel cannot check
# ---------------------------------------------------------------------------------------------
def test_param_prep_refuses_winograd_items_the_host_entry_points_refuse():
    from erd_amd import _lib, kernels as K
    prep = K.ParamPrep("cpu")
    owner = torch.zeros(1)
    for kind, elems in ((2, P.wino_image_elems), (4, P.wino_image_x3_elems)):
        for Cout, ntaps, Cin in ((16, 9, 24), (16, 9, 8), (32, 9, 17), (16, 1, 16)):
            w = torch.zeros(Cout, ntaps, Cin)
            with pytest.raises(_lib.ErdHipError):
                prep.register(("U", kind, Cin, ntaps), kind, w, None, torch.zeros(elems(Cout, Cin + 16)), Cout, ntaps, Cin, 0, owner, 0)
    with pytest.raises(_lib.ErdHipError):
        prep.register(("T", 0, False), 5, torch.zeros(4, 1, 4), None, torch.zeros(16), 4, 1, 4, 0, owner, 0)
    assert not prep.recipes
    prep.register(("U", 0), 2, torch.zeros(17, 9, 32), None, torch.zeros(P.wino_image_elems(17, 32)), 17, 9, 32, 1, owner, 0)
    prep.register(("T", 0, False), 0, torch.zeros(17, 49, 5), None, torch.zeros(17 * 49 * 5), 17, 49, 5, 0, owner, 0)
    assert len(prep.recipes) == 2
