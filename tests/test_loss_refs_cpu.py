"""CPU: the references of tests/loss_refs.py are right and its rule bites (no GPU, no erd_amd).

  * the composition in float32 reproduces what the REAL reference produced for fixtures F6 (f6_head.npz: the whole head loss and
    its gradients) and F1 (f1_leaf.npz: KD-KL and L2) at the tolerances tests/test_gpu_losses.py holds the kernels to, and equals
    the oracle's whole functions (O.loss_by_feat_single, O.distill_loss_single) where those take the targets
  * every table contains the edges it claims, branch by branch
  * the restatement of the kernels passes the rule; each of the 14 planted mistakes breaks it on at least one case
  * the decision cases do not depend on an order among equals: the oracle gives the same answer on permuted candidates"""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import golden_inputs as G
import leaf_refs as R
import loss_refs as LR
from oracle import erd_oracle as O

F32, F64 = LR.F32, LR.F64


def _by_name(name):
    i = [c.name for c in LR.cases()].index(name)
    return i, LR.cases()[i]


# ---- the tie to the real reference ------------------------------------------------------------------------------------------
def _f6_case():
    """F6's inputs with the oracle's decisions (ATSS targets, ERS lists, NMS keep) as the given targets"""
    sizes, t_cls, t_bbox, s_cls, s_bbox, gtb, gtl, metas = G.f6_inputs()
    N, c_old, c_all = 2, 40, 80
    tc, tb = O.flatten_levels(t_cls).contiguous(), O.flatten_levels(t_bbox).contiguous()
    sc, sb = O.flatten_levels(s_cls).contiguous(), O.flatten_levels(s_bbox).contiguous()
    anchors = torch.cat(O.grid_anchors(sizes), 0)
    A = anchors.shape[0]
    nl = [h * w for h, w in sizes]
    c = NS(name="f6", sizes=sizes, strides=list(O.STRIDES), nlvl=5, N=N, A=A, c_old=c_old, c_all=c_all, cls=sc, bbox=sb, anchors=anchors,
           distill=True, T=10.0, weights=LR.DEFAULT_W, cls_shift=0, c_t=c_old, t_cls=tc, t_bbox=tb, up=None,
           labels=torch.zeros(N, A, dtype=torch.int64), lw=torch.zeros(N, A), bt=torch.zeros(N, A, 4), num_pos=torch.zeros(N, dtype=torch.int32),
           idx_cls=torch.zeros(N, A, dtype=torch.int64), counts=torch.zeros(N, 2, dtype=torch.int32), keep=torch.zeros(N, A, dtype=torch.uint8))
    dec_all = [O.distance2bbox(O.anchor_centers(anchors), O.integral(tb[n])) for n in range(N)]
    for n in range(N):
        flags = torch.cat(O.valid_flags(sizes, metas[n]["pad_shape"]), 0)
        c.labels[n], c.lw[n], c.bt[n], p = O.get_targets_single(anchors, flags, nl, gtb[n], gtl[n], c_all)
        c.num_pos[n] = p
        ic, ib, _, _ = O.ers_select_single(tc[n], tb[n])
        c.idx_cls[n, :len(ic)] = ic
        conf, ids = tc[n].sigmoid().max(dim=-1)
        keep = O.nms_class_offset(dec_all[n][ib], conf[ib], ids[ib], 0.005)
        c.keep[n, ib[keep]] = 1
        c.counts[n] = torch.tensor([len(ic), len(ib)], dtype=torch.int32)
    return c


def test_composition_in_float32_reproduces_fixture_f6(golden):
    g = golden("f6_head.npz")
    c = _f6_case()
    y = LR.compose(c, F32)
    L = y.losses.numpy()
    for j, k in enumerate(["loss_cls", "loss_bbox", "loss_dfl"]):
        assert np.allclose(L[5 * j:5 * j + 5], g[k], rtol=1e-4, atol=1e-7), (k, L[5 * j:5 * j + 5], g[k])
    assert np.allclose(L[15:17], g["loss_dist_cls"], rtol=1e-4) and np.allclose(L[17:], g["loss_dist_bbox"], rtol=1e-4)
    off = 0
    for l, (h, w) in enumerate(c.sizes):
        gc = torch.from_numpy(g[f"g_cls{l}"]).permute(0, 2, 3, 1).reshape(2, h * w, 80)
        gb = torch.from_numpy(g[f"g_bbox{l}"]).permute(0, 2, 3, 1).reshape(2, h * w, 68)
        assert float((y.dcls[:, off:off + h * w] - gc).abs().max()) <= 1e-4 * float(gc.abs().max()) + 1e-9, l
        assert float((y.dbbox[:, off:off + h * w] - gb).abs().max()) <= 1e-4 * float(gb.abs().max()) + 1e-9, l
        off += h * w
    # and the restatement of the kernels, on the same inputs, under the same tolerances
    r = LR.restate(c)
    assert np.allclose(r.losses.numpy(), L, rtol=1e-4, atol=1e-7)


def test_composition_in_float32_reproduces_fixture_f1(golden):
    """the KD-KL and L2 sums on F1's inputs, as tests/test_gpu_losses.py::test_leaf_values_vs_reference_fixture takes them"""
    g = golden("f1_leaf.npz")
    d = G.f1_inputs()
    n = d["kd_pred"].shape[0] // 4
    w = d["kd_weight"].reshape(n, 4)[:, 0].clamp(1e-3, 1 - 1e-3)
    cls = torch.full((1, n, 8), -30.0)
    cls[0, :, 2] = torch.log(w / (1 - w))
    c = LR.make_case("f1", [(1, n)], [8], 1, 4, 8, 1, K=[n], keep="all")
    c.cls, c.bbox, c.t_bbox, c.t_cls = cls, d["kd_pred"].reshape(1, n, 68), d["kd_soft"].reshape(1, n, 68), cls[:, :, :4] + 0.5
    y = LR.compose(c, F32)
    ref = (O.kd_kl_div(d["kd_pred"], d["kd_soft"], 10.0) * torch.sigmoid(cls[0, :, 2])[:, None].expand(-1, 4).reshape(-1)).sum()
    assert float(y.kds[0]) == pytest.approx(float(ref), rel=1e-5)
    m = d["l2_a"].shape[0]
    c2 = LR.make_case("f1_l2", [(1, m)], [8], 1, 40, 41, 2, K=[m], keep="none")
    c2.cls = torch.cat([d["l2_a"], torch.zeros(m, 1)], 1)[None]
    c2.t_cls = d["l2_b"][None]
    c2.idx_cls = torch.arange(m)[None]
    y2 = LR.compose(c2, F32)
    assert float(y2.l2s[0]) / d["l2_a"].numel() == pytest.approx(float(g["l2"]), rel=1e-5)
    assert float(y2.losses[3]) == pytest.approx(float(g["l2"]), rel=1e-5)


def test_composition_equals_the_oracles_whole_functions():
    """with the default loss weights and `up` = 1 the composed losses are O.loss_by_feat_single's and O.distill_loss_single's (fp64)"""
    for name in ("pyr5_c0_1", "pyr3", "one_pos"):
        i, c = _by_name(name)
        assert c.weights == LR.DEFAULT_W
        r = LR.ref64(i)
        off = LR.lvl_off(c.sizes)
        a2 = max(r.avg[1], 1.0)
        for l in range(c.nlvl):
            sl = slice(off[l], off[l + 1])
            a = c.anchors.double()[sl][None].expand(c.N, -1, -1).reshape(-1, 4)
            lc, lb, ld, ws = O.loss_by_feat_single(a, c.cls.double()[:, sl].reshape(-1, c.c_all), c.bbox.double()[:, sl].reshape(-1, 68),
                                                   c.labels[:, sl].reshape(-1), c.lw.double()[:, sl].reshape(-1),
                                                   c.bt.double()[:, sl].reshape(-1, 4), c.strides[l], c.c_old, c.c_all, r.avg[0])
            want = torch.stack([lc, lb / a2, ld / a2]).double()
            got = r.losses[[l, c.nlvl + l, 2 * c.nlvl + l]]
            assert torch.allclose(got, want, rtol=1e-12, atol=1e-300), (name, l, got, want)
            assert float(ws) == pytest.approx(float(r.sums[l, 3]), rel=1e-12)
    i, c = _by_name("pyr3")                     # distillation of image 1 (K = 17) with the kept anchors as the only NMS candidates
    r = LR.ref64(i)
    n = 1
    kept = c.keep[n].nonzero().squeeze(1)
    far = torch.cat([O.grid_anchors([(1, len(kept))], [1024])[0]])          # centres 1024 apart: the NMS keeps every candidate
    s_old = c.cls.double()[n, :, :c.c_old]
    dc, db, k = O.distill_loss_single(far, s_old[kept], c.bbox.double()[n][kept], torch.arange(len(kept)), torch.arange(len(kept)),
                                      c.t_cls.double()[n][kept], c.t_bbox.double()[n][kept], c.weights[4], c.T, c.weights[3])
    assert len(k) == len(kept)
    assert float(db) == pytest.approx(float(r.losses[3 * c.nlvl + c.N + n]), rel=1e-12)
    idx = c.idx_cls[n, :int(c.counts[n, 0])]
    assert float((s_old[idx] - c.t_cls.double()[n][idx]).pow(2).mean()) * c.weights[4] == pytest.approx(float(r.losses[3 * c.nlvl + n]), rel=1e-12)


# ---- the tables contain what they claim ------------------------------------------------------------------------------------------
def test_geometry_and_channel_tables():
    cs = LR.cases()
    names = [c.name for c in cs]
    assert {(c.A, c.N) for c in cs if c.name.startswith("A")} == {(A, N) for A in (1, 63, 64, 65, 130) for N in (1, 3)}
    assert {(c.c_old, c.c_all) for c in cs} >= set(LR.CHANNELS)
    assert {c.nlvl for c in cs} >= {1, 3, 5}
    assert any(c.c_all - c.c_old < 4 for c in cs) and any((c.c_all - c.c_old) % 4 for c in cs if c.c_all - c.c_old > 4)
    _, p5 = _by_name("pyr5")
    assert p5.A == 53 < LR.GL_ROWS and len(set(p5.strides)) == 5 and all(s & (s - 1) == 0 for s in p5.strides)      # one block, five levels
    coef = LR.restate(p5).coef
    assert len({float(v) for v in coef[[0, 4, 8, 12, 16]]}) == 5 and len({float(v) for v in coef[[1, 5, 9, 13, 17]]}) == 5
    for c in cs:                                     # positives on the first and last row of a ragged block and of every level
        if c.name.startswith("A") or c.name.startswith("pyr5"):
            off = LR.lvl_off(c.sizes)
            n = 0 if c.N == 1 or c.name.startswith("pyr") else 2
            pos = set((c.labels[n] != c.c_all).nonzero().squeeze(1).tolist())
            assert {0, c.A - 1} <= pos and all({off[l], off[l + 1] - 1} <= pos for l in range(c.nlvl)), c.name
    assert any(c.N == 3 and int(c.num_pos[1]) == 0 and int(c.num_pos[0]) > 0 for c in cs)           # an image without positives
    _, nb = _by_name("nopos_batch")
    assert int(nb.num_pos.sum()) == 0 and float(LR.restate(nb).avg[1]) == 0.0 and float(LR.restate(nb).avg[0]) == 2.0
    _, op = _by_name("one_pos")
    assert int(op.num_pos.sum()) == 1 and 0.0 < float(LR.restate(op).avg[1]) < 1.0                  # avg[1] is clamped to 1
    assert any(bool(((c.lw == 0) & (c.labels == c.c_all)).any()) and bool(((c.lw == 1) & (c.labels == c.c_all)).any()) for c in cs)
    _, sh = _by_name("shifted")
    assert sh.cls_shift == 1 and sh.c_all % 4 == 0
    assert {tuple(c.up.tolist()) if c.up is not None else None for c in cs} >= {None}
    assert any(c.up is not None and bool((c.up == 0).any()) and bool((c.up < 0).any()) and len(set(c.up.tolist())) == len(c.up) for c in cs)
    assert any(c.weights != LR.DEFAULT_W for c in cs)
    _, orl = _by_name("one_row_per_level")
    lv = LR.level_of(orl.sizes)
    assert all(int(((orl.lw[0] != 0) & (lv == l)).sum()) == 1 for l in range(3))
    assert "family" in names


def test_dfl_and_saturation_edges_are_reached():
    raw_neg = raw_hi = integer = last_bin = False
    for c in LR.cases():
        p = LR.restate(c).probe
        m = p.is_pos[..., None].expand_as(p.raw)
        raw, y, tl, wr = p.raw[m], p.y[m], p.tl[m], p.wr[m]
        raw_neg |= bool(((raw < 0) & (y == 0)).any())
        raw_hi |= bool(((raw >= 15.9) & (tl == 15) & (y == torch.tensor(16.0) - torch.tensor(0.1))).any())        # the kernel reads z[16]
        integer |= bool(((wr == 0) & (y > 0)).any())
        last_bin |= bool(((tl == 15) & (raw < 15.9)).any())
    assert raw_neg and raw_hi and integer and last_bin
    for name in ("sat", "sat_c70_80"):
        _, c = _by_name(name)
        new = c.cls[:, :, c.c_old:]
        assert {0.0, 30.0, -30.0, 90.0, -90.0} <= set(c.cls.unique().tolist()) and bool((new.abs() == 90).any())
        d = LR.restate(c).probe.d
        assert bool((d == 0).any()) and bool((d == 16).any())                       # one-hot rows: an expectation of exactly 0 and 16
        lab = c.labels
        pos = lab != c.c_all                                                         # a saturated logit on a label's class
        x_lab = c.cls[:, :, c.c_old:].gather(2, lab.clamp(max=c.c_all - c.c_old - 1)[..., None])[..., 0][pos]
        assert bool((x_lab.abs() >= 30).any())


def test_family_case_reaches_every_giou_branch():
    i, c = _by_name("family")
    p = LR.restate(c).probe
    pred, tg = p.pred[0], p.tg[0]
    assert bool(p.is_pos.all())
    y32 = LR.compose(c, F32)
    eps = 1e-6
    for a, (fp, ft, what) in enumerate(c.family):
        assert torch.equal(pred[a], torch.tensor(fp) / 5.0) and torch.equal(tg[a], torch.tensor(ft) / 5.0), what     # exact in fp32
        r64 = LR.ref64(i).lv[0]
        assert torch.equal(r64.dec[a], torch.tensor(fp, dtype=F64) / 5.0), what                                  # and in fp64
        assert torch.equal(y32.lv[0].dec[a], pred[a]), what                                                      # and in the yardstick
        ties = [bool(pred[a, q] == tg[a, q]) for q in range(4)]
        if "shared edge: tie on" in what:
            assert ties[["x1", "y1", "x2", "y2"].index(what.split("tie on ")[1])], what
        if what.startswith("identical"):
            assert all(ties)
        area1 = (pred[a, 2] - pred[a, 0]) * (pred[a, 3] - pred[a, 1])
        area2 = (tg[a, 2] - tg[a, 0]) * (tg[a, 3] - tg[a, 1])
        w = (torch.minimum(pred[a, 2], tg[a, 2]) - torch.maximum(pred[a, 0], tg[a, 0]))
        h = (torch.minimum(pred[a, 3], tg[a, 3]) - torch.maximum(pred[a, 1], tg[a, 1]))
        uni0 = area1 + area2 - w.clamp(min=0) * h.clamp(min=0)
        ea0 = (torch.maximum(pred[a, 2], tg[a, 2]) - torch.minimum(pred[a, 0], tg[a, 0])) * (torch.maximum(pred[a, 3], tg[a, 3]) - torch.minimum(pred[a, 1], tg[a, 1]))
        if "union < eps" in what:
            assert float(uni0) < eps and float(ea0) < eps, what                     # both eps clamps
        if what.startswith("touching in x"):
            assert float(w) == 0 and float(h) > 0
        if what.startswith("disjoint"):
            assert float(w) < 0 or float(h) < 0
    whats = " | ".join(w for _, _, w in c.family)
    for need in ("identical", "tie on x1", "tie on y1", "tie on x2", "tie on y2", "touching in x", "touching in y", "disjoint", "contained",
                 "contains", "union < eps", "zero-area point inside", "zero-width line", "plain overlap"):
        assert need in whats, need


def test_distillation_edges_are_reached():
    cs = LR.cases()
    d = [c for c in cs if c.distill]
    assert {c.c_old for c in d} >= {1, 3, 40, 70} and {c.T for c in d} >= {1.0, 10.0}
    assert any(c.c_all == 80 and c.c_t == 40 for c in d)                                   # c_s != c_t
    Ks = {(int(k), c.A) for c in d for k in c.counts[:, 0]}
    assert any(k == 0 for k, _ in Ks) and any(k == 1 for k, _ in Ks) and any(k == A for k, A in Ks)
    assert any(len(set(c.counts[:, 0].tolist())) > 1 for c in d)                           # two images with different K
    _, big = _by_name("l2_two_passes")
    assert int(big.counts[0, 0]) * big.c_old > 64 * 256                                    # the grid-stride loop takes a second pass
    assert any(not bool(c.keep.any()) for c in d) and any(bool(c.keep.all()) for c in d)
    for T in (10, 1):
        _, c = _by_name(f"kd_edge_T{T}")
        assert c.A % 64 and c.keep[0].nonzero().squeeze(1).tolist() == [c.A - 1] and not torch.equal(c.keep[0], c.keep[1])
        assert torch.equal(c.t_bbox[1, 2], c.bbox[1, 2]) and int(c.keep[1, 2]) == 1          # student == teacher on a kept row
    zt = c.t_bbox.reshape(2, c.A, 4, 17)                                                   # (T = 1)
    gap = zt.max(3)[0] - zt.min(3)[0]
    kept_gap = gap[c.keep != 0]
    assert float(kept_gap.max()) > 104
    t = torch.softmax(zt, 3)[c.keep != 0]
    assert bool((t == 0).any())                                                            # the `t > 0` branch
    _, c = _by_name("pyr3")                                                                # kc == 0 under a non-zero upstream
    assert int(c.counts[0, 0]) == 0 and float(c.up[3 * c.nlvl + 0]) != 0
    fc = LR.finalize_cases()
    assert {f.nlvl for f in fc} == {1, 3, 5} and {f.N for f in fc} == {0, 1, 3}
    assert any(f.N and int(f.counts[f.N - 1, 0]) == 0 and float(f.up[3 * f.nlvl + f.N - 1]) != 0 for f in fc)
    assert any(float(f.sums[:, 3].sum()) < 1 for f in fc) and any(set(f.num_pos.tolist()) == {0, 1, 2} for f in fc)


# ---- the rule bites ---------------------------------------------------------------------------------------------------------
def test_the_restatement_passes_the_rule():
    E = LR.e32()
    print("\n[loss] E32", {k: f"{v:.3e}" for k, v in E.items()})
    for i, c in enumerate(LR.cases()):
        assert LR.violations(c, i, LR.restate(c)) == [], c.name


def test_restated_finalize_is_the_f64_formula():
    """finalize_restate against the reference's normalisations in fp64: a few roundings of fp32"""
    for f in LR.finalize_cases():
        avg = LR.avg_restate(f.num_pos[:f.N] if f.N else f.num_pos[:0], f.sums)
        losses, coef = LR.finalize_restate(f.sums, avg, f.l2s, f.kds, f.counts, f.nlvl, f.N, f.c_old, f.weights, f.up)
        a1, a2 = float(avg[0]), max(float(avg[1]), 1.0)
        lw_cls, lw_bbox, lw_dfl, lw_ld, w = f.weights
        e = LR.EPS32
        want = [lw_cls * float(f.sums[l, 0]) / (a1 + e) for l in range(f.nlvl)] + [lw_bbox * float(f.sums[l, 1]) / (1 + e) / a2 for l in range(f.nlvl)] \
            + [lw_dfl * float(f.sums[l, 2]) / (4 + e) / a2 for l in range(f.nlvl)] \
            + [w * float(f.l2s[n]) / (int(f.counts[n, 0]) * f.c_old) if int(f.counts[n, 0]) else 0.0 for n in range(f.N)] \
            + [w * lw_ld * float(f.kds[n]) / (4 + e) for n in range(f.N)]
        assert torch.allclose(losses.double(), torch.tensor(want, dtype=F64), rtol=8 * e, atol=0), f.name
        assert not torch.isnan(coef).any() and bool((coef[3::4][:f.nlvl] == 0).all())


@pytest.mark.parametrize("mut", LR.MUTATIONS)
def test_every_planted_mistake_breaks_the_rule(mut):
    E = LR.e32()
    caught = [c.name for i, c in enumerate(LR.cases()) if LR.violations(c, i, LR.restate(c, mut), E)]
    print(f"\n[loss] {mut}: caught on {caught}")
    assert caught, mut


def test_the_background_remap_is_redundant_in_the_kernels_form():
    """`bg_not_remapped` is planted as `label != cn` without the remap; with the kernel's `label < cn` leaving the remap out changes
    nothing, because c_all >= cn: no label is both"""
    for c in LR.cases():
        lab = c.labels
        cn = c.c_all - c.c_old
        mapped = torch.where(lab == c.c_all, torch.full_like(lab, cn), lab)
        assert torch.equal((lab >= 0) & (lab < cn), (mapped >= 0) & (mapped < cn))


# ---- the decision cases do not depend on an order among equals -----------------------------------------------------------------------
def test_ers_cases_keep_their_distance_from_the_threshold():
    shapes = set()
    for c in LR.ers_cases():
        N, A, C = c.cls.shape
        shapes.add((N, A, C % 4 == 0))
        for n in range(N):
            ic, ib, thr_c, thr_b = O.ers_select_single(c.cls[n], c.bbox[n])
            if c.name == "ers_constant" or A == 1:
                assert len(ic) == 0 and len(ib) == 0
                continue
            m_c, m_b = c.cls[n].sigmoid().max(-1)[0], c.bbox[n].max(-1)[0]
            assert float((m_c - thr_c).abs().min()) > 1e-4 * abs(thr_c) and float((m_b - thr_b).abs().min()) > 1e-4 * abs(thr_b), c.name
            assert (len(ic) > 0 and len(ib) > 0) or A == 2, c.name
    assert {A for _, A, _ in shapes} >= {1, 2, 257, 1025, 100} and (5, 100, True) in shapes and (5, 100, False) in shapes


def test_nms_and_atss_cases_do_not_depend_on_the_candidates_order():
    for c in LR.nms_cases():
        for n in range(2):
            K = c.K[n]
            want = LR.nms_oracle(c, n)
            for s in range(4):
                assert LR.nms_oracle(c, n, torch.randperm(K, generator=torch.Generator().manual_seed(s))) == want, (c.name, n)
    c = LR.nms_cases()
    assert [LR.nms_oracle(c[1], 0), LR.nms_oracle(c[1], 1), LR.nms_oracle(c[2], 0)] == [[1], [0, 1, 2], [0, 1]]
    assert {k for x in c for k in x.K} >= {0, 1, 2}
    for c in LR.atss_cases():
        for n in range(2):
            lab, lw, bt, npos = LR.atss_oracle(c, n)
            for s in range(4):
                l2, w2, b2, p2 = LR.atss_oracle(c, n, torch.randperm(16, generator=torch.Generator().manual_seed(s)))
                assert torch.equal(lab, l2) and torch.equal(bt, b2) and p2 == npos
        assert LR.atss_oracle(c, 0)[3] > 0 and LR.atss_oracle(c, 1)[3] == 0
        ctr = O.anchor_centers(torch.cat(O.grid_anchors(c.sizes, c.strides), 0))
        dist = (ctr - torch.tensor([4.0, 4.0])).pow(2).sum(1).sqrt().sort().values
        assert float(dist[0]) == float(dist[3]) < float(dist[4]) and float(dist[8]) < float(dist[9])      # four equidistant, none cut by top-k
