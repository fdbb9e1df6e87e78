"""Plain torch-CPU references, inputs, case table and a host model ("census") of the implicit-GEMM convolution conv_igemm_kernel
(erd_amd/csrc/conv_mfma.hip), for tests/test_gpu_igemm_exact.py to run and tests/test_igemm_refs_cpu.py to reason about.  No GPU and no
project kernel is touched here.

Exactness.  Activations are in {-1, 0, 1} and weights in {-2 .. 2}: every bf16 rounding and three-limb split leaves them as they are
(the mid and low limbs are zero), every product and every fp32 sum over K <= 9 * 136 terms is an integer of magnitude <= 2 K, and so
is every stream-K partial sum, whatever the partition.  The epilogue's operands keep it exact: scale in {0.5, 1, 2}, alpha in {0.5, 2},
shift / residual / accumulate base small integers, masks in {-1, 0, 1} -- results are multiples of 1/4 far below 2^24 / 4.  So every
output element has ONE right value whatever the order of the additions; a bf16-stored output is that value rounded once to bf16
(nearest even).  Column sums are sums of integers: float atomics add them exactly in any order.

Geometry.  N = 2 images, two segments whose OUTPUT maps have 7 x 11 and 4 x 6 pixels: 154 + 48 = 202 GEMM rows, the second M-tile of
the first segment ragged.  The merged stride-2 input gradient runs on one map of 13 x 21 pixels (its four parity classes are the
launch's segments).  A case names its GEMM: K contracted channels -> C output channels.

Census.  `instantiation` restates erd_conv_igemm's dispatch and `plan` the grid / stream-K plan of launch_igemm with the slab and slot
formulas of the kernel, as functions of the physical CU count and the CU reserve (defaults of every ERD_* switch)."""
from __future__ import annotations

import collections
import functools

import torch

N = 2
SIZES = ((7, 11), (4, 6))          # output pixels per segment
S2_IN = ((13, 21), (7, 11))        # 3 x 3 / stride 2 / pad 1 inputs that produce SIZES
CUS = 256                          # CUs of the device the census is asserted for
FEW = 8                            # ... and the reduced count of the cases that reserve all but eight

# epi flags: s scale + shift, r ReLU, R residual on every segment, P residual on the first segment only, a per-segment alpha,
#            A accumulate into the output, m ReLU mask, c / C column sums in one row / eight replicated rows
Case = collections.namedtuple("Case", "name mode form K C k stride epi ab ob few")


def _c(name, mode, form, K, C, epi="", k=1, stride=1, ab=False, ob=False, few=False):
    return Case(name, mode, form, K, C, k, stride, epi, ab, ob, few)


X3_EPIS = ("", "A", "m", "Am")      # (residual, mask) presence of a three-limb input gradient: none, residual, mask, both
CASES = (
    # ---- three-limb mode (each runs with ERD_IG_GLDS 0 and 1)
    [_c(f"x3-dgrad-264to136-{e or 'plain'}", "f32x3", "dgrad", 264, 136, e) for e in X3_EPIS] +           # 128 x 128; ragged N-tile; 8-channel last slice
    [_c(f"x3-dgrad-256to64-{e or 'plain'}", "f32x3", "dgrad", 256, 64, e) for e in X3_EPIS] +             # 128 x 64
    [_c(f"x3-dgrad-s2-136to72-{e or 'plain'}", "f32x3", "dgrad_s2", 136, 72, e, k=3, stride=2) for e in X3_EPIS] +      # ST: 4 + 2 + 2 + 1 taps
    [_c("x3-fwd-520to128-streamk-pair", "f32x3", "fwd", 520, 128, "srP"),              # 3 tiles x 17 slices on 6 workgroups; residual on one segment
     _c("x3-fwd-260to136-alpha", "f32x3", "fwd", 260, 136, "sa"),                      # Cin % 8 == 4: a weight chunk straddles Cin
     _c("x3-fwd-3x3s2-72to136", "f32x3", "fwd", 72, 136, "srR", k=3, stride=2),        # padding taps; 6 tiles x 27 slices on 20 workgroups
     _c("x3-fwd-520to768-few-cus", "f32x3", "fwd", 520, 768, "sr", few=True),          # 18 tiles on 16 workgroups: tiles back to back
     _c("x3-dgrad-264to136-colsum1", "f32x3", "dgrad", 264, 136, "mc"),
     _c("x3-dgrad-264to136-colsum8", "f32x3", "dgrad", 264, 136, "mC")] +
    # ---- fp32 MFMA
    [_c("f32-fwd-264to136", "f32", "fwd", 264, 136, "srR"),                            # <128, 128, 32, 2>, tile-parallel
     _c("f32-fwd-264to70-scalar-tail", "f32", "fwd", 264, 70, "sraP"),                 # Cout % 4 != 0
     _c("f32-fwd-264to2-scalar-tail", "f32", "fwd", 264, 2, "sr"),                     # ... on the 128 x 64 tiles
     _c("f32-dgrad-264to70-mask-colsum", "f32", "dgrad", 264, 70, "mc"),               # ... with the column sums' tail
     _c("f32-dgrad-256to64-colsum8", "f32", "dgrad", 256, 64, "AmC"),                  # <128, 64, 32, 2>
     _c("f32-fwd-520to128-streamk-pair", "f32", "fwd", 520, 128, "sr"),
     _c("f32-fwd-3x3s2-72to136", "f32", "fwd", 72, 136, "sa", k=3, stride=2),          # three and more contributors
     _c("f32-dgrad-s2-136to72", "f32", "dgrad_s2", 136, 72, "Am", k=3, stride=2),      # ST
     _c("f32-fwd-40to840-few-cus", "f32", "fwd", 40, 840, "sr", few=True),             # 21 tiles on 8 CUs: <128, 128, 16, 3>
     _c("f32-fwd-40to1100-few-cus", "f32", "fwd", 40, 1100, "sR", few=True)] +         # 27 tiles on 8 CUs: <128, 128, 16, 4>
    # ---- bf16 MFMA, maps stored as fp32 or bf16
    [_c(f"bf16-{n}-in{int(ab)}-out{int(ob)}", "bf16", form, K, C, e, k=k, stride=s, ab=ab, ob=ob)
     for ab in (False, True) for ob in (False, True)
     for n, form, K, C, e, k, s in (("fwd-264to136", "fwd", 264, 136, "srR", 1, 1), ("dgrad-256to64", "dgrad", 256, 64, "m", 1, 1),
                                    ("dgrad-s2-136to72", "dgrad_s2", 136, 72, "Am", 3, 2))])
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def glds_values(case):
    return (0, 1) if case.mode == "f32x3" else (1,)


# ---------------------------------------------------------------------------------------------
# inputs and the exact result
# ---------------------------------------------------------------------------------------------
def maps(case):
    """(input sizes, output sizes) per segment of the launch's tensors"""
    if case.form == "dgrad_s2":
        return (SIZES[0],), (S2_IN[0],)                 # dz 7 x 11 -> dx 13 x 21
    if case.form == "fwd" and case.stride == 2:
        return S2_IN, SIZES
    return SIZES, SIZES


ALPHAS = (0.5, 2.0)


def build_inputs(case, ins, outs, alphas=ALPHAS):
    """everything a launch of the case reads, fp32 on the CPU, from a generator seeded by the case's name: x [N, h, w, K] per segment
    in {-1, 0, 1}, the FORWARD weight w in {-2 .. 2} (fwd: [C, k, k, K]; dgrad: [K, k, k, C], the input gradient contracts over its
    output channels), and the epilogue's operands.  `ins` / `outs`: map sizes per segment (tests/thin_refs.py passes its own)"""
    g = torch.Generator().manual_seed(sum(map(ord, case.name)))
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).float()
    d = dict(x=[ri(-1, 1, N, h, w, case.K) for h, w in ins])
    d["w"] = ri(-2, 2, *((case.C, case.k, case.k, case.K) if case.form == "fwd" else (case.K, case.k, case.k, case.C)))
    oshape = [(N, h, w, case.C) for h, w in outs]
    e = case.epi
    if "s" in e:
        d["scale"] = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (case.C,), generator=g)]
        d["shift"] = ri(-3, 3, case.C)
    if "R" in e or "P" in e:
        d["res"] = [ri(-4, 4, *s) if ("R" in e or i == 0) else None for i, s in enumerate(oshape)]
    if "a" in e:
        d["alpha"] = [torch.tensor([v]) for v in alphas][:len(oshape)]
    if "A" in e:
        d["base"] = [ri(-4, 4, *s) for s in oshape]
    if "m" in e:
        d["mask"] = [ri(-1, 1, *s) for s in oshape]
    return d


@functools.lru_cache(maxsize=None)
def inputs(name):
    """build_inputs of a case of this table, on its maps"""
    case = BY_NAME[name]
    return build_inputs(case, *maps(case))


def acc_bound(case):
    """no partial sum of the GEMM can exceed this magnitude"""
    return 2 * case.k * case.k * case.K


def build_expected(case, d, outs):
    """(outputs per segment in the storage type of the case, column sums [C] or None): the one right answer for the inputs d.  The
    column sums add the exact values, BEFORE a bf16-stored output is rounded: both kernels sum their fp32 results."""
    res = []
    for i, x in enumerate(d["x"]):
        xn, p = x.permute(0, 3, 1, 2).double(), case.k // 2
        if case.form == "fwd":
            y = torch.nn.functional.conv2d(xn, d["w"].permute(0, 3, 1, 2).double(), stride=case.stride, padding=p)
        else:
            oh, ow = outs[i]
            op = (oh - ((x.shape[1] - 1) * case.stride - 2 * p + case.k), ow - ((x.shape[2] - 1) * case.stride - 2 * p + case.k))
            y = torch.nn.functional.conv_transpose2d(xn, d["w"].permute(0, 3, 1, 2).double(), stride=case.stride, padding=p, output_padding=op)
        y = y.permute(0, 2, 3, 1)
        assert tuple(y.shape[1:3]) == tuple(outs[i]) and float(y.abs().max()) <= acc_bound(case) and torch.equal(y, y.round())
        if "scale" in d:
            y = y * d["scale"].double() + d["shift"].double()
        if "alpha" in d:
            y = y * d["alpha"][i].double()
        r = d["base"][i] if "base" in d else (d["res"][i] if "res" in d else None)
        if r is not None:
            y = y + r.double()
        if "r" in case.epi:
            y = y.clamp_min(0.0)
        if "mask" in d:
            y = torch.where(d["mask"][i] > 0, y, torch.zeros_like(y))
        assert torch.equal(y * 4, (y * 4).round()) and float(y.abs().max()) * 4 < 2 ** 24
        res.append(y)
    cs = sum(y.sum((0, 1, 2)) for y in res).float() if ("c" in case.epi or "C" in case.epi) else None
    return [y.float().bfloat16() if case.ob else y.float() for y in res], cs


@functools.lru_cache(maxsize=None)
def expected(name):
    """build_expected of a case of this table"""
    case = BY_NAME[name]
    return build_expected(case, inputs(name), maps(case)[1])


# ---------------------------------------------------------------------------------------------
# the census: erd_conv_igemm's dispatch and launch_igemm's plan, restated
# ---------------------------------------------------------------------------------------------
Inst = collections.namedtuple("Inst", "BM BN WM WN BKT MINW BF ST AB OB X3 RES MSK GL")
Desc = collections.namedtuple("Desc", "rows seg_taps Cin Cout ntaps w w_x3 w_bf16 in_bf16 out_bf16 res mask sk_ws")


def cdiv(a, b):
    return -(-a // b)


def usable_cus(physical, reserve):
    return physical - reserve if physical - reserve >= 8 else min(physical, 8)


def reserve_of(case, physical=CUS):
    return physical - FEW if case.few else 0


def desc(case):
    """what kernels.conv_forward / conv_dgrad / _dgrad_s2_merged put into the launch descriptor, as far as the dispatch reads it"""
    ins, outs = maps(case)
    if case.form == "dgrad_s2":     # the parity classes (1, 1), (0, 1), (1, 0), (0, 0) of dx: segments with 4, 2, 2, 1 taps
        oh, ow = outs[0]
        rows = [N * ((oh - py + 1) // 2) * ((ow - px + 1) // 2) for py, px in ((1, 1), (0, 1), (1, 0), (0, 0))]
        seg_taps, ntaps = (4, 2, 2, 1), 4
    else:
        rows, seg_taps, ntaps = [N * h * w for h, w in outs], (0,) * len(outs), case.k * case.k
    e = case.epi
    res = [("R" in e or "A" in e or ("P" in e and i == 0)) for i in range(len(rows))]
    x3 = case.mode == "f32x3" and case.K % 4 == 0
    return Desc(tuple(rows), seg_taps, case.K, case.C, ntaps, case.mode != "bf16", x3, case.mode == "bf16", case.ab, case.ob, tuple(res),
                tuple(["m" in e] * len(rows)), case.form != "dgrad_s2")


def instantiation(d, glds=1, physical=CUS, reserve=0):
    """template arguments of the conv_igemm_kernel erd_conv_igemm launches (thin kernels disabled)"""
    st = any(d.seg_taps)
    if d.w_bf16:
        return Inst(128, 64 if (d.Cout <= 64 and not st) else 128, 2, 2, 32, 2, True, st, bool(d.in_bf16), bool(d.out_bf16), False, False, False, False)
    if d.w_x3 and d.Cin % 4 == 0 and (d.Cout % 4 == 0 or not d.w):
        return Inst(128, 64 if (d.Cout <= 64 and not st) else 128, 4, 1, 32, 2, False, st, False, False, True, any(d.res), any(d.mask), bool(glds))
    f32 = lambda bn, bkt, minw, st_=False: Inst(128, bn, 2, 2, bkt, minw, False, st_, False, False, False, False, False, False)
    if st:
        return f32(128, 32, 2, True)
    if d.Cout <= 64:
        return f32(64, 32, 2)
    tiles = sum(cdiv(r, 128) for r in d.rows) * cdiv(d.Cout, 128)
    Kdim = d.ntaps * d.Cin
    if Kdim == 256 and d.Cout >= 512:
        return f32(64, 32, 2)
    if Kdim <= 256:     # the co-residency whose last dispatch round is fullest
        cus = usable_cus(physical, reserve)
        c2, c3, c4 = (cdiv(tiles, n * cus) * (n / eff) for n, eff in ((2, 0.83), (3, 0.85), (4, 0.87)))
        if c3 < c4 and c3 <= c2:
            return f32(128, 16, 3)
        if c2 < c4 and c2 < c3:
            return f32(128, 32, 2)
        return f32(128, 16, 4)
    return f32(128, 16, 4) if tiles >= 32 * physical else f32(128, 32, 2)


def xcd_contiguous(block, grid):
    q, r, xcd, idx = grid >> 3, grid & 7, block & 7, block >> 3
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + idx


Plan = collections.namedtuple("Plan", "tiles nkt G streamk ranges")


def plan(d, inst, physical=CUS, reserve=0, min_slices=8, sk_min_k=512):
    """grid and work ranges: ranges[b] = (first unit, end unit) of the workgroup at position b of the work order (block index
    blk runs position xcd_contiguous(blk, G) unless the launch has per-segment tap sets)"""
    bk = (inst.BKT // 4) * (8 if inst.BF else 4)
    tiles = sum(cdiv(r, inst.BM) for r in d.rows) * cdiv(d.Cout, inst.BN)
    nkt = d.ntaps * cdiv(d.Cin, bk)
    slots = inst.MINW * usable_cus(physical, reserve)
    ragged = tiles < 8 * slots and tiles % slots != 0
    sk_pays = tiles * 2 <= slots if inst.BF else True
    units = tiles * nkt
    tiny = units < slots and min_slices > 0 and nkt >= 2 * min_slices and not inst.BF
    G, streamk = tiles, False
    if d.sk_ws and ragged and sk_pays and not any(d.seg_taps) and nkt * inst.BKT >= sk_min_k and (units >= slots or tiny):
        G, streamk = min(slots, max(tiles, units // min_slices)), True
    return Plan(tiles, nkt, G, streamk, tuple((units * b // G, units * (b + 1) // G) for b in range(G)))


def contributors(pl, tt):
    """positions of the workgroups that hold units of tile tt, by the kernel's formulas (first_b, last_b)"""
    U, t0 = pl.tiles * pl.nkt, tt * pl.nkt
    return ((t0 + 1) * pl.G - 1) // U, ((t0 + pl.nkt) * pl.G - 1) // U


def slot(pl, b, tt):
    """the slab slot workgroup b uses for its partial tile tt: 0 when its range starts in tt, 1 otherwise"""
    return 0 if tt == pl.ranges[b][0] // pl.nkt else 1


def paths(case, glds=1):
    """names of the work-decomposition paths a launch of the case takes at CUS compute units"""
    d = desc(case)
    inst = instantiation(d, glds, CUS, reserve_of(case))
    pl = plan(d, inst, CUS, reserve_of(case))
    out = set()
    if not pl.streamk:
        out.add("tile-parallel")
        assert pl.G == pl.tiles
        return out
    out.add("tiny" if pl.tiles * pl.nkt < inst.MINW * usable_cus(CUS, reserve_of(case)) else "stream-k")
    if pl.G < pl.tiles:
        out.add("several-tiles-per-workgroup")
    for tt in range(pl.tiles):
        f, l = contributors(pl, tt)
        holders = [b for b, (lo, hi) in enumerate(pl.ranges) if lo < (tt + 1) * pl.nkt and hi > tt * pl.nkt]
        assert holders == list(range(f, l + 1)), (case.name, tt, holders, f, l)      # the kernel's formula finds exactly the holders
        if l > f:
            out.add("pair" if l - f == 1 else "three-or-more")
            assert len({(b, slot(pl, b, tt)) for b in holders}) == len(holders)
    for b, (lo, hi) in enumerate(pl.ranges):
        if lo % pl.nkt and hi % pl.nkt and lo // pl.nkt != hi // pl.nkt:
            out.add("slots-0-and-1")
            assert slot(pl, b, lo // pl.nkt) == 0 and slot(pl, b, hi // pl.nkt) == 1
    return out
