"""GPU: the kernels that rebuild, every step, what the step derives from the convolution weights alone -- erd_weight_transpose,
_bf16 and _x3, erd_split3, erd_wino_weights and _x3, their batched form erd_weight_prep_batch, kernels.ParamPrep that drives it, and
erd_bn_fold_batch -- against the references of tests/prep_refs.py, BIT FOR BIT (the BN fold: the bound of test_bn_fold_sizes).  Every
kernel is called at the C ABI.  The convolution tests feed these kernels weights in {-4, 0, 4}, whose mid and lo limbs are zero; here
the weights have random 24-bit significands plus the values at which a limb split can go wrong, at ragged channel counts, so that a
limb plane swapped or misplaced, a padding row left unwritten, a tap not reversed or a block of the batched kernel decoded into its
neighbour's item fails and is named: the message gives the first differing element as (plane, position, co, ci).

Every destination is a slice of one arena of 0xFF bytes -- read as fp32 a NaN, as 16 bits 0xFFFF -- with at least 1 KiB (256 fp32
elements, 512 16-bit ones) of guard in front of and behind it: after the launch every guard byte is still 0xFF and no element of a
destination is the sentinel (the padding rows of the images must be WRITTEN, as zeros)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import prep_refs as P
import reduce_refs as R

GUARD = 1024            # bytes; destinations start on a multiple of it, as the allocator's blocks do


@pytest.fixture(scope="module")
def K():
    from erd_amd import kernels
    assert torch.cuda.is_available()
    return kernels


class Arena:
    """destinations of the given byte sizes in one sentinel-filled buffer, guards between them"""

    def __init__(self, nbytes):
        self.nbytes, self.offs, off = list(nbytes), [], GUARD
        for n in self.nbytes:
            self.offs.append(off)
            off += R.cdiv(n, GUARD) * GUARD + GUARD
        self.buf = torch.full((off,), 0xFF, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0

    def view(self, j):
        return self.buf[self.offs[j]:self.offs[j] + self.nbytes[j]]

    def ptr(self, j):
        return C.c_void_p(self.buf.data_ptr() + self.offs[j])

    def check(self, refs, wheres, what):
        """refs: {destination: reference}; the destinations not named must be untouched, like the guards.  -> the bytes read back"""
        host = self.buf.cpu()
        guard = torch.ones(host.numel(), dtype=torch.bool)
        for j, want in refs.items():
            assert want.numel() * want.element_size() == self.nbytes[j], (what, j)
            raw = host[self.offs[j]:self.offs[j] + self.nbytes[j]]
            guard[self.offs[j]:self.offs[j] + self.nbytes[j]] = False
            got = raw.view(want.dtype).reshape(want.shape)
            why = P.explain(got, want, wheres[j])
            assert why is None, f"{what}, destination {j}: {why}"
            cells = raw.view(torch.int32 if want.element_size() == 4 else torch.int16)
            assert not bool((cells == -1).any()), f"{what}, destination {j}: an element was left unwritten"
        bad = (host[guard] != 0xFF).nonzero()
        assert bad.numel() == 0, f"{what}: {bad.numel()} guard bytes were written, the first at byte {int(guard.nonzero()[int(bad[0])])} of the arena"
        return host


def dev(t):
    return None if t is None else t.cuda()


def nbytes(ref):
    return ref.numel() * ref.element_size()


# ---------------------------------------------------------------------------------------------
# a. the single-item transposes
# ---------------------------------------------------------------------------------------------
T_ENTRY = {"f32": "erd_weight_transpose", "bf16": "erd_weight_transpose_bf16", "x3": "erd_weight_transpose_x3"}


@pytest.mark.parametrize("ntaps", P.T_NTAPS)
@pytest.mark.parametrize("out", P.T_OUTS)
def test_transposes(K, out, ntaps):
    cases = [c for c in P.T_CASES if c.ntaps == ntaps]
    assert len(cases) == 32
    refs = {j: P.transpose_ref(*P.transpose_inputs(c), c.flip, out) for j, c in enumerate(cases)}
    ar = Arena([nbytes(r) for r in refs.values()])
    keep = []
    for j, c in enumerate(cases):
        w, rs = P.transpose_inputs(c)
        wg, rg = dev(w), dev(rs)
        keep += [wg, rg]
        K.call(T_ENTRY[out], K._p(wg), K._p(rg), ar.ptr(j), c.Cout, c.ntaps, c.Cin, c.flip, K._stream())
    wheres = {j: (lambda f, c=c: (c, P.where_transposed(f, c.Cout, c.ntaps, c.Cin))) for j, c in enumerate(cases)}
    ar.check(refs, wheres, f"{T_ENTRY[out]}, {ntaps} taps")


# ---------------------------------------------------------------------------------------------
# b. the Winograd weight images
# ---------------------------------------------------------------------------------------------
def test_image_sizes(K):
    from erd_amd import _lib
    lib = _lib.load()
    for c in P.W_CASES:
        assert int(lib.erd_wino_weights_elems(c.Cout, c.Cin)) == P.wino_image_elems(c.Cout, c.Cin), c
        assert int(lib.erd_wino_weights_x3_elems(c.Cout, c.Cin)) == P.wino_image_x3_elems(c.Cout, c.Cin), c


@pytest.mark.parametrize("data", ["int", "w24"])
@pytest.mark.parametrize("Cin", P.W_CINS)
@pytest.mark.parametrize("x3", [False, True])
def test_wino_images(K, x3, Cin, data):
    cases = [c for c in P.W_CASES if c.Cin == Cin]
    assert len(cases) == 2 * len(P.W_COUTS)
    ref_of = P.wino_image_x3_ref if x3 else P.wino_image_ref
    refs = {j: ref_of(P.wino_inputs(c, data), c.flip) for j, c in enumerate(cases)}
    ar = Arena([nbytes(r) for r in refs.values()])
    keep = []
    for j, c in enumerate(cases):
        wg = dev(P.wino_inputs(c, data))
        keep.append(wg)
        K.call("erd_wino_weights_x3" if x3 else "erd_wino_weights", K._p(wg), ar.ptr(j), c.Cout, c.Cin, c.flip, K._stream())
    where = P.where_image_x3 if x3 else P.where_image
    wheres = {j: (lambda f, c=c: (c, where(f, c.Cout, c.Cin))) for j, c in enumerate(cases)}
    ar.check(refs, wheres, f"erd_wino_weights{'_x3' if x3 else ''}, Cin = {Cin}, {data} weights")


# ---------------------------------------------------------------------------------------------
# c. the limb planes
# ---------------------------------------------------------------------------------------------
def test_split3(K):
    xs = [P.split3_inputs(n) for n in P.SPLIT3_NS] + [P.edge_values()]
    refs = {j: P.split3_ref(x) for j, x in enumerate(xs)}
    ar = Arena([nbytes(r) for r in refs.values()])
    keep = [dev(x) for x in xs]
    for j, xg in enumerate(keep):
        K.call("erd_split3", K._p(xg), ar.ptr(j), xg.numel(), K._stream())
    wheres = {j: (lambda f, n=x.numel(): (n, P.where_planes(f, n))) for j, x in enumerate(xs)}
    ar.check(refs, wheres, "erd_split3")
    for xg, x in zip(keep, xs):
        assert R.same_bits(xg.cpu(), x)


# ---------------------------------------------------------------------------------------------
# d. the batched kernel
# ---------------------------------------------------------------------------------------------
def build_table(K, items, inputs, ar, first=0):
    """the device table of `items` with destinations first, first + 1, ... of the arena -> (table, total blocks, tensors to keep)"""
    from erd_amd import _lib
    lib = _lib.load()
    tab = (_lib.WeightPrepItem * len(items))()
    keep, blk = [], 0
    for j, (it, (w, rs)) in enumerate(zip(items, inputs)):
        wg, rg = dev(w), dev(rs)
        keep += [wg, rg]
        e = tab[j]
        e.w, e.rowscale, e.dst = wg.data_ptr(), 0 if rg is None else rg.data_ptr(), ar.ptr(first + j).value
        e.Cout, e.ntaps, e.Cin, e.flip, e.kind, e.block0 = it.Cout, it.ntaps, it.Cin, it.flip, it.kind, blk
        nb = int(lib.erd_weight_prep_blocks(it.kind, it.Cout, it.ntaps, it.Cin))
        assert nb == P.item_blocks(it), it
        blk += nb
    table = torch.frombuffer(bytearray(bytes(memoryview(tab))), dtype=torch.uint8).cuda()
    return table, blk, keep


def table_refs(name):
    items = P.TABLES[name]
    refs = {j: P.item_ref(it, w, rs) for j, (it, (w, rs)) in enumerate(zip(items, P.table_inputs(name)))}
    wheres = {j: (lambda f, j=j, it=it: (f"item {j}", it, P.item_where(it)(f))) for j, it in enumerate(items)}
    return items, refs, wheres


@pytest.mark.parametrize("name", sorted(P.TABLES))
def test_batched_prep(K, name):
    items, refs, wheres = table_refs(name)
    runs = []
    for rnd in range(2):
        ar = Arena([n * size for n, size in map(P.item_out, items)])
        table, blocks, keep = build_table(K, items, P.table_inputs(name), ar)
        K.call("erd_weight_prep_batch", K._p(table), len(items), blocks, K._stream())
        runs.append(ar.check(refs, wheres, f"erd_weight_prep_batch, table {name}, run {rnd}"))
    assert torch.equal(runs[0], runs[1])


def test_batched_prep_of_nothing_touches_nothing(K):
    from erd_amd import _lib
    lib = _lib.load()
    items = P.TABLES["alone-0"]
    ar = Arena([n * size for n, size in map(P.item_out, items)])
    table, blocks, keep = build_table(K, items, P.table_inputs("alone-0"), ar)
    assert lib.erd_weight_prep_batch(K._p(table), 0, blocks, K._stream()) == 0
    assert lib.erd_weight_prep_batch(K._p(table), len(items), 0, K._stream()) == 0
    torch.cuda.synchronize()
    ar.check({}, {}, "erd_weight_prep_batch with no items / no blocks")


# ---------------------------------------------------------------------------------------------
# e. ParamPrep without a trainer
# ---------------------------------------------------------------------------------------------
class Owner:
    """one weight [Cout, 9, Cin] with a row scale, registered as the trainer's wrappers register it: a level-0 transpose and, built
    from THAT buffer at level 1, the flipped Winograd images of both layouts and the limb planes"""
    Cout, Cin, n = 32, 17, 32 * 9 * 17          # the gradient form reads the transposed buffer as 17 rows of 32 channels

    def __init__(self, seed):
        self.w = [P.weights24(seed + k, self.Cout, 9, self.Cin) for k in range(2)]
        self.rs = P.rowscale24(seed + 9, self.Cout)
        self.wg, self.rg = self.w[0].cuda(), self.rs.cuda()
        self.key = id(self.wg)

    def nbytes(self):
        return [4 * self.n, 4 * P.wino_image_elems(self.Cin, self.Cout), 2 * P.wino_image_x3_elems(self.Cin, self.Cout), 2 * 3 * self.n]

    def keys(self):
        return [("T", self.key, False), ("UT", self.key), ("UT3", self.key), ("XT", self.key)]

    def register(self, prep, ar, first):
        T = ar.view(first)
        kT, kU, kU3, kX = self.keys()
        prep.register(kT, 0, self.wg, self.rg, T, self.Cout, 9, self.Cin, 0, self.wg, 0)
        prep.register(kU, 2, T, None, ar.view(first + 1), self.Cin, 9, self.Cout, 1, self.wg, 1)
        prep.register(kU3, 4, T, None, ar.view(first + 2), self.Cin, 9, self.Cout, 1, self.wg, 1)
        prep.register(kX, 3, T, None, ar.view(first + 3), self.Cin, 9, self.Cout, 0, self.wg, 1)

    def refs(self, k, first):
        T = P.transpose_ref(self.w[k], self.rs, 0, "f32")
        wt = T.reshape(self.Cin, 9, self.Cout)
        return {first: T, first + 1: P.wino_image_ref(wt, 1), first + 2: P.wino_image_x3_ref(wt, 1), first + 3: P.split3_ref(wt)}

    def wheres(self, first):
        ci, co = self.Cin, self.Cout
        return {first: lambda f: ("T", P.where_transposed(f, co, 9, ci)), first + 1: lambda f: ("UT", P.where_image(f, ci, co)),
                first + 2: lambda f: ("UT3", P.where_image_x3(f, ci, co)), first + 3: lambda f: ("XT", P.where_planes(f, self.n))}

    def update(self, k):
        """as the trainer's raw-pointer update does: new values, same version"""
        v = self.wg._version
        self.wg.data.copy_(self.w[k].cuda())
        assert self.wg._version == v


def test_param_prep_runs_level_0_before_level_1(K):
    o = Owner(9800)
    ar = Arena(o.nbytes())
    prep = K.ParamPrep("cuda")
    o.register(prep, ar, 0)
    assert all(prep.lookup(k) is None for k in o.keys())
    prep.run()
    ar.check(o.refs(0, 0), o.wheres(0), "ParamPrep.run, first weights")
    assert all(prep.lookup(k) is not None and prep.lookup(k).stamp == prep.stamp == 1 for k in o.keys())
    o.update(1)
    prep.run()
    # the level-1 buffers held the images of the OLD transposed weights: they are right only if level 0 ran first
    ar.check(o.refs(1, 0), o.wheres(0), "ParamPrep.run, updated weights")
    assert all(prep.lookup(k) is not None and prep.lookup(k).stamp == prep.stamp == 2 for k in o.keys())
    assert prep.lookup(o.keys()[0]).matches(o.wg, o.wg, o.rg) and not prep.lookup(o.keys()[0]).matches(o.wg, o.wg, None)


def test_param_prep_groups_and_stale_recipes(K):
    a, b = Owner(9820), Owner(9840)
    ar = Arena(a.nbytes() + b.nbytes())
    prep = K.ParamPrep("cuda")
    fired = []
    prep.on_stale = lambda: fired.append(1)
    prep.group_of = lambda owner: 0 if owner is a.wg else 1
    a.register(prep, ar, 0)
    b.register(prep, ar, 4)
    wheres = {**a.wheres(0), **b.wheres(4)}
    prep.run_group(0)
    ar.check(a.refs(0, 0), wheres, "run_group(0): the other group's buffers are untouched")
    assert all(prep.recipes[k].stamp == prep.stamp == 1 for k in a.keys()) and all(prep.recipes[k].stamp == -1 for k in b.keys())
    assert all(prep.lookup(k) is not None for k in a.keys()) and all(prep.lookup(k) is None for k in b.keys())
    a.update(1)
    prep.run_group(1)
    ar.check({**a.refs(0, 0), **b.refs(0, 4)}, wheres, "run_group(1): group 0 keeps the buffers of its old weights")
    assert all(prep.lookup(k) is not None for k in a.keys() + b.keys()) and prep.stamp == 1
    prep.run_group(0)
    ar.check({**a.refs(1, 0), **b.refs(0, 4)}, wheres, "run_group(0) after its update")
    assert not fired
    # an in-place edit behind the trainer's back: the recipe and what was built from its buffer go, the rest is rebuilt
    a.wg.mul_(1.0)
    b.update(1)
    prep.run()
    assert fired
    assert all(k not in prep.recipes for k in a.keys()) and all(prep.lookup(k) is not None for k in b.keys())
    ar.check({**a.refs(1, 0), **b.refs(1, 4)}, wheres, "run() after an in-place edit of one owner")


# ---------------------------------------------------------------------------------------------
# f. the batched BN fold
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_bn_fold_batch(K, order):
    from erd_amd import _lib
    js = list(range(len(P.BN_NS)))[::1 if order == "ascending" else -1]
    ar = Arena([4 * P.BN_NS[j] for j in js for _ in (0, 1)])          # scale, shift per item
    tab = (_lib.BnFoldItem * len(js))()
    keep = []
    for i, j in enumerate(js):
        g, b, m, v = (t.cuda() for t in P.bn_inputs(j))
        keep += [g, b, m, v]
        e = tab[i]
        e.gamma, e.beta, e.mean, e.var = g.data_ptr(), b.data_ptr(), m.data_ptr(), v.data_ptr()
        e.scale, e.shift, e.n, e.eps = ar.ptr(2 * i).value, ar.ptr(2 * i + 1).value, P.BN_NS[j], P.BN_EPS[j]
    table = torch.frombuffer(bytearray(bytes(memoryview(tab))), dtype=torch.uint8).cuda()
    K.call("erd_bn_fold_batch", K._p(table), len(js), max(P.BN_NS), K._stream())
    # sqrtf, the division and a contraction of beta - mean * s are the compiler's: the bound of test_bn_fold_sizes, not bits
    got = {i: ar.view(i).cpu().view(torch.float32) for i in range(2 * len(js))}
    for i, j in enumerate(js):
        s64, h64 = P.bn_fold_ref(*P.bn_inputs(j), P.BN_EPS[j], double=True)
        s32, h32 = P.bn_fold_ref(*P.bn_inputs(j), P.BN_EPS[j])
        sc, sh = got[2 * i], got[2 * i + 1]
        assert not bool(torch.isnan(sc).any() | torch.isnan(sh).any()), (order, j)
        errs = R.relerr(sc.double(), s64), R.relerr(sh.double(), h64)
        print("bn_fold_batch relerr:", order, P.BN_NS[j], errs, "ulps from the fp32 reference:",
              int(R.ulp_distance(sc, s32).max()), int(R.ulp_distance(sh, h32).max()))
        assert errs[0] < P.BN_BOUND and errs[1] < P.BN_BOUND, (order, j, errs)
    ar.check({i: t for i, t in got.items()}, {i: None for i in got}, f"erd_bn_fold_batch, {order}")       # guards; nothing unwritten
