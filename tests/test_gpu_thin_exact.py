"""GPU: the activation-stationary kernels for thin 1x1 convolutions, conv_thin_x3_kernel and conv_thin_bf16_kernel (conv_thin.hip),
against the integer references of tests/thin_refs.py, EXACTLY: with activations in {-1, 0, 1}, weights in {-2 .. 2} and epilogue
operands that keep every value a small multiple of 1/4 (tests/test_thin_refs_cpu.py asserts it), every output element has one right
value however the (pixel tile, channel block) units are cut into work ranges -- a unit dropped, computed twice or stored under another
block's index, a weight block taken from the wrong ring buffer, a row decoded into the wrong segment, an alpha / residual / mask left
out or an element left unwritten (outputs start as NaN) fails.  bf16-stored outputs are the exact value rounded once.  Column sums
start from a non-zero integer base and are asserted, exactly, as the sum over the `colsum_copies` rows.

Every launch goes through kernels.conv_forward / conv_dgrad with the thin kernels enabled and timing on: the recorded kernel class is
the library's own dispatch predicate applied to the real descriptor -- conv_thin_* for the served cases, conv_igemm_* for the ones the
predicate must refuse.  Most cases reserve all but eight CUs, so that the five pixel tiles give every workgroup several units
(test_thin_refs_cpu.py asserts which paths each grid reaches); four run on the whole chip, one unit per workgroup."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import thin_refs as T
from test_gpu_igemm_exact import assert_exact

NAN = float("nan")
GUARD = 3          # NaN rows in front of and behind a concatenated output


@pytest.fixture()
def K():
    from erd_amd import _lib, kernels as K
    lib = _lib.load()
    keep, thin, reserve = K.WINOGRAD, int(lib.erd_conv_thin_enable(1)), K.set_cu_reserve(0)
    K.WINOGRAD = False
    yield K
    K.set_cu_reserve(reserve)
    lib.erd_conv_thin_enable(thin)
    K.WINOGRAD = keep
    K.set_compute(K.DEFAULT_COMPUTE)


def _cat(K, maps, dt, guard=0, fill=None):
    """per-segment CPU maps [N, h, w, C] (or their sizes + a fill value) -> (the whole buffer [N, guard + A + guard, C] on the GPU,
    its level views): the image stride of a view is the buffer's, not h w C"""
    sizes = [tuple(m.shape[1:3]) for m in maps]
    C, A = maps[0].shape[3], sum(h * w for h, w in sizes)
    whole = torch.full((T.N, A + 2 * guard, C), NAN, device="cuda", dtype=dt)
    cat = whole[:, guard:guard + A, :]
    if fill is None:
        cat.copy_(torch.cat([m.reshape(T.N, -1, C) for m in maps], 1).to(dt))
    views = K.level_views(cat, sizes)
    assert all(v.stride(0) != v.shape[1] * v.shape[2] * C for v in views)
    return whole, views


def run(K, case):
    """one timed launch of the case on NaN-filled outputs -> (outputs per segment, column-sum rows or None, their base, the guard rows
    of a concatenated output or None, the kernel classes timing recorded)"""
    d = T.inputs(case.name)
    _, outs = T.maps(case)
    idt = torch.bfloat16 if case.ab else torch.float32
    odt = torch.bfloat16 if case.ob else torch.float32
    dev = lambda t, dt=torch.float32: None if t is None else t.cuda().to(dt)
    group = lambda ts, dt: None if ts is None else (_cat(K, ts, dt, GUARD)[1] if case.views else [dev(t, dt) for t in ts])
    xs = _cat(K, d["x"], idt)[1] if case.views else [dev(x, idt) for x in d["x"]]
    if case.stride == 2:       # a 1 x 1 / stride-2 launch reads the even rows and columns only: the rest must never be read
        for x in xs:
            x[:, 1::2] = NAN
            x[:, :, 1::2] = NAN
    w = d["w"].cuda()
    whole = None
    if "base" in d:
        ys = [dev(b, odt) for b in d["base"]]
    elif case.alias:
        ys = [dev(r, odt) for r in d["res"]]
    elif case.views:
        whole, ys = _cat(K, [torch.empty(T.N, h, wd, case.C) for h, wd in outs], odt, GUARD, fill=NAN)
    else:
        ys = [torch.full((T.N, h, wd, case.C), NAN, device="cuda", dtype=odt) for h, wd in outs]
    res = ys if case.alias else group(d.get("res"), odt)
    cs = base = None
    K.timing_begin()
    try:
        if case.form == "fwd":
            K.conv_forward(xs, w, ys, case.k, case.stride, case.k // 2, scale=dev(d.get("scale")), shift=dev(d.get("shift")), res=res,
                           alphas=[a.cuda() for a in d["alpha"]] if "alpha" in d else None, relu="r" in case.epi)
        else:
            if "c" in case.epi or "C" in case.epi:       # a non-zero integer base: a missing final flush or a double add shows
                copies = 8 if "C" in case.epi else 1
                base = ((torch.arange(copies * case.C) % 7).float() - 3.0).reshape(copies, case.C)
                cs = base.cuda()
            K.conv_dgrad(xs, K.weight_transpose(w), ys, case.k, case.stride, case.k // 2, accumulate="base" in d, res=res,
                         relu_mask=group(d.get("mask"), odt), colsum=cs)
    finally:
        rec = K.timing_end()
    guards = None if whole is None else torch.cat([whole[:, :GUARD], whole[:, -GUARD:]], 1)
    return ys, cs, base, guards, rec


@pytest.mark.parametrize("name", [c.name for c in T.CASES])
def test_every_element_is_the_integer_result(K, name):
    case = T.BY_NAME[name]
    from erd_amd import _lib
    lib = _lib.load()
    physical = int(lib.erd_usable_cus())
    K.set_cu_reserve(T.reserve_of(case, physical))
    usable = int(lib.erd_usable_cus())
    if physical != T.CUS or usable != (T.FEW if case.few else T.CUS):
        pytest.skip(f"the census of tests/test_thin_refs_cpu.py assumes {T.CUS} CUs ({T.FEW} with the reserve): this device has {physical} ({usable})")
    K.set_compute(case.mode)
    want, want_cs = T.expected(name)
    got, cs, cs_base, guards, rec = run(K, case)
    form = "fwd" if case.form == "fwd" else "dgrad"
    klass = ("conv_thin_" if case.served else "conv_igemm_") + form
    assert set(rec) == {klass} and rec[klass]["launches"] == 1, (name, sorted(rec))
    what = name
    if case.served:
        c = T.census(case)
        what = f"{name} {c.inst} on {c.G} workgroups"
    for i, (g, wnt) in enumerate(zip(got, want)):
        assert_exact(g, wnt, f"{what}: segment {i}")
    if want_cs is not None:
        assert_exact(cs.sum(0), want_cs + cs_base.sum(0), f"{what}: column sums over {cs.shape[0]} rows")
    if guards is not None:
        assert bool(torch.isnan(guards).all()), f"{what}: a guard row of the concatenated output was written"
