"""GPU: the implicit-GEMM convolution conv_igemm_kernel (conv_mfma.hip) against the integer references of tests/igemm_refs.py, EXACTLY:
with activations in {-1, 0, 1}, weights in {-2 .. 2} and epilogue operands that keep every value a small multiple of 1/4
(tests/test_igemm_refs_cpu.py asserts it), every output element has one right value whatever the order of the additions and whatever
the stream-K partition -- a K-slice counted twice or not at all, a slab added from the wrong slot, a row or channel decoded wrongly, an
epilogue step out of order or an element left unwritten (outputs start as NaN) fails.  bf16-stored outputs are the exact value rounded
once.  Column sums are asserted as the sum over the `colsum_copies` rows (integers: float atomics add them exactly), not per row.

Every launch goes through kernels.conv_forward / conv_dgrad with the Winograd and thin kernels switched off, so that erd_conv_igemm's
own defaults pick the instantiation and launch_igemm's the grid; igemm_refs restates both as a function of the CU count and
test_igemm_refs_cpu.py asserts which instantiations and paths the cases reach at 256 CUs.  Switches the library reads once per process
(ERD_IGEMM_VARIANT, ERD_IG_FORCE, ERD_PT, ERD_SK_*, ERD_XCD) stay out of this file; ERD_IG_GLDS is read per launch."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import igemm_refs as R

NAN = float("nan")


@pytest.fixture()
def K():
    from erd_amd import _lib, kernels as K
    lib = _lib.load()
    keep, thin, reserve = K.WINOGRAD, int(lib.erd_conv_thin_enable(0)), K.set_cu_reserve(0)
    K.WINOGRAD = False
    yield K
    K.set_cu_reserve(reserve)
    lib.erd_conv_thin_enable(thin)
    K.WINOGRAD = keep
    K.set_compute(K.DEFAULT_COMPUTE)


def assert_exact(got, want, what):
    """every element equal, none NaN; the message names the first element that differs"""
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not torch.equal(got, want):
        bad = ~(got == want)
        first = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ ({int(torch.isnan(got).sum())} NaN); first at "
                             f"{first}: got {float(got[first])}, want {float(want[first])}")


def run(K, case):
    """one launch of the case on NaN-filled outputs: (outputs per segment, column-sum rows or None)"""
    d = R.inputs(case.name)
    _, outs = R.maps(case)
    idt = torch.bfloat16 if case.ab else torch.float32
    odt = torch.bfloat16 if case.ob else torch.float32
    dev = lambda t, dt=torch.float32: None if t is None else t.cuda().to(dt)
    xs = [dev(x, idt) for x in d["x"]]
    w = d["w"].cuda()
    if "base" in d:
        ys = [dev(b, odt) for b in d["base"]]
    else:
        ys = [torch.full((R.N, h, wd, case.C), NAN, device="cuda", dtype=odt) for h, wd in outs]
    res = [dev(r, odt) for r in d["res"]] if "res" in d else None
    cs = None
    if case.form == "fwd":
        K.conv_forward(xs, w, ys, case.k, case.stride, case.k // 2, scale=dev(d.get("scale")), shift=dev(d.get("shift")), res=res,
                       alphas=[a.cuda() for a in d["alpha"]] if "alpha" in d else None, relu="r" in case.epi)
    else:
        copies = 8 if "C" in case.epi else 1
        cs = torch.zeros(copies, case.C, device="cuda") if ("c" in case.epi or "C" in case.epi) else None
        K.conv_dgrad(xs, K.weight_transpose(w), ys, case.k, case.stride, case.k // 2, accumulate="base" in d, res=res,
                     relu_mask=[dev(m, odt) for m in d["mask"]] if "mask" in d else None, colsum=cs)
    torch.cuda.synchronize()
    return ys, cs


@pytest.mark.parametrize("name,glds", [(c.name, g) for c in R.CASES for g in R.glds_values(c)])      # (ERD_IG_GLDS: the three-limb mode's)
def test_every_element_is_the_integer_result(K, monkeypatch, name, glds):
    case = R.BY_NAME[name]
    from erd_amd import _lib
    lib = _lib.load()
    physical = int(lib.erd_usable_cus())
    K.set_cu_reserve(R.reserve_of(case, physical))
    usable = int(lib.erd_usable_cus())
    if physical != R.CUS or usable != (R.FEW if case.few else R.CUS):
        pytest.skip(f"the census of tests/test_igemm_refs_cpu.py assumes {R.CUS} CUs ({R.FEW} with the reserve): this device has {physical} ({usable})")
    monkeypatch.setenv("ERD_IG_GLDS", str(glds))
    K.set_compute(case.mode)
    want, want_cs = R.expected(name)
    got, cs = run(K, case)
    inst = R.instantiation(R.desc(case), glds, R.CUS, R.reserve_of(case))
    for i, (g, wnt) in enumerate(zip(got, want)):
        assert_exact(g, wnt, f"{name} ERD_IG_GLDS={glds} {tuple(inst)}: segment {i}")
    if want_cs is not None:
        assert_exact(cs.sum(0), want_cs, f"{name}: column sums over {cs.shape[0]} rows")
