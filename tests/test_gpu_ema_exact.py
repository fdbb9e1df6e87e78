"""GPU: erd_ema_update and erd_swap_f32 at the C ABI, bit for bit against the host restatement tests/ema_refs.py (the kernel's
stated order: the multiply rounded on its own, then one fused multiply-add; c and 1 - c rounded once from the double).  Ranges of
every length around the 16-byte lane and the 256-lane tile, starting at element offsets 0, 4 and 64 of a larger buffer whose canary
words before and behind the range must stay untouched; special values in the first and the last lanes of every range."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ema_refs as E

SIZES = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 4099, (1 << 20) + 3]
OFFSETS = [0, 4, 64]
PAD = 64                                         # canary words behind the range
CANARY = np.uint32(0x4B1D5EED)                   # a finite fp32 pattern no result takes
COEFS = {"momentum": 0.0002, "expmomentum-steps1": E.coefficient("ExpMomentumEMA", 0.0002, 2000, 1), "half": 0.5, "zero": 0.0, "one": 1.0}
SPECIAL = np.array([0.0, -0.0, 1e-45, -1e-40, 1.1754942e-38, np.inf, -np.inf, np.nan, 3e38, -3e38, 1.0, -2.5], dtype=np.float32)
EINVAL = -1


@pytest.fixture(scope="module")
def K():
    from erd_amd import kernels
    assert torch.cuda.is_available()
    return kernels


@functools.lru_cache(maxsize=None)
def _values(n):
    """(average, weights) of n elements: a random bulk of weight-sized values, and every pair of SPECIAL values that fits into the
    first and the last lanes (the scalar tail included); read only"""
    rng = np.random.RandomState(1000 + n % 997)
    ema = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 1, n)).astype(np.float32)
    src = (ema * (1 + 0.05 * rng.standard_normal(n)) + 1e-3 * rng.standard_normal(n)).astype(np.float32)
    m = len(SPECIAL)
    k = min(n, m * m)
    idx = np.arange(k)
    ema[:k], src[:k] = SPECIAL[idx % m], SPECIAL[(idx // m + idx) % m]
    t = min(n - k, m)
    if t > 0:
        ema[n - t:], src[n - t:] = SPECIAL[:t], SPECIAL[::-1][:t]
    ema.setflags(write=False)
    src.setflags(write=False)
    return ema, src


def _framed(vals, off):
    """the values at element `off` of a buffer whose other words are the canary"""
    buf = np.full(off + vals.size + PAD, CANARY, dtype=np.uint32)
    buf[off:off + vals.size] = vals.view(np.uint32)
    return torch.from_numpy(buf.view(np.float32).copy()).cuda()


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _frame_untouched(t, off, n):
    b = _bits(t)
    return bool((b[:off] == CANARY).all() and (b[off + n:] == CANARY).all()) and b.size == off + n + PAD


@pytest.mark.parametrize("name", list(COEFS))
def test_ema_update_equals_the_restatement_bit_for_bit(K, name):
    c = COEFS[name]
    for n in SIZES:
        ema, src = _values(n)
        want = E.update(ema, src, c)
        for off in OFFSETS:
            e, p = _framed(ema, off), _framed(src, off)
            K.ema_update(e[off:off + n], p[off:off + n], c)
            torch.cuda.synchronize()
            got = e[off:off + n].cpu().numpy()
            assert E.same_bits(got, want), (name, n, off, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
            assert _frame_untouched(e, off, n), (name, n, off)
            assert np.array_equal(_bits(p), _bits(_framed(src, off))), "the weights are only read"


def test_the_values_reach_every_special_pair_and_the_tail():
    ema, src = _values(4099)
    pairs = {(a.tobytes(), b.tobytes()) for a, b in zip(ema[:144], src[:144])}
    assert len(pairs) == 144                                         # every (average, weight) pair of the 12 special values
    for n in SIZES:
        e, s = _values(n)
        assert e.size == n and s.size == n
    e, s = _values((1 << 20) + 3)                                    # the three elements of the scalar tail
    assert np.array_equal(e[-3:].view(np.uint32), SPECIAL[9:12].view(np.uint32))
    assert np.array_equal(s[-3:].view(np.uint32), SPECIAL[::-1][9:12].view(np.uint32))
    assert sum(int(np.isnan(_values(n)[0]).any() and np.isinf(_values(n)[1]).any()) for n in SIZES) >= 8


def test_copy_mode_and_empty_range(K):
    for n in SIZES:
        ema, src = _values(n)
        for off in OFFSETS:
            e, p = _framed(ema, off), _framed(src, off)
            K.ema_update(e[off:off + n], p[off:off + n], 0.3, copy=True)
            torch.cuda.synchronize()
            assert np.array_equal(_bits(e[off:off + n]), src.view(np.uint32)), (n, off)      # a copy keeps NaN payloads too
            assert _frame_untouched(e, off, n)
    e, p = _framed(_values(5)[0], 4), _framed(_values(5)[1], 4)
    before = _bits(e).copy()
    K.ema_update(e[4:4], p[4:4], 0.5)
    K.swap_(e[4:4], p[4:4])
    lib = K._lib.load()
    assert lib.erd_ema_update(None, None, 0, 0.5, 0.5, 0, None) == 0 and lib.erd_swap_f32(None, None, 0, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_bits(e), before)


def test_rejected_arguments_return_the_error_and_write_nothing(K):
    lib = K._lib.load()
    ema, src = _values(257)
    e, p = _framed(ema, 4), _framed(src, 4)
    be, bp = _bits(e).copy(), _bits(p).copy()
    pe, pp = e.data_ptr() + 16, p.data_ptr() + 16
    V = C.c_void_p
    bad = [(None, V(pp), 257), (V(pe), None, 257), (V(pe), V(pp), -1), (V(pe + 4), V(pp), 8), (V(pe), V(pp + 8), 8),
           (V(pe), V(pe + 16), 8)]                       # null, null, negative, misaligned, misaligned, overlapping
    for a, b, n in bad:
        assert lib.erd_ema_update(a, b, n, 0.5, 0.5, 0, None) == EINVAL and b"ema_update" in lib.erd_last_error(), (a, b, n)
        assert lib.erd_ema_update(a, b, n, 0.5, 0.5, 1, None) == EINVAL
        assert lib.erd_swap_f32(a, b, n, None) == EINVAL and b"swap_f32" in lib.erd_last_error(), (a, b, n)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(e), be) and np.array_equal(_bits(p), bp)
    with pytest.raises(K._lib.ErdHipError, match="GPU only"):
        K.ema_update(torch.zeros(4), torch.zeros(4), 0.5)
    with pytest.raises(AssertionError):
        K.ema_update(e[4:12], p[4:12].double(), 0.5)
    with pytest.raises(AssertionError):
        K.swap_(e[4:12], p[4:13])
    with pytest.raises(AssertionError):
        K.swap_(e[4:20:2], p[4:12])


def test_swap_exchanges_exactly_and_twice_is_the_identity(K):
    for n in SIZES:
        ema, src = _values(n)
        for off in OFFSETS:
            a, b = _framed(ema, off), _framed(src, off)
            K.swap_(a[off:off + n], b[off:off + n])
            torch.cuda.synchronize()
            assert np.array_equal(_bits(a[off:off + n]), src.view(np.uint32)), (n, off)
            assert np.array_equal(_bits(b[off:off + n]), ema.view(np.uint32)), (n, off)
            assert _frame_untouched(a, off, n) and _frame_untouched(b, off, n)
            K.swap_(a[off:off + n], b[off:off + n])
            torch.cuda.synchronize()
            assert np.array_equal(_bits(a), _bits(_framed(ema, off))) and np.array_equal(_bits(b), _bits(_framed(src, off)))


def test_the_grid_size_does_not_matter(K):
    """the same bits with 0 and with 32 compute units held back (kernels.set_cu_reserve sizes the streaming grid)"""
    n, off, c = SIZES[-1], 4, COEFS["expmomentum-steps1"]
    ema, src = _values(n)
    prev = K.set_cu_reserve(0)
    try:
        out = {}
        for reserve in (0, 32):
            K.set_cu_reserve(reserve)
            e, p = _framed(ema, off), _framed(src, off)
            K.ema_update(e[off:off + n], p[off:off + n], c)
            K.swap_(e[off:off + n], p[off:off + n])
            torch.cuda.synchronize()
            out[reserve] = (_bits(e), _bits(p))
            assert _frame_untouched(e, off, n) and _frame_untouched(p, off, n)
    finally:
        K.set_cu_reserve(prev)
    assert np.array_equal(out[0][0], out[32][0]) and np.array_equal(out[0][1], out[32][1])
    assert E.same_bits(out[0][1][off:off + n].view(np.float32), E.update(ema, src, c))
