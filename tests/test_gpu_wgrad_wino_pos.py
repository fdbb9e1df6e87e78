"""GPU: the one-position-per-workgroup kernel of the Winograd-domain weight gradient (wgrad_wino_pos_kernel, erd_amd/csrc/wgrad_wino.hip):
256 x 256 channels and one of the 16 positions per workgroup where tests/test_gpu_wgrad_wino.py's kernel owns a transform row of 128 x 128.

Exact level, as in that file: x in {-1, 0, 1}, dz in {-2 .. 2}, every transformed value one bf16 limb, every sum exact in any order -- the
reduced dW EQUALS the integer weight gradient, from NaN-filled slabs into a NaN-filled output.  The shapes are that file's, at the channel
counts this kernel takes, plus two channel tiles on either side (the decode of the channel-tile index).

Bit-equal slabs.  Both kernels add the same six limb products of the same transformed values in the same tile order into every
accumulator, so on ANY data the partial slabs are the same bits: torch.equal with ERD_WGRAD_WINO_TILE forcing each kernel, on real-valued
data (ReLU'd x, half-zero dz with signed zeros, a nonzero mean in every fourth channel).  No tolerance.

Routing, through the library's own answer (erd_conv_wgrad_wino_tile), not through logs."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import golden_inputs as G
import wgrad_refs as R
from test_gpu_wgrad_wino import REAL_SIZES, SEG5, _correlation64, _desc, _ntiles

SWITCH = "ERD_WGRAD_WINO_TILE"


@pytest.fixture()
def K(monkeypatch):
    from erd_amd import kernels as K
    monkeypatch.delenv(SWITCH, raising=False)
    K.set_compute("f32x3")
    yield K
    K.set_compute(K.DEFAULT_COMPUTE)
    K.set_cu_reserve(0)


@functools.lru_cache(maxsize=None)
def _int_case(N, sizes, Cin, Cout):
    """integer operands on the GPU and the integer dW (computed once per shape, left unchanged)"""
    A = sum(h * w for h, w in sizes)
    g = torch.Generator().manual_seed(5000 + 7 * N + A + Cin + 3 * Cout)
    x = torch.randint(-1, 2, (N, A, Cin), generator=g).float()
    dz = torch.randint(-2, 3, (N, A, Cout), generator=g).float()
    ref = _correlation64(x, dz, N, sizes, Cin, Cout)
    assert float(ref.abs().max()) < 2 ** 20 and torch.equal(ref, ref.round())
    return x.cuda(), dz.cuda(), ref.float()


def _tile(K, d):
    return int(K._lib.load().erd_conv_wgrad_wino_tile(C.byref(d)))


def _slabs(K, xg, dg, sizes, nsplit, want_tile):
    """erd_conv_wgrad_wino at a split count of our choosing into NaN-filled slabs, on the kernel the library says it takes"""
    d, Cout, Cin = _desc(K, xg, dg, sizes)
    assert K._lib.load().erd_conv_wgrad_wino_ok(C.byref(d)) == 1
    assert _tile(K, d) == want_tile
    d.nsplit = nsplit
    part = torch.full((nsplit, 16, Cout, Cin), float("nan"), device="cuda")
    d.part = part.data_ptr()
    K.call("erd_conv_wgrad_wino", C.byref(d), K._stream())
    torch.cuda.synchronize()
    assert not torch.isnan(part).any()
    return part


def _wino(K, xg, dg, sizes, nsplit, base=None, want_tile=256):
    part = _slabs(K, xg, dg, sizes, nsplit, want_tile)
    Cout, Cin = part.shape[2], part.shape[3]
    dW = torch.full((Cout, 3, 3, Cin), float("nan"), device="cuda") if base is None else base.clone().cuda()
    K.wgrad_wino_reduce(part, nsplit, dW, base is not None)
    torch.cuda.synchronize()
    return dW.cpu()


EXACT = [
    # N, sizes, Cin, Cout, nsplit
    (1, ((8, 16),), 256, 256, 1),                # two whole K-steps of one map
    (1, ((7, 11),), 256, 256, 1),                # odd both ways: last tile row and column half outside
    (1, ((5, 3),), 256, 256, 1),                 # narrower than a K-step: 2 tiles per row, 6 in all
    (2, ((7, 11), (5, 3)), 256, 256, 2),         # K-steps straddle tile rows, images and the segment boundary
    (2, SEG5, 256, 256, 3),                      # five segments
    (1, ((8, 16),), 256, 256, 5),                # more splits than K-steps: three empty slabs
    (1, ((8, 16),), 512, 256, 1),                # two channel tiles on the input side
    (1, ((8, 16),), 256, 512, 1),                # ... on the output side
]


@pytest.mark.parametrize("N,sizes,Cin,Cout,nsplit", EXACT)
def test_integer_weight_gradient_is_exact(K, N, sizes, Cin, Cout, nsplit):
    xg, dg, ref = _int_case(N, sizes, Cin, Cout)
    print(f"N {N} sizes {sizes} {Cin} -> {Cout}: {_ntiles(N, sizes)} tiles, {-(-_ntiles(N, sizes) // 16)} K-steps, nsplit {nsplit}")
    got = _wino(K, xg, dg, sizes, nsplit)
    assert torch.equal(got, ref), float((got - ref).abs().max())


def test_the_cases_are_what_they_claim():
    assert _ntiles(2, SEG5) % 16 != 0 and _ntiles(2, ((7, 11), (5, 3))) % 16 != 0 and _ntiles(1, ((5, 3),)) < 16
    assert -(-_ntiles(1, ((8, 16),)) // 16) < 5


def test_integer_case_of_the_direct_kernels_suite(K):
    """tests/wgrad_refs.py's three-tap case (N = 2, maps 13x21, 7x11, 20x36) against ITS integer reference, at 256 channels"""
    Cin = Cout = 256
    x, dz = R.inputs(R.ROW3_CASE, Cin, Cout)
    ref = R.wgrad_of(R.ROW3_CASE, Cin, Cout, range(R.pixels(R.ROW3_SIZES))).reshape(Cout, 3, 3, Cin)
    assert torch.equal(_wino(K, x.cuda(), dz.cuda(), R.ROW3_SIZES, 4), ref)


def test_cu_reserve_gives_the_identical_gradient(K):
    """the host path (its own split count, sized for the CUs in use) with and without a reserve of 8 CUs"""
    N, sizes = 2, SEG5
    xg, dg, ref = _int_case(N, sizes, 256, 256)
    xs, dzs = K.level_views(xg, sizes), K.level_views(dg, sizes)
    got = []
    for reserve in (0, 8):
        K.set_cu_reserve(reserve)
        assert K.conv_wgrad_wino_ok(xs, dzs)
        part, S = K.conv_wgrad_wino(xs, dzs)
        dW = torch.full((256, 3, 3, 256), float("nan"), device="cuda")
        K.wgrad_wino_reduce(part, S, dW, False)
        got.append((S, dW.cpu()))
    K.set_cu_reserve(0)
    print(f"host split counts: reserve 0 -> {got[0][0]}, reserve 8 -> {got[1][0]}")
    assert got[1][0] <= got[0][0] and got[0][0] * 16 <= 256
    assert torch.equal(got[0][1], ref) and torch.equal(got[1][1], ref)


def test_accumulation_onto_an_integer_base(K):
    N, sizes = 2, ((7, 11), (5, 3))
    xg, dg, ref = _int_case(N, sizes, 256, 256)
    base = torch.randint(-50, 51, ref.shape, generator=torch.Generator().manual_seed(5)).float()
    assert torch.equal(_wino(K, xg, dg, sizes, 2, base=base), base + ref)


# ---------------------------------------------------------------------------------------------------------------------
# the two kernels' slabs, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _real_operands(Cin, Cout):
    """x = ReLU of a normal, dz normal with half the entries zero and a nonzero mean in every fourth channel (test_gpu_wgrad_wino.py's data)"""
    N, A = 2, sum(h * w for h, w in REAL_SIZES)
    x = G.randn(61, N, A, Cin).clamp_min(0)
    dz = G.randn(62, N, A, Cout)
    dz[..., ::4] += 0.5
    dz = dz * (G.randn(63, N, A, Cout) > 0).float()
    return x.cuda(), dz.cuda()


@pytest.mark.parametrize("Cin,Cout", [(256, 256), (512, 256)])
def test_partial_slabs_equal_the_row_kernels_bit_for_bit(K, monkeypatch, Cin, Cout):
    xg, dg = _real_operands(Cin, Cout)
    for nsplit in (1, 3, 16):
        monkeypatch.setenv(SWITCH, "128")
        part_128 = _slabs(K, xg, dg, REAL_SIZES, nsplit, 128).clone()
        monkeypatch.setenv(SWITCH, "256")
        part_256 = _slabs(K, xg, dg, REAL_SIZES, nsplit, 256)
        differ = int((part_256.view(torch.int32) != part_128.view(torch.int32)).sum())
        print(f"{Cin} -> {Cout}, nsplit {nsplit}: {differ} of {part_128.numel()} slab words differ, max |slab| {float(part_128.abs().max()):.3e}")
        assert float(part_128.abs().max()) > 0
        assert torch.equal(part_256, part_128), (nsplit, differ)


# ---------------------------------------------------------------------------------------------------------------------
# routing
# ---------------------------------------------------------------------------------------------------------------------
def test_routing_by_channel_counts_and_by_the_switch(K, monkeypatch):
    def tile(Cin, Cout):
        xg = torch.zeros(1, 8 * 16, Cin, device="cuda")
        dg = torch.zeros(1, 8 * 16, Cout, device="cuda")
        return _tile(K, _desc(K, xg, dg, ((8, 16),))[0])

    assert tile(256, 256) == 256 and tile(512, 256) == 256 and tile(256, 512) == 256
    assert tile(128, 256) == 128 and tile(384, 256) == 128 and tile(256, 128) == 128
    monkeypatch.setenv(SWITCH, "128")
    assert tile(256, 256) == 128 and tile(128, 256) == 128
    monkeypatch.setenv(SWITCH, "256")      # (forces the kernel only where the shape allows it)
    assert tile(256, 256) == 256 and tile(384, 256) == 128
    # and the launch follows the answer: the 128 -> 256 layer, which only the row kernel can take, comes out exact under the switch
    xg, dg, ref = _int_case(1, ((8, 16),), 128, 256)
    assert torch.equal(_wino(K, xg, dg, ((8, 16),), 1, want_tile=128), ref)
