"""CPU: the references and case tables of tests/wgrad_refs.py -- that the inputs make every kernel's arithmetic exact, that the
per-split unit sets partition the K axis, that the integer gradient agrees with torch's own weight gradient, and that the cases reach
the kernel instantiations tests/test_gpu_wgrad_exact.py claims to pin."""
import pytest
import torch

import wgrad_refs as Wr

ALL = [(c, ch, False) for c in Wr.ONE_TAP_CASES for ch in Wr.ONE_TAP_CHANNELS] + [(Wr.ROW3_CASE, ch, True) for ch in Wr.THREE_TAP_CHANNELS]


def test_every_value_and_every_sum_is_exact():
    """one bf16 limb holds every input (integers of magnitude <= 2: the bf16 rounding and the three-limb split leave them as they are),
    and no sum of products over a case's pixels can leave the integers fp32 holds exactly"""
    assert max(Wr.pixels(Wr.geometry(c)[1]) for c in Wr.ONE_TAP_CASES) == 498
    for case, (Cin, Cout), _ in ALL:
        x, dz = Wr.inputs(case, Cin, Cout)
        assert set(x.unique().tolist()) == {-1.0, 0.0, 1.0} and set(dz.unique().tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0}
        for t in (x, dz):
            assert torch.equal(t.bfloat16().float(), t)                    # limb 0 is the value, limbs 1 and 2 are zero
        assert 2 * Wr.pixels(Wr.geometry(case)[1]) < 2 ** 24               # |dz| * |x| * pixels bounds every partial sum


@pytest.mark.parametrize("three_taps,bk", [(False, Wr.BK_F32), (False, Wr.BK_BF16), (True, Wr.BK_F32)])
def test_splits_partition_the_axis(three_taps, bk):
    for case in ([Wr.ROW3_CASE] if three_taps else Wr.ONE_TAP_CASES):
        sizes_out = Wr.geometry(case)[1]
        us = Wr.units(sizes_out, three_taps, bk)
        counts = Wr.split_counts(len(us))
        assert counts[0] == 1 and len(counts) >= 2
        for S in counts:
            parts = Wr.split_units(us, S)
            assert len(parts) == S
            flat = [p for su in parts for u in su for p in u]
            assert flat == list(range(Wr.pixels(sizes_out)))               # every pixel once, in the axis' order
        assert Wr.split_units(us, counts[-1])[-1] == [] and all(Wr.split_units(us, counts[-1])[:-1])      # exactly the last split is empty
        if len(counts) == 3:
            last = Wr.split_units(us, counts[1])
            assert 0 < len(last[-1]) < len(last[0])                        # the last split is short
        if three_taps:
            assert all(1 <= len(u) <= Wr.CHUNK for u in us) and len(us) == Wr.N * sum(h * Wr.cdiv(w, Wr.CHUNK) for h, w in sizes_out)
        else:
            assert all(len(u) == bk for u in us[:-1]) and 0 < len(us[-1]) < bk      # the pixel count is no multiple of the slice
    if bk == Wr.BK_F32:
        assert all(len(Wr.split_counts(len(Wr.units(Wr.geometry(c)[1], three_taps, bk)))) == 3
                   for c in ([Wr.ROW3_CASE] if three_taps else Wr.ONE_TAP_CASES))


@pytest.mark.parametrize("case,ch,three_taps", ALL)
def test_integer_gradient_is_the_weight_gradient(case, ch, three_taps):
    Cin, Cout = ch
    sizes_in, sizes_out, k, stride, pad = Wr.geometry(case)
    x, dz = Wr.inputs(case, Cin, Cout)
    ref = torch.zeros(Cout, Cin, k, k, dtype=torch.float64)
    oi = oo = 0
    for (ih, iw), (h, w) in zip(sizes_in, sizes_out):
        xl = x[:, oi:oi + ih * iw].reshape(Wr.N, ih, iw, Cin).permute(0, 3, 1, 2).double()
        dl = dz[:, oo:oo + h * w].reshape(Wr.N, h, w, Cout).permute(0, 3, 1, 2).double()
        ref += torch.nn.grad.conv2d_weight(xl, (Cout, Cin, k, k), dl, stride=stride, padding=pad)
        oi, oo = oi + ih * iw, oo + h * w
    ref = ref.permute(0, 2, 3, 1).reshape(Cout, k * k, Cin)
    whole = Wr.wgrad_of(case, Cin, Cout, range(Wr.pixels(sizes_out)))
    assert torch.equal(whole.double(), ref)
    S = Wr.split_counts(len(Wr.units(sizes_out, three_taps)))[1]
    sl = Wr.slabs(case, Cin, Cout, three_taps, Wr.BK_F32, S)
    assert torch.equal(sl.sum(0), whole) and float(sl[-1].abs().max()) > 0


def test_the_cases_reach_every_instantiation():
    """erd_conv_wgrad's rules (restated in wgrad_refs.instantiation) send the cases to all twelve instantiations but the tuning aid
    conv_wgrad_kernel<128, 128, 32, 2> (ERD_WGRAD_VARIANT=0, read once per process), and every channel tile is ragged on one side"""
    got = {}
    for case, (Cin, Cout), three_taps in ALL:
        for mode in ("f32", "f32x3"):
            got.setdefault(Wr.instantiation(mode, three_taps, Cin, Cout), []).append((Cin, Cout))
        if not three_taps:
            for xb in (False, True):
                for db in (False, True):
                    got.setdefault(Wr.instantiation("bf16", False, Cin, Cout, xb, db), []).append((Cin, Cout))
    assert got["conv_wgrad_row3_kernel<1, 2, 1>"] == [(64, 64)] and got["conv_wgrad_row3_kernel<1, 3, 1>"] == [(128, 80)]
    assert got["conv_wgrad_row3_kernel<2, 2, 2>"] == [(68, 136)]
    assert got["conv_wgrad_row3_x3_kernel<1, 1, true>"] == [(64, 64)]
    assert got["conv_wgrad_row3_x3_kernel<2, 1, true>"] == [(128, 80), (68, 136)]
    assert sorted(got) == sorted(
        ["conv_wgrad_kernel<128, 128, 16, 4>", "conv_wgrad_row3_kernel<1, 2, 1>", "conv_wgrad_row3_kernel<1, 3, 1>",
         "conv_wgrad_row3_kernel<2, 2, 2>", "conv_wgrad_row3_x3_kernel<1, 1, true>", "conv_wgrad_row3_x3_kernel<2, 1, true>",
         "conv_wgrad_row3_x3_kernel<2, 2, false>"] + [f"conv_wgrad_bf16_kernel<{a}, {b}>" for a in ("false", "true") for b in ("false", "true")])
    for inst, chans in got.items():
        bm, bn = Wr.tile(inst)
        if chans != [(64, 64)]:                                            # (64 -> 64 fills its 64 x 64 / 64 x 128 tiles' rows exactly)
            assert any(Cout % bm or Cin % bn for Cin, Cout in chans), inst
