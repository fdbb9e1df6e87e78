"""GPU: the deformable convolution on random fp32 data against the fp64 restatement tests/deform_refs.py -- the sampling kernels at
every element within their rounding-error bounds, the layer node (functional.DeformConvBNAct) and the DCN Bottleneck within the
bounds the grouped layer and the ResNeXt block carry in tests/test_gpu_resnext.py, in the compute modes "f32" and "f32x3".

Error bounds of the kernels, |got - want| <= k * 2^-24 * sum |w_i| |x_i| (first order; u = 2^-24), from the operation order stated in
csrc/conv_deform.hip:
  col      k = 7.  ly = h - floor(h) is exact for h >= 0 (and where h < 0 it rounds once, but then hy only multiplies corners of row
           -1, which are zero); hy = 1 - ly rounds once: every weight that meets a nonzero corner carries ONE rounding.  A product of
           two weights: 2 + 1 = 3 roundings; times the corner value: 4; the three additions of ((t00 + t01) + t10) + t11 add up to 3
           more on the first term: 7.
  doffset  k = 5 + (ceil(C / 64) - 1) + 6.  x10 - x00: 1; times hx (which carries 1): 3; the sum of the two such products: 4; times
           dcol: 5; a lane adds its ceil(C / 64) channels in order (the first addition, to zero, is exact); the xor butterfly over the
           64 lanes adds 6 levels.  The magnitude is sum_c |g| (hx (|x10| + |x00|) + lx (|x11| + |x01|)).

The conv_offset gradients have no number in the project: their tolerance is 4 x the distance of the SAME restatement evaluated in
fp32 on the CPU to its fp64 evaluation on the test's own inputs (another summation order on the GPU), computed by the test and printed.
Measured (relative to the tensor's largest entry; EXPERIMENTS 8.8): layer cases, conv_offset.weight 0.87e-6 / 0.99e-6 / 1.23e-6 / 1.98e-6
and bias 0.48e-6 / 1.77e-6 / 0.72e-6 / 1.51e-6 (C 64 / 128 / 256 / 512); block cases, weight 0.74e-6 / 0.67e-6 / 1.91e-6 and bias
0.54e-6 / 0.62e-6 / 1.29e-6; the kernels read 0.55-1.19e-6 (weight) and 0.27-1.17e-6 (bias) against them."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("oracle_threads")]

import deform_refs as R
import golden_inputs as G

U24 = 2.0 ** -24
DCN = dict(type="DCN", deform_groups=1, fallback_on_stride=False)
SPREAD = 0.75      # standard deviation of the offsets the tests produce: about +-1.5 pixels at two sigma


def relerr(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-20))


def worst(err, bound):
    return float((err / bound.clamp(min=1e-300)).max())


@pytest.fixture()
def K():
    from erd_amd import kernels as K
    yield K
    K.set_compute(K.DEFAULT_COMPUTE)


# ---- kernels: error bounds at every element -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cc,s", [(4, 1), (68, 2), (64, 1), (128, 2), (512, 1), (512, 2)])
def test_sampling_kernels_within_their_rounding_bounds_of_fp64(K, Cc, s):
    N, H, W = 2, 13, 17
    OH, OW = R.out_hw(H, W, s)
    x, dcol = G.randn(10 + Cc, N, H, W, Cc), G.randn(11 + Cc, N, OH, OW, 9 * Cc)
    off = G.randn(12 + Cc, N, OH, OW, 18, scale=1.5)      # a third of the samples leave their cell; the borders see outside samples
    off.view(-1)[::97] *= 8.0                             # and some leave the map altogether
    col = torch.full((N, OH, OW, 9 * Cc), float("nan"), device="cuda")
    K.deform_cols(x.cuda(), off.cuda(), s, out=col)
    want = R.deform_cols(x, off, s).reshape(N, OH, OW, 9 * Cc)
    mag = R.deform_cols_abs(x, off, s).reshape(N, OH, OW, 9 * Cc)
    assert 0.02 < float((want == 0).double().mean()) < 0.5      # outside samples exist and are the minority
    ratio = worst((col.cpu().double() - want).abs(), 7 * U24 * mag)
    print(f"col C {Cc} s{s}: worst err / bound {ratio:.3f}")
    assert bool(((col.cpu() == 0) | (mag > 0)).all()) and ratio <= 1.0

    base = G.randn(13 + Cc, N, H, W, Cc)
    dx, doff = base.cuda(), torch.full((N, OH, OW, 18), float("nan"), device="cuda")
    K.deform_cols_bwd(dcol.cuda(), x.cuda(), off.cuda(), s, dx, doff)
    dx_want, doff_want = R.deform_cols_bwd(dcol, x, off, s)
    k = 5 + ((Cc + 63) // 64 - 1) + 6
    ratio = worst((doff.cpu().double() - doff_want).abs(), k * U24 * R.deform_doffset_abs(dcol, x, off, s))
    print(f"doffset C {Cc} s{s}: worst err / bound {ratio:.3f} (k = {k})")
    assert ratio <= 1.0
    # dx: an element is its base plus n contributions, n = the (sample, corner) pairs landing on the pixel; a contribution carries 4
    # roundings (two weights, their product, times dcol) and ANY order of the n atomic additions rounds at most n times, each below
    # u times the sum of the magnitudes
    dx_mag, _ = R.deform_cols_bwd(dcol.abs(), x.abs(), off, s)
    n = R.corner_counts(off, (H, W), s).unsqueeze(-1)
    ratio = worst((dx.cpu().double() - (dx_want + base.double())).abs(), (n + 4) * U24 * (dx_mag + base.double().abs()))
    print(f"dx C {Cc} s{s}: worst err / bound {ratio:.3f} (up to {int(n.max())} additions)")
    assert ratio <= 1.0


# ---- the layer node --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def layer_case(N, H, W, Cc, Cout, s):
    seed = 1000 + Cc + 7 * s
    x = G.randn(seed, N, H, W, Cc)
    w = G.randn(seed + 1, Cout, Cc, 3, 3, scale=(2.0 / (9 * Cc)) ** 0.5)
    w_off, b_off = G.randn(seed + 2, 18, Cc, 3, 3), G.randn(seed + 3, 18, scale=0.2)
    w_off = w_off * (SPREAD / float(R.conv_offset(x, w_off, None, s).std()))
    gamma, beta = 0.5 + G.rand(seed + 4, Cout), G.randn(seed + 5, Cout, scale=0.2)
    mean, var = G.randn(seed + 6, Cout, scale=0.2), 0.5 + G.rand(seed + 7, Cout)
    OH, OW = R.out_hw(H, W, s)
    dy = G.randn(seed + 8, N, OH, OW, Cout)
    t = dict(x=x, w=w, w_off=w_off, b_off=b_off, gamma=gamma, beta=beta)
    refs = {}
    for dtype in (torch.float64, torch.float32):
        leaf = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in t.items()}
        off = R.conv_offset(leaf["x"], leaf["w_off"], leaf["b_off"], s)
        z = R.deform_conv(leaf["x"], off, leaf["w"], s, dtype)
        y = F.relu((z - mean.to(dtype)) / torch.sqrt(var.to(dtype) + 1e-5) * leaf["gamma"] + leaf["beta"])
        y.backward(dy.to(dtype))
        refs[dtype] = dict(y=y.detach(), off=off.detach(), **{"d" + k: v.grad for k, v in leaf.items()})
    return dict(t, mean=mean, var=var, dy=dy, ref=refs[torch.float64], ref32=refs[torch.float32])


def offset_grad_tolerance(c, what):
    """4 x the distance of the fp32 evaluation of the restatement to its fp64 evaluation, relative to the largest entry"""
    d = relerr(c["ref32"][what].double(), c["ref"][what])
    print(f"{what}: fp32 restatement to fp64 {d:.2e} -> tolerance {4 * d:.2e}")
    return 4 * d


@pytest.mark.parametrize("mode", ["f32", "f32x3"])
@pytest.mark.parametrize("N,H,W,Cc,Cout,s", [(2, 8, 10, 128, 128, 1), (2, 7, 9, 256, 256, 2), (2, 8, 10, 512, 512, 1), (2, 16, 20, 64, 64, 2)])
def test_deform_conv_bn_act(K, mode, N, H, W, Cc, Cout, s):
    from erd_amd import functional as Fn
    c = layer_case(N, H, W, Cc, Cout, s)
    ref = c["ref"]
    spread = float(ref["off"].std())
    assert 0.6 < spread < 0.9 and float((ref["off"].abs() > 1.0).double().mean()) > 0.1, spread      # about +-1.5 pixels, not zero
    K.set_compute(mode)
    cl = lambda w: w.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    xg = c["x"].cuda().requires_grad_(True)
    wg, wog = cl(c["w"]), cl(c["w_off"])
    bog, gg, bg = (c[k].cuda().requires_grad_(True) for k in ("b_off", "gamma", "beta"))
    out = Fn.DeformConvBNAct.apply(xg, wg, wog, bog, gg, bg, c["mean"].cuda(), c["var"].cuda(), s, True, 1e-5)
    e = relerr(out.detach().cpu().double(), ref["y"])
    print(f"{mode} C {Cc} s{s}: out {e:.2e}")
    assert e < 2e-5
    out.backward(c["dy"].cuda())
    torch.cuda.synchronize()
    errs = dict(dx=relerr(xg.grad.cpu().double(), ref["dx"]), dw=relerr(wg.grad.cpu().double(), ref["dw"]),
                dgamma=relerr(gg.grad.cpu().double(), ref["dgamma"]), dbeta=relerr(bg.grad.cpu().double(), ref["dbeta"]),
                dw_off=relerr(wog.grad.cpu().double(), ref["dw_off"]), db_off=relerr(bog.grad.cpu().double(), ref["db_off"]))
    print(f"{mode} C {Cc} s{s}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert tuple(wg.grad.shape) == (Cout, Cc, 3, 3) and tuple(wog.grad.shape) == (18, Cc, 3, 3)
    assert errs["dx"] < 5e-5 and errs["dw"] < 5e-5 and errs["dgamma"] < 2e-4 and errs["dbeta"] < 5e-5
    assert errs["dw_off"] <= offset_grad_tolerance(c, "dw_off") and errs["db_off"] <= offset_grad_tolerance(c, "db_off")


# ---- the DCN Bottleneck ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def block_case(cin, planes, li, b):
    from erd_amd.modules import Bottleneck
    N, H, W = 2, 12, 14
    stride, down = (2 if (b == 0 and li > 0) else 1), b == 0
    p = f"layer{li + 1}.{b}."
    blk = Bottleneck(cin, planes, stride, down, dcn=DCN)
    sd = {}
    for i, (k, v) in enumerate(blk.state_dict().items()):
        leaf = k.rsplit(".", 1)[-1]
        if leaf == "num_batches_tracked":
            sd[k] = v
        elif leaf == "running_var" or (leaf == "weight" and v.dim() == 1 and "conv_offset" not in k):
            sd[k] = 0.5 + G.rand(100 + i, *v.shape)
        elif v.dim() == 4:
            sd[k] = G.randn(100 + i, *v.shape, scale=(2.0 / (v.shape[1] * v.shape[2] * v.shape[3])) ** 0.5)
        else:
            sd[k] = G.randn(100 + i, *v.shape, scale=0.2)
    x = G.randn(90 + li, N, cin, H, W)
    # scale conv_offset so that the offsets spread over about +-1.5 pixels
    sub = {p + k: v.double() if v.dtype == torch.float32 else v for k, v in sd.items()}
    o1 = F.relu(R.O._bn_eval(F.conv2d(x.double(), sub[p + "conv1.weight"]), sub, p + "bn1")).permute(0, 2, 3, 1)
    sd["conv2.conv_offset.weight"] = sd["conv2.conv_offset.weight"] * (SPREAD / float(R.conv_offset(o1, sub[p + "conv2.conv_offset.weight"], None, stride).std()))
    refs = {}
    for dtype in (torch.float64, torch.float32):
        leaf = {k: (v.detach().clone().to(dtype).requires_grad_(True) if v.dtype == torch.float32 and "running" not in k else
                    (v.to(dtype) if v.dtype == torch.float32 else v)) for k, v in sd.items()}
        xr = x.detach().clone().to(dtype).requires_grad_(True)
        y = R.dcn_block({p + k: v for k, v in leaf.items()}, xr, li, b)
        dy = G.randn(91, *y.shape)
        y.backward(dy.to(dtype))
        refs[dtype] = dict(y=y.detach(), dx=xr.grad, grads={k: v.grad for k, v in leaf.items() if v.dtype == dtype and v.grad is not None})
    off = R.conv_offset(F.relu(R.O._bn_eval(F.conv2d(x.double(), sub[p + "conv1.weight"]), sub, p + "bn1")).permute(0, 2, 3, 1),
                        sd["conv2.conv_offset.weight"].double(), sd["conv2.conv_offset.bias"].double(), stride)
    return dict(sd=sd, x=x, dy=dy, stride=stride, down=down, ref=refs[torch.float64], ref32=refs[torch.float32], spread=float(off.detach().std()))


@pytest.mark.parametrize("mode", ["f32", "f32x3"])
@pytest.mark.parametrize("cin,planes,li,b", [(256, 128, 1, 0), (512, 128, 1, 1), (1024, 512, 3, 0)])
def test_dcn_bottleneck_block(K, mode, cin, planes, li, b):
    """composed leaf nodes (ConvBNAct, DeformConvBNAct, ConvBNAct with the shortcut) against autograd of the fp64 block"""
    from erd_amd.modules import Bottleneck
    c = block_case(cin, planes, li, b)
    assert 0.6 < c["spread"] < 0.9, c["spread"]
    K.set_compute(mode)
    blk = Bottleneck(cin, planes, c["stride"], c["down"], dcn=DCN)
    blk.load_state_dict(c["sd"])
    blk = blk.cuda()
    ref = c["ref"]
    xg = c["x"].permute(0, 2, 3, 1).contiguous().cuda().requires_grad_(True)
    out = blk(xg)
    e = relerr(out.detach().permute(0, 3, 1, 2).cpu().double(), ref["y"])
    print(f"{mode} block {cin}->{planes} s{c['stride']}: out {e:.2e}")
    assert e < 2e-5
    out.backward(c["dy"].permute(0, 2, 3, 1).contiguous().cuda())
    from erd_amd import functional as Fn
    Fn.trail_join(xg.device)
    torch.cuda.synchronize()
    assert relerr(xg.grad.permute(0, 3, 1, 2).cpu().double(), ref["dx"]) < 1e-4
    for k, p in blk.named_parameters():
        e = relerr(p.grad.cpu().double(), ref["grads"][k])
        if "conv_offset" in k:
            d = relerr(c["ref32"]["grads"][k].double(), ref["grads"][k])
            print(f"{mode} {k}: {e:.2e} (fp32 restatement to fp64 {d:.2e} -> tolerance {4 * d:.2e})")
            assert e <= 4 * d, k
        else:
            assert e < 3e-4, (k, e)
