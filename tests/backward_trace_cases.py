"""Small forward + backward cases of the backbone's autograd layer (erd_amd.functional) and the recorder of their launch schedule.
Shared by tests/test_gpu_backward_trace.py and tools/gen_backward_trace_golden.py (which writes tests/golden/backward_launch_trace.json).

A trace is the list of launches a case issues through ``kernels.call``: [C entry name, stream role] (+ the descriptor's ``ngroups`` for
``erd_conv_wgrad``).  The role is "main" for the stream that is current when the case starts, "trail" for ``functional.trail_stream``, "aux"
for any other.  No pointers and no split counts: the trace pins WHICH launches go out, in which order and on which stream.

Every case builds fresh parameters (the first use of a frozen-statistics BN differs from later ones in the fold cache), runs one forward and
one backward, joins the trailing stream and synchronizes.  It returns {name: tensor} of the input gradient and every parameter gradient."""
import torch

import golden_inputs as G

STAGE_EPS = 1e-5


def _mark_sinks(params):
    """what engine.FlatParams does: a zeroed gradient slot per trainable parameter, marked as the place the backward kernels write to"""
    for p in params:
        if isinstance(p, torch.nn.Parameter) and p.requires_grad:
            p.grad = torch.zeros_like(p)
            p._erd_sink = True
            if p.dim() == 4:
                assert p.permute(0, 2, 3, 1).is_contiguous() and p.grad.permute(0, 2, 3, 1).is_contiguous()


def _cl(w):      # OIHW cpu -> channels_last parameter on the GPU
    return torch.nn.Parameter(w.cuda().contiguous(memory_format=torch.channels_last))


def _vec(t):
    return torch.nn.Parameter(t.cuda())


def _grads(named, x):
    out = {"dx": x.grad.detach().float().cpu().clone()}
    for n, p in named:
        if isinstance(p, torch.nn.Parameter) and p.requires_grad:
            assert p.grad is not None, n
            out[n] = p.grad.detach().cpu().clone()
    return out


def _finish(Fn):
    Fn.trail_join()
    torch.cuda.synchronize()


# ---- stages: the stage of tests/test_gpu_wgrad_grouped.py (32 -> 8 -> 32 channels, input 2 x 12 x 20, stride 2) -------------------------------
def _stage_blocks(n_identity, cin=32, mid=8, seed=300):
    def conv(i, cout, ci, k):
        w = G.randn(seed + i, cout, ci, k, k) * (2.0 / (ci * k * k)) ** 0.5
        return [_cl(w), _vec(1.0 + 0.1 * G.randn(seed + i + 1, cout)), _vec(0.1 * G.randn(seed + i + 2, cout)),
                (0.1 * G.randn(seed + i + 3, cout)).cuda(), (1.0 + 0.2 * G.randn(seed + i + 4, cout).abs()).cuda()]

    blocks, i = [], 0
    for b in range(1 + n_identity):
        prm = []
        for cout, ci, k in [(mid, cin, 1), (mid, mid, 3), (cin, mid, 1)] + ([(cin, cin, 1)] if b == 0 else []):
            prm += conv(i, cout, ci, k)
            i += 5
        blocks.append(prm)
    return blocks


def stage(mode, n_identity, sink):
    def run():
        from erd_amd import functional as Fn, kernels as K
        K.set_compute(mode)
        blocks = _stage_blocks(n_identity)
        params = [p for b in blocks for p in b]
        if sink:
            _mark_sinks(params)
        x = G.randn(7, 2, 12, 20, 32).abs().to(K.act_dtype()).cuda().requires_grad_(True)
        dy = G.randn(8, 2, 6, 10, 32).to(K.act_dtype()).cuda()
        y = Fn.ResLayerFn.apply(x, (2,) + (1,) * n_identity, STAGE_EPS, tuple(len(b) for b in blocks), *params)
        y.backward(dy)
        _finish(Fn)
        return _grads([(f"p{i}", p) for i, p in enumerate(params)], x)
    return run


# ---- single blocks through modules.Bottleneck --------------------------------------------------------------------------------------------------
def block(cin, planes, stride, down, sink, H=12, W=20, **kw):
    def run():
        from erd_amd import functional as Fn, kernels as K
        from erd_amd.modules import Bottleneck
        K.set_compute("f32x3")
        blk = Bottleneck(cin, planes, stride, down, **kw)
        sd = {}
        for i, (k, v) in enumerate(blk.state_dict().items()):
            leaf = k.rsplit(".", 1)[-1]
            if leaf == "num_batches_tracked":
                sd[k] = v
            elif leaf == "running_var" or (leaf == "weight" and v.dim() == 1):
                sd[k] = 0.5 + G.rand(400 + i, *v.shape)
            elif v.dim() == 4:
                sd[k] = G.randn(400 + i, *v.shape, scale=(2.0 / (v.shape[1] * v.shape[2] * v.shape[3])) ** 0.5)
            else:
                sd[k] = G.randn(400 + i, *v.shape, scale=0.2)
        blk.load_state_dict(sd)
        blk = blk.cuda()
        named = list(blk.named_parameters())
        if sink:
            _mark_sinks([p for _, p in named])
        x = G.randn(9, 2, H, W, cin).abs().cuda().requires_grad_(True)
        y = blk(x)
        y.backward(G.randn(10, *y.shape).cuda())
        _finish(Fn)
        return _grads(named, x)
    return run


# ---- leaf nodes -------------------------------------------------------------------------------------------------------------------------
def _bn(seed, c):
    return (_vec(0.5 + G.rand(seed, c)), _vec(G.randn(seed + 1, c, scale=0.2)), G.randn(seed + 2, c, scale=0.2).cuda(),
            (0.5 + G.rand(seed + 3, c)).cuda())


def conv_bn_act(cin, cout, k, stride, res, relu, sink):
    def run():
        from erd_amd import functional as Fn, kernels as K
        K.set_compute("f32x3")
        w = _cl(G.randn(500, cout, cin, k, k, scale=(2.0 / (cin * k * k)) ** 0.5))
        gamma, beta, mean, var = _bn(501, cout)
        if sink:
            _mark_sinks([w, gamma, beta])
        x = G.randn(505, 2, 6, 10, cin).cuda().requires_grad_(True)
        oh, ow = K.conv_out_size(6, k, stride, k // 2), K.conv_out_size(10, k, stride, k // 2)
        r = G.randn(506, 2, oh, ow, cout).cuda().requires_grad_(True) if res else None
        y = Fn.ConvBNAct.apply(x, w, gamma, beta, mean, var, r, k, stride, k // 2, relu, 1e-5)
        y.backward(G.randn(507, *y.shape).cuda())
        _finish(Fn)
        out = _grads([("w", w), ("gamma", gamma), ("beta", beta)], x)
        if res:
            out["dres"] = r.grad.detach().cpu().clone()
        return out
    return run


def deform_conv_bn_act(c, stride, sink):
    def run():
        from erd_amd import functional as Fn, kernels as K
        K.set_compute("f32x3")
        w = _cl(G.randn(520, c, c, 3, 3, scale=(2.0 / (9 * c)) ** 0.5))
        w_off, b_off = _cl(G.randn(521, 18, c, 3, 3, scale=0.05)), _vec(G.randn(522, 18, scale=0.2))
        gamma, beta, mean, var = _bn(523, c)
        if sink:
            _mark_sinks([w, w_off, b_off, gamma, beta])
        x = G.randn(527, 2, 6, 10, c).cuda().requires_grad_(True)
        y = Fn.DeformConvBNAct.apply(x, w, w_off, b_off, gamma, beta, mean, var, stride, True, 1e-5)
        y.backward(G.randn(528, *y.shape).cuda())
        _finish(Fn)
        return _grads([("w", w), ("w_off", w_off), ("b_off", b_off), ("gamma", gamma), ("beta", beta)], x)
    return run


def head_conv_bias(cout, sink):
    def run():
        from erd_amd import functional as Fn, kernels as K
        K.set_compute("f32x3")
        sizes = [(6, 10), (3, 5)]
        w, b = _cl(G.randn(540, cout, 64, 3, 3, scale=(1.0 / 576) ** 0.5)), _vec(G.randn(541, cout, scale=0.1))
        if sink:
            _mark_sinks([w, b])
        x = G.randn(542, 2, 75, 64).cuda().requires_grad_(True)
        y = Fn.HeadConvBias.apply(x, w, b, sizes)
        y.backward(G.randn(543, *y.shape).cuda())
        _finish(Fn)
        return _grads([("w", w), ("b", b)], x)
    return run


def _cases():
    c = {"stage_f32x3_sink": stage("f32x3", 3, True), "stage_f32x3_nosink": stage("f32x3", 3, False),
         "stage_bf16_sink": stage("bf16", 3, True), "stage_f32x3_10_identity_sink": stage("f32x3", 10, True)}
    for sink in (True, False):
        s = "sink" if sink else "nosink"
        c[f"block_32_8_s2_down_{s}"] = block(32, 8, 2, True, sink)
        c[f"block_32_8_s1_identity_{s}"] = block(32, 8, 1, False, sink)
        c[f"conv_bn_act_3x3_s1_res_relu_{s}"] = conv_bn_act(16, 16, 3, 1, True, True, sink)
        c[f"conv_bn_act_1x1_s2_{s}"] = conv_bn_act(16, 32, 1, 2, False, False, sink)
        c[f"deform_16_s1_{s}"] = deform_conv_bn_act(16, 1, sink)
        c[f"deform_16_s2_{s}"] = deform_conv_bn_act(16, 2, sink)
        c[f"head_conv_bias_70_{s}"] = head_conv_bias(70, sink)
        c[f"head_conv_bias_80_{s}"] = head_conv_bias(80, sink)
    c["block_resnext_256_64_s2_down_sink"] = block(256, 64, 2, True, True, H=12, W=14, groups=32, base_width=4)
    return c


CASES = _cases()


def record(name):
    """run case `name` with every kernels.call recorded: (trace, {name: gradient})"""
    from erd_amd import functional as Fn, kernels as K
    dev = torch.device("cuda", torch.cuda.current_device())
    main, trail = torch.cuda.current_stream(dev).cuda_stream, Fn.trail_stream(dev).cuda_stream
    trace, real = [], K.call

    def recording(entry, *args):
        s = torch.cuda.current_stream(dev).cuda_stream
        e = [entry, "main" if s == main else ("trail" if s == trail else "aux")]
        if entry == "erd_conv_wgrad":
            e.append(int(args[0]._obj.ngroups))
        trace.append(e)
        return real(entry, *args)

    K.call = recording
    try:
        grads = CASES[name]()
    finally:
        K.call = real
        K.set_compute(K.DEFAULT_COMPUTE)
    return trace, grads


def first_difference(got, want):
    """None when equal, else a line naming the first index at which the traces differ, with both entries"""
    for i in range(max(len(got), len(want))):
        a, b = (got[i] if i < len(got) else None), (want[i] if i < len(want) else None)
        if a != b:
            return f"launch {i}: got {a}, pinned {b} (lengths {len(got)} / {len(want)})"
    return None
