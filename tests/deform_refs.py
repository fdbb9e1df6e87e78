"""Host reference of the deformable convolution (DCNv1) and of ResNet backbones with DCN blocks (test-only, CPU, pure torch).

The operator is the one DESIGN 8 fixes (mmcv is not available to pin against): 3x3, pad 1, dilation 1, deform_groups 1, groups 1,
stride 1 | 2, maps NHWC.  offset[..., 2t] / [..., 2t + 1] displace tap t = 3 i + j in y / x; the sampling position is ONE fp32
addition per coordinate, (float)(oy * s - 1 + i) + dy, and is otherwise carried in the evaluation's dtype (fp64 by default); a sample
is 0 unless h > -1, w > -1, h < H, w < W; bilinear corners outside the map contribute 0.  Gradients come from autograd with
floor() and the inside mask detached.  The four-term sum keeps the kernels' operation order, so that an fp32 evaluation of this file
is the fp32 restatement the tests measure tolerances with."""
from typing import Dict, List, Tuple

import torch
import torch.nn.functional as F

from oracle import erd_oracle as O

Tensor = torch.Tensor


def out_hw(H: int, W: int, s: int) -> Tuple[int, int]:
    return (H - 1) // s + 1, (W - 1) // s + 1


def positions(offset: Tensor, stride: int, dtype=torch.float64, round_pos: bool = True) -> Tuple[Tensor, Tensor]:
    """(h, w) [N, OH, OW, 9] of every tap; round_pos: the position is formed by one fp32 addition (the operator), else in `dtype`"""
    N, OH, OW, _ = offset.shape
    t = torch.arange(9)
    by = (torch.arange(OH) * stride - 1).view(1, OH, 1, 1) + (t // 3).view(1, 1, 1, 9)
    bx = (torch.arange(OW) * stride - 1).view(1, 1, OW, 1) + (t % 3).view(1, 1, 1, 9)
    off = offset.reshape(N, OH, OW, 9, 2)
    if round_pos:
        return (by.float() + off[..., 0].float()).to(dtype), (bx.float() + off[..., 1].float()).to(dtype)
    return by.to(dtype) + off[..., 0].to(dtype), bx.to(dtype) + off[..., 1].to(dtype)


def _corners(x: Tensor, h: Tensor, w: Tensor):
    """weights (ly, lx, hy, hx) [N, OH, OW, 9, 1] and the four corner values [N, OH, OW, 9, C] (0 outside the map / the inside test)"""
    N, IH, IW, C = x.shape
    inside = ((h > -1) & (w > -1) & (h < IH) & (w < IW)).detach()
    h0, w0 = torch.floor(h).detach(), torch.floor(w).detach()
    ly, lx = (h - h0).unsqueeze(-1), (w - w0).unsqueeze(-1)
    hy, hx = 1 - ly, 1 - lx
    r0, c0 = h0.clamp(-2, IH + 1).long(), w0.clamp(-2, IW + 1).long()
    n = torch.arange(N).view(N, 1, 1, 1)
    flat = x.reshape(N * IH * IW, C)
    vals = []
    for dy in (0, 1):
        for dx in (0, 1):
            r, c = r0 + dy, c0 + dx
            ok = inside & (r >= 0) & (r <= IH - 1) & (c >= 0) & (c <= IW - 1)
            idx = (n * IH + r.clamp(0, IH - 1)) * IW + c.clamp(0, IW - 1)
            vals.append(flat[idx.reshape(-1)].reshape(*idx.shape, C) * ok.unsqueeze(-1).to(x.dtype))
    zero = torch.zeros((), dtype=x.dtype)
    keep = inside.unsqueeze(-1)      # an outside sample has no weights either (a position of 3e9 must not reach an output as inf * 0)
    ly, lx, hy, hx = (torch.where(keep, v, zero) for v in (ly, lx, hy, hx))
    return (ly, lx, hy, hx), vals


def deform_cols(x: Tensor, offset: Tensor, stride: int, dtype=torch.float64, round_pos: bool = True) -> Tensor:
    """col [N, OH, OW, 9, C] in `dtype`: ((hy hx x00 + hy lx x01) + ly hx x10) + ly lx x11"""
    h, w = positions(offset, stride, dtype, round_pos)
    (ly, lx, hy, hx), (v00, v01, v10, v11) = _corners(x.to(dtype), h, w)
    return (((hy * hx) * v00 + (hy * lx) * v01) + (ly * hx) * v10) + (ly * lx) * v11


def deform_cols_abs(x: Tensor, offset: Tensor, stride: int) -> Tensor:
    """sum |w_i| |x_i| of every sample (the magnitude its rounding-error bound scales with)"""
    return deform_cols(x.abs(), offset, stride)


def deform_cols_bwd(dcol: Tensor, x: Tensor, offset: Tensor, stride: int, dtype=torch.float64) -> Tuple[Tensor, Tensor]:
    """(dx [N, IH, IW, C], doffset [N, OH, OW, 18]) of <dcol, col> by autograd"""
    xr, orr = x.to(dtype).requires_grad_(True), offset.to(dtype).requires_grad_(True)
    col = deform_cols(xr, orr, stride, dtype)
    dx, do = torch.autograd.grad((col * dcol.to(dtype).reshape(col.shape)).sum(), (xr, orr))
    return dx, do


def deform_doffset_abs(dcol: Tensor, x: Tensor, offset: Tensor, stride: int) -> Tensor:
    """sum_c |g| (hx (|x10| + |x00|) + lx (|x11| + |x01|)) and the symmetric expression, [N, OH, OW, 18]"""
    h, w = positions(offset, stride)
    (ly, lx, hy, hx), (v00, v01, v10, v11) = _corners(x.double().abs(), h, w)
    g = dcol.double().abs().reshape(v00.shape)
    ay = (g * (hx * (v10 + v00) + lx * (v11 + v01))).sum(-1)
    ax = (g * (hy * (v01 + v00) + ly * (v11 + v10))).sum(-1)
    return torch.stack((ay, ax), -1).reshape(offset.shape)


def corner_counts(offset: Tensor, in_hw: Tuple[int, int], stride: int) -> Tensor:
    """[N, IH, IW]: how many (sample, corner) pairs land on each input pixel -- the additions the scatter makes into one dx element"""
    IH, IW = in_hw
    N = offset.shape[0]
    h, w = positions(offset, stride)
    inside = (h > -1) & (w > -1) & (h < IH) & (w < IW)
    r0, c0 = torch.floor(h).clamp(-2, IH + 1).long(), torch.floor(w).clamp(-2, IW + 1).long()
    n = torch.arange(N).view(N, 1, 1, 1).expand_as(r0)
    cnt = torch.zeros(N * IH * IW, dtype=torch.float64)
    for dy in (0, 1):
        for dx in (0, 1):
            r, c = r0 + dy, c0 + dx
            ok = inside & (r >= 0) & (r <= IH - 1) & (c >= 0) & (c <= IW - 1)
            cnt.index_add_(0, ((n * IH + r) * IW + c)[ok], torch.ones(int(ok.sum()), dtype=torch.float64))
    return cnt.view(N, IH, IW)


def conv_offset(x: Tensor, w_off: Tensor, b_off: Tensor, stride: int) -> Tensor:
    """offset [N, OH, OW, 18] = conv3x3(x [NHWC], w_off [18, C, 3, 3] OIHW) + b_off at the layer's stride, pad 1"""
    return F.conv2d(x.permute(0, 3, 1, 2), w_off, b_off, stride, 1).permute(0, 2, 3, 1).contiguous()


def deform_conv(x: Tensor, offset: Tensor, w: Tensor, stride: int, dtype=torch.float64, round_pos: bool = True) -> Tensor:
    """y [N, OH, OW, Cout] = col . W^T with W the OIHW parameter [Cout, C, 3, 3] in its OHWI view [Cout, 9 C]"""
    col = deform_cols(x, offset, stride, dtype, round_pos)
    N, OH, OW = col.shape[:3]
    return col.reshape(N, OH, OW, -1) @ w.to(dtype).permute(0, 2, 3, 1).reshape(w.shape[0], -1).t()


def dcn_conv2_nchw(x: Tensor, w: Tensor, w_off: Tensor, b_off: Tensor, stride: int) -> Tensor:
    """DeformConv2dPack.forward on an NCHW map in the map's dtype: offsets from conv_offset, then the deformable convolution"""
    xh = x.permute(0, 2, 3, 1)
    off = conv_offset(xh, w_off, b_off, stride)
    return deform_conv(xh, off, w, stride, x.dtype).permute(0, 3, 1, 2)


# ----------------------------------------------------------------------------------------------------------------
# ResNet with DCN blocks (resnet.py:174-197, 448-481), composed with the oracle's restatements
# ----------------------------------------------------------------------------------------------------------------
def dcn_param_shapes(depth: int, stage_with_dcn=(False, True, True, True), fallback_on_stride: bool = False) -> Dict[str, Tuple[int, ...]]:
    """state-dict keys / shapes of a ResNet with dcn=dict(type='DCN', deform_groups=1): the ResNet's plus conv2.conv_offset.*"""
    s = dict(O.resnet_param_shapes(depth))
    for li, nblk in enumerate(O.RESNET_BLOCKS[depth]):
        planes = 64 * 2 ** li
        for b in range(nblk):
            stride = 2 if (b == 0 and li > 0) else 1
            if stage_with_dcn[li] and not (fallback_on_stride and stride > 1):
                s[f"layer{li + 1}.{b}.conv2.conv_offset.weight"] = (18, planes, 3, 3)
                s[f"layer{li + 1}.{b}.conv2.conv_offset.bias"] = (18,)
    return s


def dcn_gfl_state_dict(num_classes: int, depth: int = 50, seed: int = 0, offset_scale: float = 1.0, offset_zero: bool = False) -> Dict[str, Tensor]:
    """procedural weights (O.procedural_tensor) of a GFL detector on a DCN c3-c5 backbone; the conv_offset parameters are the
    procedural tensors times offset_scale (or zero: mmcv's initialisation)"""
    shapes = O.gfl_param_shapes(num_classes, depth)
    shapes.update({"backbone." + k: v for k, v in dcn_param_shapes(depth).items()})
    sd = {k: O.procedural_tensor(seed, k, shp) for k, shp in shapes.items()}
    for k in sd:
        if ".conv_offset." in k:
            sd[k] = torch.zeros_like(sd[k]) if offset_zero else sd[k] * offset_scale
    return sd


def dcn_block(sub: Dict[str, Tensor], x: Tensor, li: int, b: int) -> Tensor:
    """O.resnet_block with conv2 a DeformConv2dPack where the state dict holds its conv_offset"""
    p = f"layer{li + 1}.{b}"
    if p + ".conv2.conv_offset.weight" not in sub:
        return O.resnet_block(sub, x, li, b)
    stride = 2 if (b == 0 and li > 0) else 1
    identity = x
    out = F.relu(O._bn_eval(F.conv2d(x, sub[p + ".conv1.weight"]), sub, p + ".bn1"))
    out = dcn_conv2_nchw(out, sub[p + ".conv2.weight"], sub[p + ".conv2.conv_offset.weight"], sub[p + ".conv2.conv_offset.bias"], stride)
    out = F.relu(O._bn_eval(out, sub, p + ".bn2"))
    out = O._bn_eval(F.conv2d(out, sub[p + ".conv3.weight"]), sub, p + ".bn3")
    if b == 0:
        identity = O._bn_eval(F.conv2d(x, sub[p + ".downsample.0.weight"], None, stride), sub, p + ".downsample.1")
    return F.relu(out + identity)


def dcn_resnet_forward(sd: Dict[str, Tensor], x: Tensor, depth: int = 50, prefix: str = "backbone.") -> List[Tensor]:
    """the four stage outputs of a ResNet whose state dict carries conv_offset parameters in its DCN blocks"""
    sub = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
    x = O.resnet_stem(sub, x)
    outs = []
    for li, nblk in enumerate(O.RESNET_BLOCKS[depth]):
        for b in range(nblk):
            x = dcn_block(sub, x, li, b)
        outs.append(x)
    return outs


def gfl_forward(sd, x, depth: int = 50):
    return O.gfl_head_forward(sd, O.fpn_forward(sd, dcn_resnet_forward(sd, x, depth)))


def erd_step_loss(teacher_sd, student_sd, x, gt_bboxes, gt_labels, metas, c_old, c_all, depth: int = 50, return_aux: bool = False):
    """O.erd_step_loss on DCN backbones: teacher forward, ERS, student forward, losses"""
    with torch.no_grad():
        t_cls, t_bbox = gfl_forward(teacher_sd, x, depth)
    s_cls, s_bbox = gfl_forward(student_sd, x, depth)
    return O.erd_head_loss(t_cls, t_bbox, s_cls, s_bbox, gt_bboxes, gt_labels, metas, c_old, c_all, 1.0, return_aux=return_aux)
