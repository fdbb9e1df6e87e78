"""Host references of the grouped convolutions and of the ResNeXt backbone (test-only, CPU).

conv_g and its two gradients are torch's own grouped convolution in fp64; `resnext_forward` restates
mmdet/models/backbones/resnext.py (Bottleneck width rule :29-33, conv2 with groups :55-64) in the style of the oracle's
`resnet_block`, and composes with the oracle's FPN / head / loss restatements for whole-model checks."""
import math
from typing import Dict, List, Tuple

import torch
import torch.nn.functional as F

from oracle import erd_oracle as O

Tensor = torch.Tensor


# ----------------------------------------------------------------------------------------------------------------
# the three grouped launches, fp64.  Maps are NHWC, the weight is the parameter's layout [C, 3, 3, cg].
# ----------------------------------------------------------------------------------------------------------------
def _oihw(w_ohwi: Tensor) -> Tensor:
    return w_ohwi.permute(0, 3, 1, 2).double()


def _nchw(m: Tensor) -> Tensor:
    return m.permute(0, 3, 1, 2).double()


def conv_g(x: Tensor, w: Tensor, stride: int, cardinality: int) -> Tensor:
    """conv_g(x, w): [N, OH, OW, C] fp64"""
    return F.conv2d(_nchw(x), _oihw(w), None, stride, 1, 1, cardinality).permute(0, 2, 3, 1).contiguous()


def conv_g_abs(x: Tensor, w: Tensor, stride: int, cardinality: int) -> Tensor:
    """sum |a| |b| of every output's products (the magnitude an rounding-error bound scales with)"""
    return conv_g(x.abs(), w.abs(), stride, cardinality)


def conv_g_dgrad(dz: Tensor, w: Tensor, in_hw: Tuple[int, int], stride: int, cardinality: int) -> Tensor:
    """conv_g^T(dz, w): the gradient of conv_g with respect to its input of extent in_hw, [N, IH, IW, C] fp64"""
    N, _, _, C = dz.shape
    g = torch.nn.grad.conv2d_input((N, C, in_hw[0], in_hw[1]), _oihw(w), _nchw(dz), stride, 1, 1, cardinality)
    return g.permute(0, 2, 3, 1).contiguous()


def conv_g_wgrad(x: Tensor, dz: Tensor, stride: int, cardinality: int) -> Tensor:
    """the weight gradient in the parameter's layout [C, 3, 3, cg], fp64"""
    C = x.shape[3]
    g = torch.nn.grad.conv2d_weight(_nchw(x), (C, C // cardinality, 3, 3), _nchw(dz), stride, 1, 1, cardinality)
    return g.permute(0, 2, 3, 1).contiguous()


# ----------------------------------------------------------------------------------------------------------------
# ResNeXt
# ----------------------------------------------------------------------------------------------------------------
def resnext_width(planes: int, groups: int, base_width: int) -> int:
    """resnext.py:29-33"""
    return planes if groups == 1 else math.floor(planes * (base_width / 64)) * groups


def resnext_param_shapes(depth: int, groups: int, base_width: int) -> Dict[str, Tuple[int, ...]]:
    """state-dict keys / shapes of a ResNeXt backbone: the ResNet's with conv1 / conv2 / conv3 at the ResNeXt width"""
    s = dict(O.resnet_param_shapes(depth))
    inplanes = 64
    for li, nblk in enumerate(O.RESNET_BLOCKS[depth]):
        planes = 64 * 2 ** li
        w = resnext_width(planes, groups, base_width)
        for b in range(nblk):
            p = f"layer{li + 1}.{b}"
            s[p + ".conv1.weight"] = (w, inplanes, 1, 1)
            s[p + ".conv2.weight"] = (w, w // groups, 3, 3)
            s[p + ".conv3.weight"] = (planes * 4, w, 1, 1)
            for bn in (".bn1", ".bn2"):
                for leaf in (".weight", ".bias", ".running_mean", ".running_var"):
                    s[p + bn + leaf] = (w,)
            inplanes = planes * 4
    return s


def resnext_gfl_state_dict(num_classes: int, depth: int, groups: int, base_width: int, seed: int = 0) -> Dict[str, Tensor]:
    """procedural weights (the oracle's spec, O.procedural_tensor) of a GFL detector on a ResNeXt backbone"""
    shapes = O.gfl_param_shapes(num_classes, depth)
    shapes.update({"backbone." + k: v for k, v in resnext_param_shapes(depth, groups, base_width).items()})
    return {k: O.procedural_tensor(seed, k, shp) for k, shp in shapes.items()}


def resnext_block(sub: Dict[str, Tensor], x: Tensor, li: int, b: int, groups: int) -> Tensor:
    """resnext.py Bottleneck (forward inherited from resnet.py:263-302): O.resnet_block with conv2 in `groups` groups"""
    p = f"layer{li + 1}.{b}"
    stride = 2 if (b == 0 and li > 0) else 1
    identity = x
    out = F.relu(O._bn_eval(F.conv2d(x, sub[p + ".conv1.weight"]), sub, p + ".bn1"))
    out = F.relu(O._bn_eval(F.conv2d(out, sub[p + ".conv2.weight"], None, stride, 1, 1, groups), sub, p + ".bn2"))
    out = O._bn_eval(F.conv2d(out, sub[p + ".conv3.weight"]), sub, p + ".bn3")
    if b == 0:
        identity = O._bn_eval(F.conv2d(x, sub[p + ".downsample.0.weight"], None, stride), sub, p + ".downsample.1")
    return F.relu(out + identity)


def resnext_forward(sd: Dict[str, Tensor], x: Tensor, depth: int, groups: int, base_width: int, prefix: str = "backbone.") -> List[Tensor]:
    """the four stage outputs (resnet.py:631-646 with resnext.py's blocks); base_width only fixes the shapes `sd` must have"""
    sub = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
    want = resnext_param_shapes(depth, groups, base_width)
    assert all(tuple(sub[k].shape) == tuple(v) for k, v in want.items()), "state dict is not this ResNeXt's"
    x = O.resnet_stem(sub, x)
    outs = []
    for li, nblk in enumerate(O.RESNET_BLOCKS[depth]):
        for b in range(nblk):
            x = resnext_block(sub, x, li, b, groups)
        outs.append(x)
    return outs


def gfl_forward(sd, x, depth, groups, base_width):
    return O.gfl_head_forward(sd, O.fpn_forward(sd, resnext_forward(sd, x, depth, groups, base_width)))


def erd_step_loss(teacher_sd, student_sd, x, gt_bboxes, gt_labels, metas, c_old, c_all, depth, groups, base_width, return_aux=False):
    """O.erd_step_loss on ResNeXt backbones: teacher forward, ERS, student forward, losses"""
    with torch.no_grad():
        t_cls, t_bbox = gfl_forward(teacher_sd, x, depth, groups, base_width)
    s_cls, s_bbox = gfl_forward(student_sd, x, depth, groups, base_width)
    return O.erd_head_loss(t_cls, t_bbox, s_cls, s_bbox, gt_bboxes, gt_labels, metas, c_old, c_all, 1.0, return_aux=return_aux)


def stage_loss_weights(outs: List[Tensor], seed: int = 5) -> List[Tensor]:
    """fixed weights of the weighted-sum loss the backbone pins differentiate: sum_i <w_i, out_i> / numel_i"""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(o.shape, generator=g) / o.numel() for o in outs]
