# Stage 1 of the 40+40 protocol on a ResNeXt-101 32x4d backbone.  Not a file of the reference (it ships the R50 pair only):
# the R50 first-40 config with the backbone of the reference's configs/gfl/gfl_x101-32x4d_fpn_ms-2x_coco.py.
_base_ = './gfl_r50_fpn_1x_coco_first_40_cats.py'

model = dict(
    backbone=dict(
        type='ResNeXt', depth=101, groups=32, base_width=4, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=1,
        norm_cfg=dict(type='BN', requires_grad=True), norm_eval=True, style='pytorch',
        init_cfg=dict(type='Pretrained', checkpoint='open-mmlab://resnext101_32x4d')))
