# Stage 2 of the 40+40 protocol on a ResNeXt-101 32x4d backbone: an 80-class student learns the last 40 categories; ERD distils the
# 40 old-class responses of the frozen stage-1 teacher.  Derived from the R50 40+40 config; not a file of the reference.
_base_ = './gfl_r50_fpn_1x_coco_first_40_incre_last_40_cats.py'

model = dict(
    ori_setting=dict(
        ori_checkpoint_file='../ERD_results/gfl_increment/gfl_x101_32x4d_fpn_1x_coco_first_40_cats/epoch_12.pth',
        ori_config_file='configs/gfl_increment/gfl_x101_32x4d_fpn_1x_coco_first_40_cats.py'),
    backbone=dict(
        type='ResNeXt', depth=101, groups=32, base_width=4, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=1,
        norm_cfg=dict(type='BN', requires_grad=True), norm_eval=True, style='pytorch',
        init_cfg=dict(type='Pretrained', checkpoint='open-mmlab://resnext101_32x4d')))
