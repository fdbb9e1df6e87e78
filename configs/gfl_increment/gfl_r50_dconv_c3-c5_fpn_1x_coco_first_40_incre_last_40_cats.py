# Stage 2 of the 40+40 protocol on a ResNet-50 with deformable convolutions (DCNv1) in c3-c5: an 80-class student learns the last 40
# categories; ERD distils the 40 old-class responses of the frozen stage-1 teacher.  Derived from the R50 40+40 config; not a file of
# the reference.  Stage 1 has no DCN block, so student and teacher still share the frozen trunk.
_base_ = './gfl_r50_fpn_1x_coco_first_40_incre_last_40_cats.py'

model = dict(
    ori_setting=dict(
        ori_checkpoint_file='../ERD_results/gfl_increment/gfl_r50_dconv_c3-c5_fpn_1x_coco_first_40_cats/epoch_12.pth',
        ori_config_file='configs/gfl_increment/gfl_r50_dconv_c3-c5_fpn_1x_coco_first_40_cats.py'),
    backbone=dict(
        type='ResNet', depth=50, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=1,
        norm_cfg=dict(type='BN', requires_grad=True),
        dcn=dict(type='DCN', deform_groups=1, fallback_on_stride=False), stage_with_dcn=(False, True, True, True),
        norm_eval=True, style='pytorch', init_cfg=dict(type='Pretrained', checkpoint='torchvision://resnet50')))
