# Stage 1 of the 40+40 protocol on a ResNet-50 with deformable convolutions (DCNv1) in c3-c5.  Not a file of the reference (it ships
# the plain R50 pair only): the R50 first-40 config with the backbone block of the reference's
# configs/gfl/gfl_r101-dconv-c3-c5_fpn_ms-2x_coco.py at depth 50.  The ImageNet file has no conv_offset keys: they start at zero.
_base_ = './gfl_r50_fpn_1x_coco_first_40_cats.py'

model = dict(
    backbone=dict(
        type='ResNet', depth=50, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=1,
        norm_cfg=dict(type='BN', requires_grad=True),
        dcn=dict(type='DCN', deform_groups=1, fallback_on_stride=False), stage_with_dcn=(False, True, True, True),
        norm_eval=True, style='pytorch', init_cfg=dict(type='Pretrained', checkpoint='torchvision://resnet50')))
