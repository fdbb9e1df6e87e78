# Phase 3 of the 40+10x4 protocol: a 60-class R50 student learns categories [50, 60); ERD distils the 50 old-class
# responses of the frozen phase-2 model (gfl_r50_fpn_1x_coco_40_10x4_phase2_40_50_cats.py), whose checkpoint includes its own teacher copy (dropped at load).
# Our own chain config, derived from the 40+40 stage-2 config; not a file of the reference.
_base_ = './gfl_r50_fpn_1x_coco_first_40_incre_last_40_cats.py'

data_root = '../data/coco/'

model = dict(
    ori_setting=dict(
        ori_checkpoint_file='../ERD_results/gfl_increment/gfl_r50_fpn_1x_coco_40_10x4_phase2_40_50_cats/epoch_12.pth',
        ori_num_classes=50,
        ori_config_file='configs/gfl_increment/gfl_r50_fpn_1x_coco_40_10x4_phase2_40_50_cats.py'),
    bbox_head=dict(num_classes=60))

train_dataloader = dict(dataset=dict(ann_file='annotations/instances_train2017_cats_50_60.json'))
val_dataloader = dict(dataset=dict(ann_file='annotations/instances_val2017_cats_0_60.json'))
val_evaluator = dict(ann_file=data_root + 'annotations/instances_val2017_cats_0_60.json')
test_dataloader = val_dataloader
test_evaluator = val_evaluator
