# Stage 2 of ERD 40+40 with multi-scale training: every image draws its own target scale, long edge 1333 and short edge
# anywhere in 480..800 (mmdet's "ms" recipe), aspect ratio kept; the batch is padded to its largest image.  Only the
# train pipeline differs from the base; testing stays at (1333, 800) and the schedule stays 1x.  (mmdet pairs the recipe
# with 24 epochs, milestones 16 and 22: a child config sets `train_cfg.max_epochs` and the MultiStepLR entry for that.)
_base_ = './gfl_r50_fpn_1x_coco_first_40_incre_last_40_cats.py'

train_pipeline = [
    dict(type='LoadImageFromFile', backend_args=None),
    dict(type='LoadAnnotations', with_bbox=True),
    dict(type='RandomResize', scale=[(1333, 480), (1333, 800)], keep_ratio=True),
    dict(type='RandomFlip', prob=0.5),
    dict(type='PackDetInputs'),
]
train_dataloader = dict(dataset=dict(pipeline=train_pipeline))
