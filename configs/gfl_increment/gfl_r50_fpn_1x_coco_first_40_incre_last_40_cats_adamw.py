# Stage 2 of ERD 40+40 under AdamW: the adaptive update with decoupled weight decay that mmdet recipes pair with a slower
# backbone -- a gentler step on the old weights is the first thing to try against forgetting.  The optimizer REPLACES the base's
# SGD dict (`_delete_`: no `momentum` is left behind); normalisation parameters are not decayed and the gradient is clipped.
_base_ = ['./gfl_r50_fpn_1x_coco_first_40_incre_last_40_cats.py']

optim_wrapper = dict(
    optimizer=dict(_delete_=True, type='AdamW', lr=1e-4,
                   betas=(0.9, 0.999), weight_decay=0.05),
    paramwise_cfg=dict(norm_decay_mult=0.,
                       custom_keys={'backbone': dict(lr_mult=0.1)}),
    clip_grad=dict(max_norm=35, norm_type=2))
