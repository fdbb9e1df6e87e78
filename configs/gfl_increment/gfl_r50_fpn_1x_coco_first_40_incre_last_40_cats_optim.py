# Stage 2 of ERD 40+40 with the optimizer wrapper's options: a slower backbone (the forgetting-vs-plasticity knob), no weight
# decay on normalisation parameters and biases, gradient clipping, and 4 micro-steps per update so that one GPU at batch 4
# trains at the batch 16 the schedule was written for.
_base_ = ['./gfl_r50_fpn_1x_coco_first_40_incre_last_40_cats.py']

optim_wrapper = dict(
    paramwise_cfg=dict(
        norm_decay_mult=0.,
        bias_lr_mult=2.,
        bias_decay_mult=0.,
        custom_keys={
            'backbone': dict(lr_mult=0.1),
            'backbone.layer4': dict(lr_mult=0.5, decay_mult=2.)}),
    clip_grad=dict(max_norm=35, norm_type=2),
    accumulative_counts=4)
