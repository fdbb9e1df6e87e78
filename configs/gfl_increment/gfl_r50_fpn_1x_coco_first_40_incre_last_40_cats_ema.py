# Stage 2 of ERD 40+40 with an averaged student: mmengine's EMAHook keeps an exponential moving average of the trainable weights
# (mmdet's ExpMomentumEMA: a large coefficient early, annealed towards `momentum`).  Validation scores the average, checkpoints
# hold it in `state_dict` (the raw training weights travel in `ema_state_dict`), so tools/test.py and the next phase's
# `ori_setting.ori_checkpoint_file` read the averaged detector with no change.
_base_ = ['./gfl_r50_fpn_1x_coco_first_40_incre_last_40_cats.py']

custom_hooks = [dict(type='EMAHook', ema_type='ExpMomentumEMA', momentum=0.0002, update_buffers=True, priority=49)]
