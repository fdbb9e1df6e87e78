# Stage 2 of ERD 40+40 with CIoULoss as the head's box loss: the box term is the one supervised signal that pulls the new classes'
# localisation away from the distilled old-class responses, and CIoU adds a centre-distance and an aspect-ratio penalty to it.
# Only `loss_bbox` is overridden (IoULoss and DIoULoss are accepted in the same slot); everything else is the base's.
_base_ = ['./gfl_r50_fpn_1x_coco_first_40_incre_last_40_cats.py']

model = dict(bbox_head=dict(loss_bbox=dict(_delete_=True, type='CIoULoss', loss_weight=2.0)))
