"""BEVFormer detector -- the 3D-detection fine-tune target of a ViDAR checkpoint: training-step orchestration and the
video-mode inference of projects/mmdet3d_plugin/bevformer/detectors/bevformer.py:20-347 (constructor protocol of
mmdet3d's MVXTwoStageDetector, third party, recalled, unpinned: `train_cfg.pts` / `test_cfg.pts` go to pts_bbox_head).

History BEV, image branch and the SpatialCrossAttention plan are the ViDAR detector's (same code: frozen history frames,
optionally back-propagated last ones, one camera-projection plan per step).  As there, `img_feats` (list over levels of
[bs, T, cams, C, h, w]) may replace `img` when no backbone is built."""
from __future__ import annotations

import copy

import torch
import torch.nn as nn

from ..core_bbox import bbox3d2result
from ..registry import BACKBONES, DETECTORS, NECKS, build_head
from .vidar import ViDAR


@DETECTORS.register_module()
class BEVFormer(nn.Module):
    def __init__(self, use_grid_mask=False, pts_voxel_layer=None, pts_voxel_encoder=None, pts_middle_encoder=None,
                 pts_fusion_layer=None, img_backbone=None, pts_backbone=None, img_neck=None, pts_neck=None,
                 pts_bbox_head=None, img_roi_head=None, img_rpn_head=None, train_cfg=None, test_cfg=None, pretrained=None,
                 video_test_mode=False, backwarded_prev_frame_num=0):
        super().__init__()
        for name, v in dict(pts_voxel_layer=pts_voxel_layer, pts_voxel_encoder=pts_voxel_encoder,
                            pts_middle_encoder=pts_middle_encoder, pts_fusion_layer=pts_fusion_layer,
                            pts_backbone=pts_backbone, pts_neck=pts_neck, img_roi_head=img_roi_head,
                            img_rpn_head=img_rpn_head).items():
            if v is not None:
                raise NotImplementedError(f"BEVFormer: {name}")
        self.img_backbone = BACKBONES.build(img_backbone) if (
            img_backbone and img_backbone.get("type") in BACKBONES) else None
        self.img_neck = NECKS.build(img_neck) if (img_neck and img_neck.get("type") in NECKS) else None
        head = dict(pts_bbox_head)
        head.update(train_cfg=(train_cfg or {}).get("pts"), test_cfg=(test_cfg or {}).get("pts"))
        self.pts_bbox_head = build_head(head)
        from ..utils.grid_mask import GridMask
        self.grid_mask = GridMask(True, True, rotate=1, offset=False, ratio=0.5, mode=1, prob=0.7)
        self.use_grid_mask = use_grid_mask
        self.grid_mask_image, self.grid_mask_backbone_feat, self.grid_mask_fpn_feat = True, False, False
        self.fp16_enabled = False
        self.video_test_mode = video_test_mode
        self.prev_frame_info = dict(prev_bev=None, scene_token=None, prev_pos=0, prev_angle=0)
        self.backwarded_prev_frame_num = backwarded_prev_frame_num
        self.bev_h, self.bev_w = self.pts_bbox_head.bev_h, self.pts_bbox_head.bev_w
        self.train_cfg, self.test_cfg = train_cfg, test_cfg

    def init_weights(self):
        self.pts_bbox_head.init_weights()

    # image branch, history BEV and the per-step camera plan: shared with the ViDAR detector
    extract_feat = ViDAR.extract_feat
    _queue_feats = ViDAR._queue_feats
    obtain_history_bev = ViDAR.obtain_history_bev
    _plan_sca = ViDAR._plan_sca

    def forward_pts_train(self, pts_feats, gt_bboxes_3d, gt_labels_3d, img_metas, gt_bboxes_ignore=None, prev_bev=None):
        outs = self.pts_bbox_head(pts_feats, img_metas, prev_bev)
        return self.pts_bbox_head.loss(gt_bboxes_3d, gt_labels_3d, outs, img_metas=img_metas)

    def forward_train(self, points=None, img_metas=None, gt_bboxes_3d=None, gt_labels_3d=None, gt_labels=None,
                      gt_bboxes=None, img=None, proposals=None, gt_bboxes_ignore=None, img_depth=None, img_mask=None,
                      img_feats=None):
        """bevformer.py:235-289: history BEV over frames [0, T-1) -> current frame -> head -> losses"""
        num_frames = img.size(1) if img is not None else img_feats[0].size(1)
        self._plan_sca(img_metas, num_frames, (img if img is not None else img_feats[0]).device)
        prev_img_metas = copy.deepcopy(img_metas)
        prev_bev = self.obtain_history_bev(img, prev_img_metas, img_feats, num_frames - 1)
        cur_metas = [m[num_frames - 1] for m in img_metas]
        if not cur_metas[0]["prev_bev_exists"]:
            prev_bev = None
        cur_feats = [f[:, 0] for f in self._queue_feats(img, img_feats, img_metas, num_frames - 1, num_frames, grad=True)]
        return dict(self.forward_pts_train(cur_feats, gt_bboxes_3d, gt_labels_3d, cur_metas, gt_bboxes_ignore, prev_bev))

    @torch.no_grad()
    def forward_test(self, img_metas, img=None, img_feats=None, **kwargs):
        """bevformer.py:291-324: one frame per call; `prev_frame_info` carries the BEV features and the ego pose of the
        previous call, reset at a scene change.  img_metas: [[dict per sample]], img: [tensor [bs, cams, 3, H, W]]
        (or img_feats: [list over levels of [bs, cams, C, h, w]])."""
        if not isinstance(img_metas, list):
            raise TypeError(f"img_metas must be a list, but got {type(img_metas)}")
        img = [img] if img is None else img
        info = self.prev_frame_info
        if img_metas[0][0]["scene_token"] != info["scene_token"]:
            info["prev_bev"] = None                                   # the first sample of each scene is truncated
        info["scene_token"] = img_metas[0][0]["scene_token"]
        if not self.video_test_mode:
            info["prev_bev"] = None
        tmp_pos = copy.deepcopy(img_metas[0][0]["can_bus"][:3])
        tmp_angle = copy.deepcopy(img_metas[0][0]["can_bus"][-1])
        if info["prev_bev"] is not None:
            img_metas[0][0]["can_bus"][:3] -= info["prev_pos"]
            img_metas[0][0]["can_bus"][-1] -= info["prev_angle"]
        else:
            img_metas[0][0]["can_bus"][-1] = 0
            img_metas[0][0]["can_bus"][:3] = 0
        new_prev_bev, bbox_results = self.simple_test(img_metas[0], img[0], prev_bev=info["prev_bev"],
                                                      img_feats=None if img_feats is None else img_feats[0], **kwargs)
        info["prev_pos"], info["prev_angle"], info["prev_bev"] = tmp_pos, tmp_angle, new_prev_bev
        return bbox_results

    def simple_test_pts(self, x, img_metas, prev_bev=None, rescale=False):
        outs = self.pts_bbox_head(x, img_metas, prev_bev=prev_bev)
        bbox_list = self.pts_bbox_head.get_bboxes(outs, img_metas, rescale=rescale)
        return outs["bev_embed"], [bbox3d2result(b, s, l) for b, s, l in bbox_list]

    def simple_test(self, img_metas, img=None, prev_bev=None, rescale=False, img_feats=None):
        if img_feats is None:
            img_feats = self.extract_feat(img, img_metas)
        new_prev_bev, bbox_pts = self.simple_test_pts(img_feats, img_metas, prev_bev, rescale=rescale)
        return new_prev_bev, [dict(pts_bbox=b) for b in bbox_pts]

    def forward(self, return_loss=True, **kwargs):
        if return_loss:
            return self.forward_train(**kwargs)
        return self.forward_test(**kwargs)
