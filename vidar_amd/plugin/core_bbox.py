"""Box code, coder, matching costs and assigner of the BEVFormer detection head.

Restated from the reference's own files:
  * normalize_bbox / denormalize_bbox -- projects/mmdet3d_plugin/core/bbox/util.py:4-53
  * NMSFreeCoder                      -- core/bbox/coders/nms_free_coder.py:9-121
  * BBox3DL1Cost                      -- core/bbox/match_costs/match_cost.py:6-28
  * HungarianAssigner3D               -- core/bbox/assigners/hungarian_assigner_3d.py:17-136
Third party, recalled, unpinned (mmdet / mmdet3d are not vendored in the reference):
  * FocalLossCost (mmdet.core.bbox.match_costs, eps 1e-12, sigmoid form), IoUCost (accepted with weight 0 only),
  * AssignResult / PseudoSampler semantics (positives = queries with a 1-based gt index > 0),
  * LiDARInstance3DBoxes (mmdet3d): `tensor [G, 7|9]` with a BOTTOM-centred z (`origin` names where the given centre
    sits inside the box, (0.5, 0.5, 0.5) = gravity centre), `gravity_center` lifts z by half the height, `to(device)`,
    `__len__`;  bbox3d2result: dict(boxes_3d, scores_3d, labels_3d) on the CPU."""
from __future__ import annotations

import torch

from .registry import Registry

BBOX_CODERS = Registry("bbox coder")
BBOX_ASSIGNERS = Registry("bbox assigner")
MATCH_COST = Registry("match cost")


def build_bbox_coder(cfg, **kw): return BBOX_CODERS.build(cfg, **kw)
def build_assigner(cfg, **kw): return BBOX_ASSIGNERS.build(cfg, **kw)
def build_match_cost(cfg, **kw): return MATCH_COST.build(cfg, **kw)


def normalize_bbox(bboxes, pc_range=None):
    cx, cy, cz = bboxes[..., 0:1], bboxes[..., 1:2], bboxes[..., 2:3]
    w, l, h = bboxes[..., 3:4].log(), bboxes[..., 4:5].log(), bboxes[..., 5:6].log()
    rot = bboxes[..., 6:7]
    parts = (cx, cy, w, l, cz, h, rot.sin(), rot.cos())
    if bboxes.size(-1) > 7:
        parts = parts + (bboxes[..., 7:8], bboxes[..., 8:9])
    return torch.cat(parts, dim=-1)


def denormalize_bbox(normalized_bboxes, pc_range=None):
    rot = torch.atan2(normalized_bboxes[..., 6:7], normalized_bboxes[..., 7:8])
    cx, cy, cz = normalized_bboxes[..., 0:1], normalized_bboxes[..., 1:2], normalized_bboxes[..., 4:5]
    w, l, h = normalized_bboxes[..., 2:3].exp(), normalized_bboxes[..., 3:4].exp(), normalized_bboxes[..., 5:6].exp()
    if normalized_bboxes.size(-1) > 8:
        return torch.cat([cx, cy, cz, w, l, h, rot, normalized_bboxes[:, 8:9], normalized_bboxes[:, 9:10]], dim=-1)
    return torch.cat([cx, cy, cz, w, l, h, rot], dim=-1)


class LiDARInstance3DBoxes:
    def __init__(self, tensor, box_dim=None, with_yaw=True, origin=(0.5, 0.5, 0)):
        tensor = torch.as_tensor(tensor, dtype=torch.float32)
        if tensor.numel() == 0:
            tensor = tensor.reshape((0, box_dim or (tensor.size(-1) if tensor.dim() == 2 else 7)))
        assert tensor.dim() == 2 and tensor.size(-1) in (7, 9) and len(origin) == 3
        if tuple(origin) != (0.5, 0.5, 0):          # another reference point of the centre: move it to the bottom face
            tensor = tensor.clone()
            tensor[:, :3] += tensor[:, 3:6] * (tensor.new_tensor((0.5, 0.5, 0)) - tensor.new_tensor(origin))
        self.tensor = tensor
        self.box_dim = tensor.size(-1)

    @property
    def gravity_center(self):
        c = self.tensor[:, :3].clone()
        c[:, 2] = c[:, 2] + self.tensor[:, 5] * 0.5
        return c

    def to(self, device):
        return LiDARInstance3DBoxes(self.tensor.to(device), box_dim=self.box_dim)

    def __len__(self):
        return self.tensor.shape[0]


def bbox3d2result(bboxes, scores, labels):
    return dict(boxes_3d=bboxes.to("cpu"), scores_3d=scores.cpu(), labels_3d=labels.cpu())


@BBOX_CODERS.register_module()
class NMSFreeCoder:
    def __init__(self, pc_range, voxel_size=None, post_center_range=None, max_num=100, score_threshold=None,
                 num_classes=10):
        self.pc_range = pc_range
        self.voxel_size = voxel_size
        self.post_center_range = post_center_range
        self.max_num = max_num
        self.score_threshold = score_threshold
        self.num_classes = num_classes

    def decode_single(self, cls_scores, bbox_preds):
        """top-`max_num` (query, class) scores -> boxes inside post_center_range (nms_free_coder.py:40-100)"""
        cls_scores = cls_scores.sigmoid()
        scores, indexs = cls_scores.view(-1).topk(min(self.max_num, cls_scores.numel()))
        labels = indexs % self.num_classes
        bbox_index = torch.div(indexs, self.num_classes, rounding_mode="floor")
        final_box_preds = denormalize_bbox(bbox_preds[bbox_index], self.pc_range)
        if self.score_threshold is not None:
            thresh_mask = scores > self.score_threshold
            tmp_score = self.score_threshold
            while thresh_mask.sum() == 0:
                tmp_score *= 0.9
                if tmp_score < 0.01:
                    thresh_mask = scores > -1
                    break
                thresh_mask = scores >= tmp_score
        if self.post_center_range is None:
            raise NotImplementedError("NMSFreeCoder: post_center_range=None")
        rng = torch.as_tensor(self.post_center_range, device=scores.device, dtype=final_box_preds.dtype)
        mask = (final_box_preds[..., :3] >= rng[:3]).all(1)
        mask &= (final_box_preds[..., :3] <= rng[3:]).all(1)
        if self.score_threshold:
            mask &= thresh_mask
        return dict(bboxes=final_box_preds[mask], scores=scores[mask], labels=labels[mask])

    def decode(self, preds_dicts):
        all_cls_scores = preds_dicts["all_cls_scores"][-1]
        all_bbox_preds = preds_dicts["all_bbox_preds"][-1]
        return [self.decode_single(all_cls_scores[i], all_bbox_preds[i]) for i in range(all_cls_scores.size(0))]


@MATCH_COST.register_module()
class BBox3DL1Cost:
    def __init__(self, weight=1.):
        self.weight = weight

    def __call__(self, bbox_pred, gt_bboxes):
        return torch.cdist(bbox_pred, gt_bboxes, p=1) * self.weight


@MATCH_COST.register_module()
class FocalLossCost:
    def __init__(self, weight=1., alpha=0.25, gamma=2, eps=1e-12, binary_input=False):
        if binary_input:
            raise NotImplementedError("FocalLossCost: binary_input")
        self.weight, self.alpha, self.gamma, self.eps = weight, alpha, gamma, eps

    def __call__(self, cls_pred, gt_labels):
        cls_pred = cls_pred.sigmoid()
        neg_cost = -(1 - cls_pred + self.eps).log() * (1 - self.alpha) * cls_pred.pow(self.gamma)
        pos_cost = -(cls_pred + self.eps).log() * self.alpha * (1 - cls_pred).pow(self.gamma)
        return (pos_cost[:, gt_labels] - neg_cost[:, gt_labels]) * self.weight


@MATCH_COST.register_module()
class IoUCost:
    """The released configs carry `iou_cost=dict(type='IoUCost', weight=0.0)` as a placeholder ("Fake cost"); the 3D
    assigner never evaluates it."""

    def __init__(self, iou_mode="giou", weight=1.):
        if weight != 0:
            raise NotImplementedError("IoUCost with a non-zero weight")
        self.weight = weight


class AssignResult:
    def __init__(self, num_gts, gt_inds, max_overlaps, labels=None):
        self.num_gts, self.gt_inds, self.max_overlaps, self.labels = num_gts, gt_inds, max_overlaps, labels


@BBOX_ASSIGNERS.register_module()
class HungarianAssigner3D:
    def __init__(self, cls_cost=dict(type="ClassificationCost", weight=1.), reg_cost=dict(type="BBoxL1Cost", weight=1.0),
                 iou_cost=dict(type="IoUCost", weight=0.0), pc_range=None):
        self.cls_cost = build_match_cost(cls_cost)
        self.reg_cost = build_match_cost(reg_cost)
        self.iou_cost = build_match_cost(iou_cost)
        self.pc_range = pc_range

    def cost(self, bbox_pred, cls_pred, gt_bboxes, gt_labels):
        """[num_query, num_gt] (hungarian_assigner_3d.py:106-116)"""
        normalized_gt_bboxes = normalize_bbox(gt_bboxes, self.pc_range)
        return self.cls_cost(cls_pred, gt_labels) + self.reg_cost(bbox_pred[:, :8], normalized_gt_bboxes[:, :8])

    def assign(self, bbox_pred, cls_pred, gt_bboxes, gt_labels, gt_bboxes_ignore=None, eps=1e-7):
        """one query set against one sample's ground truth; the cost matrix goes to the host with a blocking copy, as in
        the reference (:119-123)"""
        from scipy.optimize import linear_sum_assignment
        assert gt_bboxes_ignore is None, "Only case when gt_bboxes_ignore is None is supported."
        num_gts, num_bboxes = gt_bboxes.size(0), bbox_pred.size(0)
        assigned_gt_inds = bbox_pred.new_full((num_bboxes,), -1, dtype=torch.long)
        assigned_labels = bbox_pred.new_full((num_bboxes,), -1, dtype=torch.long)
        if num_gts == 0 or num_bboxes == 0:
            if num_gts == 0:
                assigned_gt_inds[:] = 0
            return AssignResult(num_gts, assigned_gt_inds, None, labels=assigned_labels)
        cost = self.cost(bbox_pred, cls_pred, gt_bboxes, gt_labels).detach().cpu()
        rows, cols = linear_sum_assignment(cost)
        rows = torch.from_numpy(rows).to(bbox_pred.device)
        cols = torch.from_numpy(cols).to(bbox_pred.device)
        assigned_gt_inds[:] = 0
        assigned_gt_inds[rows] = cols + 1
        assigned_labels[rows] = gt_labels[cols]
        return AssignResult(num_gts, assigned_gt_inds, None, labels=assigned_labels)
