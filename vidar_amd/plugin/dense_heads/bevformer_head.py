"""BEVFormerHead -- registry name, constructor arguments, parameter names and semantics of
projects/mmdet3d_plugin/bevformer/dense_heads/bevformer_head.py:16-509 on top of mmdet's DETRHead constructor protocol
(third party, recalled, unpinned: num_classes / in_channels / num_query / num_reg_fcs / sync_cls_avg_factor /
loss_cls / loss_bbox / loss_iou / train_cfg['assigner'], bg_cls_weight 0 for a sigmoid focal loss, PseudoSampler).

What changed is the execution plan of the loss, not the math.  On CUDA tensors `loss` packs the ground truth of the batch
once, builds the Hungarian cost matrices of all decoder layers and samples with one kernel, reads them with ONE host
copy, and evaluates focal + L1 losses of all layers with one kernel each way (dense_heads/det_ops.py, csrc/det_loss.hip).
With det_ops.set_assign("device") / VIDAR_DET_ASSIGN=device (off by default) the assignment runs on the device too
(csrc/det_assign.hip) and that host copy goes: `last_assign_status` keeps the launch's status for whoever reads the loss.
With VIDAR_DET_LOSS=torch, or on CPU tensors, the reference's own structure runs: loss_single per decoder layer,
HungarianAssigner3D.assign per (layer, sample) with its blocking copy, FocalLoss and L1Loss modules."""
from __future__ import annotations

import copy

import numpy as np
import torch
import torch.distributed as dist
import torch.nn as nn

from ..bricks import Linear
from ..core_bbox import LiDARInstance3DBoxes, build_assigner, build_bbox_coder, normalize_bbox
from ..det_losses import bias_init_with_prob, build_loss
from ..modules.decoder import inverse_sigmoid
from ..registry import HEADS, build_positional_encoding, build_transformer
from ..utils.host import to_device_async
from . import det_ops


def reduce_mean(tensor):
    """mmdet.core.reduce_mean: the mean over ranks, on the device, never read back here"""
    if not (dist.is_available() and dist.is_initialized()):
        return tensor
    tensor = tensor.clone()
    dist.all_reduce(tensor.div_(dist.get_world_size()), op=dist.ReduceOp.SUM)
    return tensor


@HEADS.register_module()
class BEVFormerHead(nn.Module):
    def __init__(self, num_classes, in_channels, num_query=100, num_reg_fcs=2, transformer=None,
                 sync_cls_avg_factor=False, positional_encoding=None,
                 loss_cls=dict(type="FocalLoss", use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=2.0),
                 loss_bbox=dict(type="L1Loss", loss_weight=0.25), loss_iou=dict(type="GIoULoss", loss_weight=0.0),
                 train_cfg=None, test_cfg=None, init_cfg=None, with_box_refine=False, as_two_stage=False,
                 bbox_coder=None, num_cls_fcs=2, code_weights=None, bev_h=30, bev_w=30, code_size=10, **kwargs):
        super().__init__()
        if as_two_stage:
            raise NotImplementedError("BEVFormerHead: as_two_stage=True")
        if code_size != 10:
            raise NotImplementedError(f"BEVFormerHead: code_size={code_size} (10 only)")
        if kwargs:
            raise NotImplementedError(f"BEVFormerHead: unsupported options {sorted(kwargs)}")
        self.bev_h, self.bev_w = bev_h, bev_w
        self.fp16_enabled = False
        self.with_box_refine = with_box_refine
        self.as_two_stage = as_two_stage
        self.code_size = code_size
        cw = code_weights if code_weights is not None else [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2]
        self.bbox_coder = build_bbox_coder(bbox_coder)
        self.pc_range = self.bbox_coder.pc_range
        self.real_w = self.pc_range[3] - self.pc_range[0]
        self.real_h = self.pc_range[4] - self.pc_range[1]
        self.num_cls_fcs = num_cls_fcs - 1
        # ---- DETRHead.__init__ ----
        self.bg_cls_weight = 0
        self.sync_cls_avg_factor = sync_cls_avg_factor
        if loss_cls.get("class_weight") is not None:
            raise NotImplementedError("BEVFormerHead: loss_cls.class_weight")
        self.assigner = None
        self.last_assign_status = None      # device assignment: status tensor of the most recent loss (det_ops.assign_device)
        if train_cfg:
            assert "assigner" in train_cfg, "assigner should be provided when train_cfg is set."
            assigner = train_cfg["assigner"]
            assert loss_cls["loss_weight"] == assigner["cls_cost"]["weight"], \
                "The classification weight for loss and matcher should be exactly the same."
            assert loss_bbox["loss_weight"] == assigner["reg_cost"]["weight"], \
                "The regression L1 weight for loss and matcher should be exactly the same."
            self.assigner = build_assigner(assigner)
        self.num_query = num_query
        self.num_classes = num_classes
        self.in_channels = in_channels
        self.num_reg_fcs = num_reg_fcs
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.loss_cls = build_loss(loss_cls)
        self.loss_bbox = build_loss(loss_bbox)
        self.loss_iou = build_loss(loss_iou)
        self.cls_out_channels = num_classes if self.loss_cls.use_sigmoid else num_classes + 1
        self.positional_encoding = build_positional_encoding(positional_encoding)
        transformer = copy.deepcopy(dict(transformer))
        transformer["build_decoder"] = True                      # the decoder exists only where this head asks for it
        self.transformer = build_transformer(transformer)
        self.embed_dims = self.transformer.embed_dims
        self._init_layers()
        self.code_weights = nn.Parameter(torch.tensor(cw, requires_grad=False), requires_grad=False)

    def _init_layers(self):
        """bevformer_head.py:69-107"""
        cls_branch = []
        for _ in range(self.num_reg_fcs):
            cls_branch += [Linear(self.embed_dims, self.embed_dims), nn.LayerNorm(self.embed_dims), nn.ReLU(inplace=True)]
        cls_branch.append(Linear(self.embed_dims, self.cls_out_channels))
        fc_cls = nn.Sequential(*cls_branch)
        reg_branch = []
        for _ in range(self.num_reg_fcs):
            reg_branch += [Linear(self.embed_dims, self.embed_dims), nn.ReLU()]
        reg_branch.append(Linear(self.embed_dims, self.code_size))
        reg_branch = nn.Sequential(*reg_branch)
        num_pred = self.transformer.decoder.num_layers
        if self.with_box_refine:
            self.cls_branches = nn.ModuleList([copy.deepcopy(fc_cls) for _ in range(num_pred)])
            self.reg_branches = nn.ModuleList([copy.deepcopy(reg_branch) for _ in range(num_pred)])
        else:
            self.cls_branches = nn.ModuleList([fc_cls for _ in range(num_pred)])
            self.reg_branches = nn.ModuleList([reg_branch for _ in range(num_pred)])
        self.bev_embedding = nn.Embedding(self.bev_h * self.bev_w, self.embed_dims)
        self.query_embedding = nn.Embedding(self.num_query, self.embed_dims * 2)

    def init_weights(self):
        self.transformer.init_weights()
        if self.loss_cls.use_sigmoid:
            bias_init = bias_init_with_prob(0.01)
            for m in self.cls_branches:
                nn.init.constant_(m[-1].bias, bias_init)

    def forward(self, mlvl_feats, img_metas, prev_bev=None, only_bev=False):
        """bevformer_head.py:118-213 -> BEV features [bs, H*W, C] (only_bev) or dict(bev_embed, all_cls_scores
        [nb_dec, bs, num_query, C], all_bbox_preds [nb_dec, bs, num_query, 10], enc_*)"""
        bs = mlvl_feats[0].shape[0]
        dtype = mlvl_feats[0].dtype
        object_query_embeds = self.query_embedding.weight.to(dtype)
        bev_queries = self.bev_embedding.weight.to(dtype)
        bev_mask = torch.zeros((bs, self.bev_h, self.bev_w), device=bev_queries.device).to(dtype)
        bev_pos = self.positional_encoding(bev_mask).to(dtype)
        grid_length = (self.real_h / self.bev_h, self.real_w / self.bev_w)
        if only_bev:
            return self.transformer.get_bev_features(mlvl_feats, bev_queries, self.bev_h, self.bev_w,
                                                     grid_length=grid_length, bev_pos=bev_pos, img_metas=img_metas,
                                                     prev_bev=prev_bev)
        bev_embed, hs, init_reference, inter_references = self.transformer(
            mlvl_feats, bev_queries, object_query_embeds, self.bev_h, self.bev_w, grid_length=grid_length,
            bev_pos=bev_pos, reg_branches=self.reg_branches if self.with_box_refine else None, cls_branches=None,
            img_metas=img_metas, prev_bev=prev_bev)
        hs = hs.permute(0, 2, 1, 3)
        r = self.pc_range
        outputs_classes, outputs_coords = [], []
        for lvl in range(hs.shape[0]):
            reference = inverse_sigmoid(init_reference if lvl == 0 else inter_references[lvl - 1])
            outputs_classes.append(self.cls_branches[lvl](hs[lvl]))
            tmp = self.reg_branches[lvl](hs[lvl])
            assert reference.shape[-1] == 3
            # out of place (the reference writes the slices in place): same values, no CopySlices nodes in the graph
            xy = (tmp[..., 0:2] + reference[..., 0:2]).sigmoid()
            z = (tmp[..., 4:5] + reference[..., 2:3]).sigmoid()
            outputs_coords.append(torch.cat((xy[..., 0:1] * (r[3] - r[0]) + r[0], xy[..., 1:2] * (r[4] - r[1]) + r[1],
                                             tmp[..., 2:4], z * (r[5] - r[2]) + r[2], tmp[..., 5:]), -1))
        return dict(bev_embed=bev_embed, all_cls_scores=torch.stack(outputs_classes),
                    all_bbox_preds=torch.stack(outputs_coords), enc_cls_scores=None, enc_bbox_preds=None)

    # ---- the reference's loss structure (CPU tensors, VIDAR_DET_LOSS=torch) ------------------------------------------
    def _get_target_single(self, cls_score, bbox_pred, gt_labels, gt_bboxes, gt_bboxes_ignore=None):
        """bevformer_head.py:215-272 (PseudoSampler: positives are the assigned queries)"""
        num_bboxes = bbox_pred.size(0)
        gt_c = gt_bboxes.shape[-1]
        assign_result = self.assigner.assign(bbox_pred, cls_score, gt_bboxes, gt_labels, gt_bboxes_ignore)
        pos_inds = torch.nonzero(assign_result.gt_inds > 0, as_tuple=False).squeeze(-1).unique()
        neg_inds = torch.nonzero(assign_result.gt_inds == 0, as_tuple=False).squeeze(-1).unique()
        pos_assigned_gt_inds = assign_result.gt_inds[pos_inds] - 1
        labels = gt_bboxes.new_full((num_bboxes,), self.num_classes, dtype=torch.long)
        labels[pos_inds] = gt_labels[pos_assigned_gt_inds]
        label_weights = gt_bboxes.new_ones(num_bboxes)
        bbox_targets = torch.zeros_like(bbox_pred)[..., :gt_c]
        bbox_weights = torch.zeros_like(bbox_pred)
        bbox_weights[pos_inds] = 1.0
        bbox_targets[pos_inds] = gt_bboxes[pos_assigned_gt_inds].reshape(-1, gt_c)
        return labels, label_weights, bbox_targets, bbox_weights, pos_inds, neg_inds

    def get_targets(self, cls_scores_list, bbox_preds_list, gt_bboxes_list, gt_labels_list, gt_bboxes_ignore_list=None):
        """bevformer_head.py:274-323"""
        assert gt_bboxes_ignore_list is None, "Only supports for gt_bboxes_ignore setting to None."
        res = [self._get_target_single(c, b, l, g) for c, b, l, g in
               zip(cls_scores_list, bbox_preds_list, gt_labels_list, gt_bboxes_list)]
        labels_list, label_weights_list, bbox_targets_list, bbox_weights_list, pos_inds_list, neg_inds_list = map(list, zip(*res))
        num_total_pos = sum(inds.numel() for inds in pos_inds_list)
        num_total_neg = sum(inds.numel() for inds in neg_inds_list)
        return labels_list, label_weights_list, bbox_targets_list, bbox_weights_list, num_total_pos, num_total_neg

    def loss_single(self, cls_scores, bbox_preds, gt_bboxes_list, gt_labels_list, gt_bboxes_ignore_list=None):
        """bevformer_head.py:325-393"""
        num_imgs = cls_scores.size(0)
        (labels_list, label_weights_list, bbox_targets_list, bbox_weights_list, num_total_pos, num_total_neg) = \
            self.get_targets([cls_scores[i] for i in range(num_imgs)], [bbox_preds[i] for i in range(num_imgs)],
                             gt_bboxes_list, gt_labels_list, gt_bboxes_ignore_list)
        labels = torch.cat(labels_list, 0)
        label_weights = torch.cat(label_weights_list, 0)
        bbox_targets = torch.cat(bbox_targets_list, 0)
        bbox_weights = torch.cat(bbox_weights_list, 0)
        cls_scores = cls_scores.reshape(-1, self.cls_out_channels)
        cls_avg_factor = num_total_pos * 1.0 + num_total_neg * self.bg_cls_weight
        if self.sync_cls_avg_factor:
            cls_avg_factor = reduce_mean(cls_scores.new_tensor([cls_avg_factor]))
            cls_avg_factor = torch.clamp(cls_avg_factor, min=1)
        else:
            cls_avg_factor = max(cls_avg_factor, 1)
        loss_cls = self.loss_cls(cls_scores, labels, label_weights, avg_factor=cls_avg_factor)
        if torch.is_tensor(loss_cls) and loss_cls.dim() > 0:
            loss_cls = loss_cls.reshape(())
        num_total_pos = torch.clamp(reduce_mean(loss_cls.new_tensor([num_total_pos])), min=1).item()
        bbox_preds = bbox_preds.reshape(-1, bbox_preds.size(-1))
        normalized_bbox_targets = normalize_bbox(bbox_targets, self.pc_range)
        isnotnan = torch.isfinite(normalized_bbox_targets).all(dim=-1)
        bbox_weights = bbox_weights * self.code_weights
        loss_bbox = self.loss_bbox(bbox_preds[isnotnan, :10], normalized_bbox_targets[isnotnan, :10],
                                   bbox_weights[isnotnan, :10], avg_factor=num_total_pos)
        return torch.nan_to_num(loss_cls), torch.nan_to_num(loss_bbox)

    # ---- the fused plan (CUDA tensors) -------------------------------------------------------------------------------
    def _loss_fused(self, all_cls_scores, all_bbox_preds, gt_bboxes_list, gt_labels_list):
        NL, B, Q, C = all_cls_scores.shape
        device = all_cls_scores.device
        counts = [int(g.shape[0]) for g in gt_bboxes_list]
        total = sum(counts)
        gt_start = to_device_async(det_ops.gt_starts(counts), device, torch.int32)     # differs from step to step: not cached
        if total:
            if all(not g.is_cuda for g in gt_bboxes_list):           # one pinned staging copy each, no host wait
                host_labels = torch.cat(gt_labels_list)
                if int(host_labels.min()) < 0 or int(host_labels.max()) >= self.num_classes:
                    raise ValueError(f"gt_labels_3d outside [0, {self.num_classes})")
                raw = to_device_async(torch.cat(gt_bboxes_list).numpy(), device)
                gt_label = to_device_async(host_labels.numpy(), device, torch.int32)
            else:
                raw = torch.cat([g.to(device) for g in gt_bboxes_list]).float()
                gt_label = torch.cat([l.to(device) for l in gt_labels_list]).to(torch.int32)
            if raw.shape[-1] != 9:
                raise NotImplementedError("BEVFormerHead: ground-truth boxes without velocity (code size 8)")
            gt_norm = normalize_bbox(raw, self.pc_range).contiguous()
        else:
            gt_norm = all_bbox_preds.new_zeros((0, 10))
            gt_label = torch.zeros((0,), dtype=torch.int32, device=device)
        alpha, gamma = self.loss_cls.alpha, self.loss_cls.gamma
        if not hasattr(self.assigner.cls_cost, "gamma") or type(self.assigner.reg_cost).__name__ != "BBox3DL1Cost":
            raise NotImplementedError("BEVFormerHead: the fused loss tail needs FocalLossCost + BBox3DL1Cost in the assigner")
        cost = det_ops.match_cost(all_cls_scores, all_bbox_preds, gt_norm, gt_label, gt_start, total, self.assigner.cls_cost.alpha,
                                  float(self.assigner.cls_cost.gamma), float(self.assigner.cls_cost.weight),
                                  float(self.assigner.reg_cost.weight))
        # 'host' (default): det_ops.hungarian, the step's one host read.  'device': csrc/det_assign.hip, no read; the
        # status of the launch stays on the device until someone asks (det_ops.check_assign_status)
        matched, self.last_assign_status = det_ops.assign(cost, NL, B, Q, gt_start, counts)
        labels = det_ops.labels_from_matched(matched, gt_label, gt_start, self.num_classes)
        sums = det_ops.det_loss_sums(all_cls_scores, all_bbox_preds, labels, matched, gt_norm, gt_start, self.code_weights,
                                     alpha, gamma)
        # the assignment is a perfect matching of the smaller side: known without reading the device
        num_total_pos = sum(min(Q, g) for g in counts)
        num_total_neg = B * Q - num_total_pos
        cls_avg_factor = num_total_pos * 1.0 + num_total_neg * self.bg_cls_weight
        synced = dist.is_available() and dist.is_initialized()
        if synced:
            f = reduce_mean(to_device_async(np.asarray([cls_avg_factor if self.sync_cls_avg_factor else 0.0, num_total_pos],
                                                       dtype=np.float32), device))
            pos = torch.clamp(f[1], min=1)
            cls_avg = torch.clamp(f[0], min=1) if self.sync_cls_avg_factor else max(cls_avg_factor, 1)
        else:
            pos, cls_avg = max(num_total_pos, 1), max(cls_avg_factor, 1)
        losses_cls = torch.nan_to_num(sums[:, 0] * self.loss_cls.loss_weight / cls_avg)
        losses_bbox = torch.nan_to_num(sums[:, 1] * self.loss_bbox.loss_weight / pos)
        return losses_cls.unbind(0), losses_bbox.unbind(0)

    def loss(self, gt_bboxes_list, gt_labels_list, preds_dicts, gt_bboxes_ignore=None, img_metas=None):
        """bevformer_head.py:396-480 -> dict(loss_cls, loss_bbox, d0.loss_cls, d0.loss_bbox, ...)"""
        assert gt_bboxes_ignore is None, f"{self.__class__.__name__} only supports for gt_bboxes_ignore setting to None."
        if self.assigner is None:
            raise RuntimeError("BEVFormerHead.loss needs train_cfg with an assigner")
        all_cls_scores = preds_dicts["all_cls_scores"].float()
        all_bbox_preds = preds_dicts["all_bbox_preds"].float()
        if preds_dicts.get("enc_cls_scores") is not None:
            raise NotImplementedError("BEVFormerHead: as_two_stage=True")
        gt_bboxes_list = [torch.cat((g.gravity_center, g.tensor[:, 3:]), dim=1) for g in gt_bboxes_list]
        if det_ops.use_fused(all_cls_scores):
            losses_cls, losses_bbox = self._loss_fused(all_cls_scores, all_bbox_preds, gt_bboxes_list, gt_labels_list)
        else:
            device = all_cls_scores.device
            boxes = [g.to(device) for g in gt_bboxes_list]
            labels = [l.to(device).long() for l in gt_labels_list]
            per_layer = [self.loss_single(c, b, boxes, labels) for c, b in zip(all_cls_scores, all_bbox_preds)]
            losses_cls, losses_bbox = zip(*per_layer)
        loss_dict = dict(loss_cls=losses_cls[-1], loss_bbox=losses_bbox[-1])
        for i, (lc, lb) in enumerate(zip(losses_cls[:-1], losses_bbox[:-1])):
            loss_dict[f"d{i}.loss_cls"] = lc
            loss_dict[f"d{i}.loss_bbox"] = lb
        return loss_dict

    @torch.no_grad()
    def get_bboxes(self, preds_dicts, img_metas, rescale=False):
        """bevformer_head.py:483-509: decoded boxes, z moved from the gravity centre to the bottom face"""
        ret_list = []
        for i, preds in enumerate(self.bbox_coder.decode(preds_dicts)):
            bboxes = preds["bboxes"]
            bboxes[:, 2] = bboxes[:, 2] - bboxes[:, 5] * 0.5
            box_type = (img_metas[i] or {}).get("box_type_3d", LiDARInstance3DBoxes) if img_metas else LiDARInstance3DBoxes
            ret_list.append([box_type(bboxes, bboxes.shape[-1]), preds["scores"], preds["labels"]])
        return ret_list
