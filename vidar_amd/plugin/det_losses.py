"""Losses the detection head names in its config.  Third party (mmdet), recalled, unpinned:
  * FocalLoss -- sigmoid form only; elementwise mmcv `sigmoid_focal_loss` semantics (target class
    -alpha (1-p)^gamma log(max(p, FLT_MIN)), other classes -(1-alpha) p^gamma log(max(1-p, FLT_MIN)), label == num_classes is
    background), optional per-sample weight, `avg_factor`: loss_weight * sum / avg_factor;
  * L1Loss -- loss_weight * sum(|pred - target| * weight) / avg_factor (mean without an avg_factor);
  * GIoULoss -- accepted with loss_weight 0 only (the released configs carry it as a placeholder)."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from .registry import LOSSES

FLT_MIN = float(np.finfo(np.float32).tiny)


def sigmoid_focal_loss(pred, target, gamma=2.0, alpha=0.25):
    """[N, C] logits, [N] labels in [0, C] -> [N, C] elementwise loss"""
    p = pred.sigmoid()
    onehot = target.long().unsqueeze(-1) == torch.arange(pred.shape[-1], device=pred.device)
    tiny = torch.full_like(p, FLT_MIN)
    pg = (1 - p) * (1 - p) if gamma == 2.0 else (1 - p).pow(gamma)
    ng = p * p if gamma == 2.0 else p.pow(gamma)
    return torch.where(onehot, -alpha * pg * torch.maximum(p, tiny).log(), -(1 - alpha) * ng * torch.maximum(1 - p, tiny).log())


def _weight_reduce(loss, weight, reduction, avg_factor):
    if weight is not None:
        loss = loss * weight
    if avg_factor is None:
        return loss.mean() if reduction == "mean" else (loss.sum() if reduction == "sum" else loss)
    if reduction == "mean":
        return loss.sum() / avg_factor
    if reduction == "none":
        return loss
    raise ValueError('avg_factor can not be used with reduction="sum"')


@LOSSES.register_module()
class FocalLoss(nn.Module):
    def __init__(self, use_sigmoid=True, gamma=2.0, alpha=0.25, reduction="mean", loss_weight=1.0, activated=False):
        super().__init__()
        if not use_sigmoid:
            raise NotImplementedError("FocalLoss: use_sigmoid=False")
        if activated:
            raise NotImplementedError("FocalLoss: activated=True")
        self.use_sigmoid, self.gamma, self.alpha = use_sigmoid, float(gamma), float(alpha)
        self.reduction, self.loss_weight = reduction, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None):
        loss = sigmoid_focal_loss(pred, target, self.gamma, self.alpha)
        if weight is not None and weight.dim() == 1:
            weight = weight.view(-1, 1)
        return self.loss_weight * _weight_reduce(loss, weight, reduction_override or self.reduction, avg_factor)


@LOSSES.register_module()
class L1Loss(nn.Module):
    def __init__(self, reduction="mean", loss_weight=1.0):
        super().__init__()
        self.reduction, self.loss_weight = reduction, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None):
        if target.numel() == 0:
            return pred.sum() * 0
        return self.loss_weight * _weight_reduce((pred - target).abs(), weight, reduction_override or self.reduction,
                                                 avg_factor)


@LOSSES.register_module()
class GIoULoss(nn.Module):
    def __init__(self, eps=1e-6, reduction="mean", loss_weight=1.0):
        super().__init__()
        if loss_weight != 0:
            raise NotImplementedError("GIoULoss with a non-zero loss_weight")
        self.loss_weight = loss_weight


def build_loss(cfg, **kw):
    return LOSSES.build(cfg, **kw)


def bias_init_with_prob(prior_prob):
    """mmcv.cnn.bias_init_with_prob"""
    return float(-np.log((1 - prior_prob) / prior_prob))
