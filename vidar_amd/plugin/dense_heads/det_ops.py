"""The detection loss tail of BEVFormerHead (bevformer_head.py:215-393) for all decoder layers and samples at once.

Two implementations of the SAME arithmetic:
  * fused (CUDA tensors, default): csrc/det_loss.hip through ctypes -- `match_cost` is one launch, `hungarian` makes ONE
    pinned non-blocking copy + one event wait for the NL * B cost matrices of a step, `DetLossFunction` is one launch each
    way; the reductions are deterministic (same inputs, same bits); under `set_assign("device")` / VIDAR_DET_ASSIGN=device
    (off by default) `assign_device` solves all NL * B problems in one launch of csrc/det_assign.hip and no host read is
    left in the tail;
  * torch (`*_torch`, CPU tensors, or CUDA with VIDAR_DET_LOSS=torch): the plain composition -- the CPU path of the
    feature, the A/B partner for timing and the second opinion of the GPU tests.
Ground truth is packed over the batch: gt_box_norm [total_g, 10] (normalize_bbox applied), gt_label [total_g],
gt_counts = (G_0 .. G_{B-1}) known on the host; cost layout as in include/vidar_hip.h (a layer's row holds, per sample,
a [Q, G_b] row-major block at offset Q * start_b)."""
from __future__ import annotations

import os

import numpy as np
import torch

FLT_MIN = float(np.finfo(np.float32).tiny)
CODE = 10


def use_fused(t):
    mode = os.environ.get("VIDAR_DET_LOSS", "hip")
    if mode not in ("hip", "torch"):
        raise ValueError(f"VIDAR_DET_LOSS={mode!r}: expected 'hip' or 'torch'")
    return t.is_cuda and mode == "hip"


def gt_starts(gt_counts):
    return np.concatenate([[0], np.cumsum(np.asarray(gt_counts, dtype=np.int64))]).astype(np.int32)


def _pow(x, gamma):
    return x * x if gamma == 2.0 else x.pow(gamma)


# ---- matching cost -------------------------------------------------------------------------------------------------
def match_cost_torch(cls, box, gt_box_norm, gt_label, gt_counts, alpha, gamma, cls_weight, reg_weight):
    """FocalLossCost (mmdet, eps 1e-12) + BBox3DL1Cost over the first 8 code dims -> [NL, Q * total_g]"""
    NL, B, Q, C = cls.shape
    start = gt_starts(gt_counts)
    p = cls.sigmoid()
    pos = -alpha * _pow(1 - p, gamma) * (p + 1e-12).log()
    neg = -(1 - alpha) * _pow(p, gamma) * (1 - p + 1e-12).log()
    cc = (pos - neg) * cls_weight                                                 # [NL, B, Q, C]
    blocks = []
    for b in range(B):
        s, e = int(start[b]), int(start[b + 1])
        lab = gt_label[s:e].long()
        reg = (box[:, b, :, None, :8] - gt_box_norm[None, None, s:e, :8]).abs().sum(-1)      # [NL, Q, G]
        blocks.append((cc[:, b][:, :, lab] + reg * reg_weight).reshape(NL, -1))
    return torch.cat(blocks, 1) if blocks else cls.new_zeros((NL, 0))


def match_cost(cls, box, gt_box_norm, gt_label, gt_start_dev, total_g, alpha, gamma, cls_weight, reg_weight):
    """vidar_det_match_cost_f32.  gt_label / gt_start_dev int32 on the device."""
    from ..._lib import lib, check, ptr, stream_of
    if not cls.is_cuda:
        raise RuntimeError("det_ops.match_cost runs on the GPU only (match_cost_torch is the CPU composition)")
    NL, B, Q, C = cls.shape
    cls, box = cls.detach().float().contiguous(), box.detach().float().contiguous()
    assert box.shape == (NL, B, Q, CODE) and gt_label.dtype == torch.int32 and gt_start_dev.dtype == torch.int32
    cost = torch.empty((NL, Q * total_g), device=cls.device, dtype=torch.float32)
    check(lib().vidar_det_match_cost_f32(ptr(cls), ptr(box), ptr(gt_box_norm), ptr(gt_label), ptr(gt_start_dev), ptr(cost),
                                         alpha, gamma, cls_weight, reg_weight, NL, B, Q, C, int(total_g), stream_of(cls)),
          "det_match_cost")
    return cost


def solve(cost_host, NL, Q, gt_counts):
    """linear_sum_assignment on every (layer, sample) block of a host cost array [NL, Q * total_g]
    -> matched [NL, B, Q] int32 (index inside the sample's ground truth, -1 = background)"""
    from scipy.optimize import linear_sum_assignment
    B = len(gt_counts)
    start = gt_starts(gt_counts)
    matched = np.full((NL, B, Q), -1, dtype=np.int32)
    for l in range(NL):
        for b in range(B):
            G = int(gt_counts[b])
            if G == 0 or Q == 0:
                continue
            blk = cost_host[l, Q * int(start[b]):Q * int(start[b + 1])].reshape(Q, G)
            rows, cols = linear_sum_assignment(blk)
            matched[l, b, rows] = cols
    return matched


_PINNED = {}


def _pinned_like(cost):
    """one pinned staging buffer per process, grown when a step needs more: every use waits for its own copy before the
    host reads it, so the buffer is free again when the next step asks (a fresh pinned allocation per step is a slow,
    serialising driver call)"""
    buf = _PINNED.get("cost")
    if buf is None or buf.numel() < cost.numel():
        buf = _PINNED["cost"] = torch.empty(max(cost.numel(), 1 << 20), dtype=torch.float32, pin_memory=True)
    return buf[:cost.numel()].view(cost.shape)


def hungarian(cost, NL, Q, gt_counts):
    """device cost [NL, Q * total_g] -> matched [NL, B, Q] int32 on the device: ONE pinned non-blocking copy and one
    event wait for all NL * B problems, asynchronous upload of the result."""
    from ..utils.host import to_device_async
    if cost.numel() == 0:
        return torch.full((NL, len(gt_counts), Q), -1, dtype=torch.int32, device=cost.device)
    if cost.is_cuda:
        host = _pinned_like(cost)
        host.copy_(cost, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        done.synchronize()
    else:
        host = cost
    matched = solve(host.numpy(), NL, Q, gt_counts)
    return to_device_async(matched, cost.device, torch.int32)


# ---- the assignment on the device (csrc/det_assign.hip), off by default ------------------------------------------------
_ASSIGN_MODES = ("host", "device")
_ASSIGN = {"mode": None, "warned": False}
STATUS_MESSAGES = {1: "matrix contains invalid numeric entries", 2: "cost matrix is infeasible",
                   3: "gt_start does not describe the packed ground truth"}


def set_assign(mode):
    """'host' (scipy behind one cost copy, `hungarian`) or 'device' (`assign_device`, no host read); None hands the choice
    back to the environment variable VIDAR_DET_ASSIGN (same two values, default 'host')"""
    if mode is not None and mode not in _ASSIGN_MODES:
        raise ValueError(f"set_assign({mode!r}): expected 'host' or 'device'")
    _ASSIGN["mode"] = mode


def assign_mode():
    mode = _ASSIGN["mode"] or os.environ.get("VIDAR_DET_ASSIGN", "host")
    if mode not in _ASSIGN_MODES:
        raise ValueError(f"VIDAR_DET_ASSIGN={mode!r}: expected 'host' or 'device'")
    return mode


def assign_supported(NL, B, Q, total_g):
    """workspace bytes of vidar_det_assign_f32, or None when the extent is beyond the solver's LDS state (host arithmetic)"""
    import ctypes
    from ..._lib import lib, check
    n = ctypes.c_int64(0)
    check(lib().vidar_det_assign_workspace_bytes(NL, B, Q, int(total_g), ctypes.addressof(n)), "det_assign_workspace_bytes")
    return None if n.value < 0 else n.value


def assign_device(cost, NL, B, Q, gt_start_dev, total_g):
    """vidar_det_assign_f32: device cost [NL, Q * total_g] -> (matched [NL, B, Q] int32, status [NL * B] int32), both on
    the device and written completely by the launch (total_g == 0 included).  No host read, no event wait; runs on torch's
    current stream.  status: 0 solved, else see STATUS_MESSAGES / `check_assign_status`."""
    from ..._lib import lib, check, ptr, stream_of
    if not cost.is_cuda:
        raise RuntimeError("det_ops.assign_device runs on the GPU only (`solve` is the host path)")
    nbytes = assign_supported(NL, B, Q, total_g)
    if nbytes is None:
        raise ValueError(f"det_ops.assign_device: Q {Q} x total_g {total_g} is beyond the supported extent")
    cost = cost.detach().float().contiguous()
    assert cost.numel() == NL * Q * total_g and gt_start_dev.dtype == torch.int32 and gt_start_dev.numel() >= B + 1
    matched = torch.empty((NL, B, Q), device=cost.device, dtype=torch.int32)
    status = torch.empty((NL * B,), device=cost.device, dtype=torch.int32)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=cost.device) if nbytes else None
    check(lib().vidar_det_assign_f32(ptr(cost) if cost.numel() else None, ptr(gt_start_dev), ptr(matched) if Q else None,
                                     ptr(status), NL, B, Q, int(total_g), ptr(ws), nbytes, stream_of(cost)), "det_assign")
    return matched, status


def assign(cost, NL, B, Q, gt_start_dev, gt_counts):
    """the assignment of a step under the switch -> (matched, status or None).  'device' falls back to the host path, with
    one warning per process, for an extent the kernel does not hold."""
    total_g = int(sum(gt_counts))
    if assign_mode() == "device" and cost.is_cuda:
        if assign_supported(NL, B, Q, total_g) is not None:
            return assign_device(cost, NL, B, Q, gt_start_dev, total_g)
        if not _ASSIGN["warned"]:
            import warnings
            _ASSIGN["warned"] = True
            warnings.warn(f"device assignment: {Q} queries x {total_g} boxes is beyond the supported extent; "
                          "this and every such step is assigned on the host", RuntimeWarning, stacklevel=2)
    return hungarian(cost, NL, Q, gt_counts), None


def check_assign_status(status):
    """read a status tensor of `assign_device` (ONE host read: call it where the loss is read anyway, not per step) and
    raise what scipy.optimize.linear_sum_assignment would have raised for the first problem that was refused"""
    if status is None:
        return
    codes = status.detach().cpu().tolist()
    for p, code in enumerate(codes):
        if code:
            raise ValueError(f"{STATUS_MESSAGES.get(code, f'status {code}')} (assignment problem {p} of {len(codes)})")


def labels_from_matched(matched, gt_label, gt_start_dev, num_classes):
    """labels [NL, B, Q] int32 (num_classes = background) of an assignment, on the device the tensors live on"""
    B = matched.shape[1]
    if gt_label.numel() == 0:
        return torch.full_like(matched, num_classes)
    idx = (matched.clamp(min=0) + gt_start_dev[:B].view(1, B, 1)).long().clamp(max=gt_label.numel() - 1)
    return torch.where(matched >= 0, gt_label[idx], torch.full_like(matched, num_classes)).to(torch.int32)


# ---- losses --------------------------------------------------------------------------------------------------------
def det_loss_sums_torch(cls, box, labels, matched, gt_box_norm, gt_start_dev, code_weights, alpha, gamma):
    """-> [NL, 2]: sigmoid focal loss sums (mmcv semantics) and the code-weighted L1 sums of the matched queries whose
    target row is finite (bevformer_head.py:381-389)"""
    NL, B, Q, C = cls.shape
    p = cls.sigmoid()
    onehot = labels.long().unsqueeze(-1) == torch.arange(C, device=cls.device).view(1, 1, 1, C)
    tiny = torch.full_like(p, FLT_MIN)
    focal = torch.where(onehot, -alpha * _pow(1 - p, gamma) * torch.maximum(p, tiny).log(),
                        -(1 - alpha) * _pow(p, gamma) * torch.maximum(1 - p, tiny).log())
    s_cls = focal.reshape(NL, -1).sum(1)
    if gt_box_norm.shape[0] == 0:
        return torch.stack([s_cls, (box * 0).reshape(NL, -1).sum(1)], 1)
    idx = (matched.clamp(min=0) + gt_start_dev[:B].view(1, B, 1)).long().clamp(max=gt_box_norm.shape[0] - 1)
    tgt = gt_box_norm[idx]                                                        # [NL, B, Q, 10]
    ok = (matched >= 0) & torch.isfinite(tgt).all(-1)
    diff = (box - torch.where(ok.unsqueeze(-1), tgt, box.detach())).abs() * code_weights
    s_box = torch.where(ok.unsqueeze(-1), diff, torch.zeros_like(diff)).reshape(NL, -1).sum(1)
    return torch.stack([s_cls, s_box], 1)


class DetLossFunction(torch.autograd.Function):
    """vidar_det_loss_fwd_f32 / vidar_det_loss_bwd_f32: (cls, box) -> [NL, 2] sums"""

    @staticmethod
    def forward(ctx, cls, box, labels, matched, gt_box_norm, gt_start_dev, code_weights, alpha, gamma):
        from ..._lib import lib, check, ptr, stream_of, workspace
        if not cls.is_cuda:
            raise RuntimeError("DetLossFunction runs on the GPU only (det_loss_sums_torch is the CPU composition)")
        NL, B, Q, C = cls.shape
        cls, box = cls.float().contiguous(), box.float().contiguous()
        labels, matched = labels.contiguous(), matched.contiguous()
        gt_box_norm, code_weights = gt_box_norm.float().contiguous(), code_weights.float().contiguous()
        assert box.shape == (NL, B, Q, CODE) and labels.dtype == torch.int32 and matched.dtype == torch.int32
        assert gt_start_dev.dtype == torch.int32 and code_weights.numel() == CODE
        total_g = gt_box_norm.shape[0]
        sums = torch.empty((NL, 2), device=cls.device, dtype=torch.float32)
        ws, ws_ptr, ws_n = workspace(lib().vidar_det_loss_workspace_bytes, NL, B, Q, like=cls)
        check(lib().vidar_det_loss_fwd_f32(ptr(cls), ptr(box), ptr(labels), ptr(matched), ptr(gt_box_norm), ptr(gt_start_dev),
                                           ptr(code_weights), ptr(sums), alpha, gamma, NL, B,
                                           Q, C, total_g, ws_ptr, ws_n, stream_of(cls)), "det_loss_fwd")
        ctx.save_for_backward(cls, box, labels, matched, gt_box_norm, gt_start_dev, code_weights)
        ctx.cfg = (float(alpha), float(gamma))
        return sums

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        from ..._lib import lib, check, ptr, stream_of
        cls, box, labels, matched, gt_box_norm, gt_start_dev, code_weights = ctx.saved_tensors
        alpha, gamma = ctx.cfg
        NL, B, Q, C = cls.shape
        g = g.float().contiguous()
        d_cls, d_box = torch.empty_like(cls), torch.empty_like(box)
        check(lib().vidar_det_loss_bwd_f32(ptr(cls), ptr(box), ptr(labels), ptr(matched), ptr(gt_box_norm), ptr(gt_start_dev),
                                           ptr(code_weights), ptr(g), ptr(d_cls), ptr(d_box), alpha, gamma,
                                           NL, B, Q, C, gt_box_norm.shape[0], stream_of(cls)),
              "det_loss_bwd")
        return d_cls, d_box, None, None, None, None, None, None, None


def det_loss_sums(cls, box, labels, matched, gt_box_norm, gt_start_dev, code_weights, alpha, gamma):
    if use_fused(cls):
        return DetLossFunction.apply(cls, box, labels, matched, gt_box_norm, gt_start_dev, code_weights, alpha, gamma)
    return det_loss_sums_torch(cls, box, labels, matched, gt_box_norm, gt_start_dev, code_weights, alpha, gamma)
