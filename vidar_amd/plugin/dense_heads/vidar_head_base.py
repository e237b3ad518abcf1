"""ViDARHeadTemplate / ViDARHeadBase -- registry names, kwargs, parameter names and loss / decode
semantics of projects/mmdet3d_plugin/bevformer/dense_heads/vidar_head_base.py:31-773.

What changed is the execution plan, not the math:
  * the waypoint / grid_sample / -inf mask / cross-entropy chain (:420-509, :586-592) is one fused
    kernel per (batch item) call (ray_ops.ray_ce), likewise the distance loss on the GT rays
    (:575-585, ray_ops.ray_dist), the dense gumbel render (:594-630, :754-773) and the test-time
    arg-max decode (:697-731); any ray_grid_num up to ray_ops.max_k();
  * GT clouds are never compacted with boolean indexing (host syncs at :441, :464-467, :636-644):
    rays carry a frame slot (-1 = ignore) and validity is decided on device;
  * the training chamfer (:654) runs on the nearest-neighbour kernel with a validity mask instead
    of a dense [N, M, 3] expansion."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from ..utils.host import const_tensor, to_device_async
import torch.nn as nn
import torch.nn.functional as F

from ..bricks import xavier_init
from ..losses import chamfer_distance
from ..registry import HEADS, build_positional_encoding, build_transformer
from ..utils import e2e_predictor_utils
from . import ray_ops


class DecodeRays(NamedTuple):
    """The rays the decode marches (ViDARHeadBase._decode_rays), per sample b what a listed ray op takes:
    (volumes[b], origin_grids[b], end_grids[b], tindex[b]) in voxel units."""
    volumes: tuple               # bs x [F, Z, H, W] logits
    origin_grids: torch.Tensor   # [bs, F, 3]
    end_grids: torch.Tensor      # [bs, N, 3], a NaN (padding) moved far outside: -1e6
    tindex: torch.Tensor         # [bs, N] frame slot of a ray, -1 = skip it
    origin_pts: torch.Tensor     # [bs, F, 3] metric origins
    xyz: torch.Tensor            # [bs, N, 3] metric end points, NaN-padded
    scale: float                 # metres per voxel unit along a ray (the BEV cell size)
    shape: tuple                 # (F, Z, H, W)


def _metre_stats(stats, scale):
    """[..., 4] (p_max, mean, rms, entropy) of ray_ops.ray_stats: the two lengths from voxel units to metres"""
    return stats * const_tensor([1.0, scale, scale, 1.0], stats.device, stats.dtype)


@HEADS.register_module()
class ViDARHeadTemplate(nn.Module):
    def __init__(self, *args, transformer=None, num_pred_fcs=2, num_pred_height=1, can_bus_norm=True,
                 can_bus_dims=(0, 1, 2, 17), bev_h=30, bev_w=30, pc_range=None, loss_weight=None,
                 positional_encoding=dict(type="SinePositionalEncoding", num_feats=128, normalize=True),
                 eval_within_grid=False, init_cfg=None, **kwargs):
        super().__init__()
        self.bev_h, self.bev_w = bev_h, bev_w
        self.pc_range = pc_range
        self.real_w = pc_range[3] - pc_range[0]
        self.real_h = pc_range[4] - pc_range[1]
        self.can_bus_norm = can_bus_norm
        self.can_bus_dims = can_bus_dims
        self.num_pred_fcs = num_pred_fcs
        self.num_pred_height = num_pred_height
        self.positional_encoding = build_positional_encoding(positional_encoding)
        self.transformer = build_transformer(transformer)
        self.embed_dims = self.transformer.embed_dims
        self.loss_weight = np.array(loss_weight)
        assert self.loss_weight.shape[-1] == 1
        self.eval_within_grid = eval_within_grid
        self._init_layers()

    def _init_layers(self):
        self.bev_embedding = nn.Embedding(self.bev_h * self.bev_w, self.embed_dims)
        self.prev_frame_embedding = nn.Parameter(torch.Tensor(1, self.embed_dims))
        self.can_bus_mlp = nn.Sequential(
            nn.Linear(len(self.can_bus_dims), self.embed_dims // 2), nn.ReLU(inplace=True),
            nn.Linear(self.embed_dims // 2, self.embed_dims), nn.ReLU(inplace=True))
        if self.can_bus_norm:
            self.can_bus_mlp.add_module("norm", nn.LayerNorm(self.embed_dims))

    def init_weights(self):
        if getattr(self, "transformer", None) is None:
            return
        self.transformer.init_weights()
        nn.init.normal_(self.prev_frame_embedding)
        xavier_init(self.can_bus_mlp, distribution="uniform", bias=0.)

    def _get_next_bev_features(self, prev_features, img_metas, target_frame_index, tgt_points,
                               ref_points, bev_h, bev_w):
        bs = prev_features.shape[0]
        dtype = prev_features.dtype
        bev_queries = self.bev_embedding.weight.to(dtype).unsqueeze(0)
        bev_mask = torch.zeros((bs, self.bev_h, self.bev_w), device=bev_queries.device).to(dtype)
        bev_pos = self.positional_encoding(bev_mask).to(dtype)
        can_bus = np.array([m["future_can_bus"][target_frame_index] for m in img_metas])[:, self.can_bus_dims]
        can_bus = to_device_async(can_bus, bev_pos.device, dtype)
        bev_queries_input = bev_queries + self.can_bus_mlp(can_bus).unsqueeze(1)
        prev_features_input = prev_features + self.prev_frame_embedding[None, :, None, :]
        return self.transformer(prev_features_input, bev_queries_input, tgt_points=tgt_points,
                                ref_points=ref_points, bev_h=bev_h, bev_w=bev_w, bev_pos=bev_pos,
                                img_metas=img_metas)

    def forward(self, prev_feats, img_metas, target_frame_index, tgt_points, ref_points, bev_h, bev_w):
        bs, num_frames, bev_grids_num, bev_dims = prev_feats.shape
        assert bev_dims == self.embed_dims
        assert bev_h * bev_w == bev_grids_num == tgt_points.shape[1]
        return self._get_next_bev_features(prev_feats, img_metas, target_frame_index, tgt_points,
                                           ref_points, bev_h, bev_w)

    # ------------------------------------------------------------------------------------------
    def _process_gt_points(self, bev_preds, gt_points, batched_origin_points, valid_frames,
                           start_idx, pred_frame_num, bev_h, bev_w, pc_range):
        """Select the GT rays of `valid_frames` (:219-276).  Static shapes: every point is kept, the
        per-ray frame slot `tindex` is -1 for points of other frames (the reference drops them and
        NaN-pads to the longest cloud of the batch instead)."""
        valid_frame_num, inter_num, bs, token_num, num_height_pred = bev_preds.shape
        max_pts = max(p.shape[0] for p in gt_points)
        pts = torch.stack([F.pad(p, (0, 0, 0, max_pts - p.shape[0]), value=float("nan"))
                           for p in gt_points])
        t = pts[..., -1] - start_idx
        keep = torch.zeros_like(t, dtype=torch.bool)
        for i in range(start_idx, pred_frame_num):
            if i in valid_frames:
                keep |= pts[..., -1] == i
        tindex = torch.where(keep, t, torch.full_like(t, -1.0))
        tindex = torch.clamp(tindex, max=valid_frame_num - 1)
        xyz = pts[..., :3].contiguous()
        if batched_origin_points is None:
            batched_origin_points = xyz.new_zeros((bs, len(valid_frames), 3))
        origin_grids = e2e_predictor_utils.coords_to_voxel_grids(
            batched_origin_points, bev_h=bev_h, bev_w=bev_w, pillar_num=num_height_pred, pc_range=pc_range)
        gt_grids = e2e_predictor_utils.coords_to_voxel_grids(
            xyz, bev_h=bev_h, bev_w=bev_w, pillar_num=num_height_pred, pc_range=pc_range)
        return origin_grids, batched_origin_points, gt_grids, xyz, tindex

    def get_rendered_pcds(self, origin, points, tindex, gt_dist, pred_dist, pc_range):
        """(:344-389) list[bs] of list[frames] of [n,3] rendered points (boolean selection: used by
        the evaluation path, where a sync per frame is harmless)."""
        bs, num_frames, _ = origin.shape
        pcds = []
        for b in range(bs):
            per_frame = []
            for t in range(num_frames):
                mask = self._rendered_mask(points[b], tindex[b], gt_dist[b], t, pc_range)
                p = points[b][mask]
                r = p - origin[b, t].view(1, 3)
                rn = r / torch.sqrt((r ** 2).sum(1, keepdim=True))
                per_frame.append(origin[b, t].view(1, 3) + rn * pred_dist[b][mask].view(-1, 1))
            pcds.append(per_frame)
        return pcds

    def _rendered_mask(self, points, tindex, gt_dist, t, pc_range):
        """the rays of one sample that get_rendered_pcds keeps for frame t"""
        mask = (tindex == t) & (gt_dist > 0.)
        if self.eval_within_grid:
            mask = mask & e2e_predictor_utils.get_inside_mask(points, pc_range)
        return mask

    def get_rendered_stats(self, points, tindex, gt_dist, stats, pc_range, num_frames):
        """per-ray values stats [bs, N, 4] laid out like get_rendered_pcds' points: list[bs] of list[frames] of [n, 4]"""
        return [[stats[b][self._rendered_mask(points[b], tindex[b], gt_dist[b], t, pc_range)]
                 for t in range(num_frames)] for b in range(len(stats))]

    def get_rendered_rays(self, origin, points, tindex, gt_dist, pred_dist, pc_range):
        """get_rendered_pcds without the boolean selections (no host sync): every ray keeps its place, the selection
        is the per-ray frame id.  -> dict(pred_pts [bs,N,3], gt_pts [bs,N,3] -- the rendered points of the predicted
        and of the ground-truth depth --, frame [bs,N] int64: the frame a ray belongs to, -1 for a ray that
        get_rendered_pcds would drop (its points may hold anything, NaN included), origin [bs,F,3])."""
        bs, num_frames, _ = origin.shape
        valid = (tindex >= 0) & (tindex < num_frames) & (gt_dist > 0.)
        if self.eval_within_grid:
            valid = valid & e2e_predictor_utils.get_inside_mask(points, pc_range)
        frame = torch.where(valid, tindex, torch.full_like(tindex, -1.0)).long()
        o = torch.gather(origin, 1, frame.clamp(min=0).unsqueeze(-1).expand(-1, -1, 3))
        r = points - o
        rn = r / torch.sqrt((r ** 2).sum(-1, keepdim=True))
        return dict(pred_pts=o + rn * pred_dist.unsqueeze(-1), gt_pts=o + rn * gt_dist.unsqueeze(-1), frame=frame,
                    origin=origin)


@HEADS.register_module()
class ViDARHeadBase(ViDARHeadTemplate):
    def __init__(self, ray_grid_num=1026, ray_grid_step=1.0, use_ce_loss=True, use_dist_loss=False,
                 use_dense_loss=True, dense_loss_weight=1.0, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.ray_grid_num = ray_grid_num
        self.ray_grid_step = ray_grid_step
        self.use_ce_loss = use_ce_loss
        self.use_dist_loss = use_dist_loss
        self.use_dense_loss = use_dense_loss
        assert self.use_ce_loss or self.use_dist_loss or self.use_dense_loss
        self.dense_loss_weight = dense_loss_weight
        self.gumbel_noise_fn = None      # tests inject the reference's noise here

    @staticmethod
    def _volumes(bev_preds, b, Z, H, W):
        """bev_preds [F, 1, bs, H*W, Z] -> sigma of batch item b as [F, Z, H, W] (:548-558)."""
        return bev_preds[:, 0, b].permute(0, 2, 1).contiguous().view(-1, Z, H, W)

    def _dense_rays(self, bs, F_, Z, H, W, device):
        interval = 4
        v = e2e_predictor_utils.get_bev_grids_3d(H // interval, W // interval, Z // interval, bs=1,
                                                 device=device)
        v = (v * const_tensor([W, H, Z], v.device, v.dtype)).view(-1, 3)
        pts = v.repeat(F_, 1)
        tix = torch.arange(F_, device=device, dtype=v.dtype).repeat_interleave(v.shape[0])
        return pts, tix, v.shape[0]

    def loss(self, pred_dict, gt_points, start_idx, tgt_bev_h, tgt_bev_w, tgt_pc_range,
             pred_frame_num, img_metas=None, batched_origin_points=None, loss_weight=None):
        valid_frames = pred_dict["valid_frames"]
        bev_preds = pred_dict["next_bev_preds"][:, -1:].float()
        F_, inter_num, bs, token_num, Z = bev_preds.shape
        H, W = tgt_bev_h, tgt_bev_w
        origin_grids, origin_pts, gt_grids, gt_xyz, tindex = self._process_gt_points(
            bev_preds, gt_points, batched_origin_points, valid_frames, start_idx, pred_frame_num,
            H, W, tgt_pc_range)
        loss_weight = self.loss_weight if loss_weight is None else loss_weight
        lw = const_tensor(np.asarray(loss_weight, dtype=np.float32)[:, 0], bev_preds.device)
        step = self.ray_grid_step
        loss_dict = dict()
        sigmas = [self._volumes(bev_preds, b, Z, H, W) for b in range(bs)]

        if self.use_dist_loss:
            # (:575-585) hard gumbel sample over {end point, waypoints} of the GT rays, L1 against the ray length.
            # Its noise is drawn before the dense loss's, as in the reference.
            num = bev_preds.new_zeros(())
            den = bev_preds.new_zeros(())
            scale = (tgt_pc_range[3] - tgt_pc_range[0]) / W
            for b in range(bs):
                R = gt_grids[b].shape[0]
                noise = (self.gumbel_noise_fn(R, self.ray_grid_num + 1) if self.gumbel_noise_fn
                         else ray_ops.gumbel_noise(R, self.ray_grid_num + 1, gt_grids.device))
                dist, gt_len, valid = ray_ops.ray_dist(sigmas[b], origin_grids[b], gt_grids[b], tindex[b], noise,
                                                       step, self.ray_grid_num)
                w = lw[tindex[b].clamp(min=0).long()] * valid
                num = num + (torch.abs(dist - gt_len) * scale * w).sum()
                den = den + w.sum()
            loss_dict["dist.loss"] = num / torch.clamp(den, min=1)

        if self.use_ce_loss:
            num = bev_preds.new_zeros(())
            den = bev_preds.new_zeros(())
            for b in range(bs):
                ce, valid = ray_ops.ray_ce(sigmas[b], origin_grids[b], gt_grids[b], tindex[b], step,
                                           self.ray_grid_num)
                w = lw[tindex[b].clamp(min=0).long()] * valid
                num = num + (ce * w).sum()
                den = den + w.sum()
            loss_dict["regularization.loss"] = num / torch.clamp(den, min=1)

        if self.use_dense_loss:
            pts, tix, per_frame = self._dense_rays(bs, F_, Z, H, W, bev_preds.device)
            total = bev_preds.new_zeros(())
            size = const_tensor([W - 1, H - 1, Z - 1], gt_grids.device, gt_grids.dtype)
            for b in range(bs):
                noise = (self.gumbel_noise_fn(pts.shape[0], self.ray_grid_num) if self.gumbel_noise_fn
                         else ray_ops.gumbel_noise(pts.shape[0], self.ray_grid_num, pts.device))
                dist = ray_ops.ray_gumbel(sigmas[b], origin_grids[b], pts, tix, noise, step,
                                          self.ray_grid_num)
                inside = ((gt_grids[b] > 0) & (gt_grids[b] < size)).all(-1)
                for f in range(F_):
                    o = origin_grids[b, f].view(1, 3)
                    p = pts[f * per_frame:(f + 1) * per_frame]
                    r = p - o
                    d = dist[f * per_frame:(f + 1) * per_frame]
                    # get_rendered_pcds keeps rays with a positive rendered distance only (:392-395);
                    # a dense voxel centre that coincides with the origin (zero-length ray) drops out
                    live = d > 0
                    # NaN-free also for the dropped zero-length ray: a masked 0/0 would still poison the
                    # backward of `unit * d` (0 * NaN), so the norm is floored and d masked BEFORE the product
                    unit = r / torch.sqrt((r ** 2).sum(1, keepdim=True)).clamp_min(1e-12)
                    pred = unit * torch.where(live, d, torch.zeros_like(d)).view(-1, 1) * 0.1
                    gt = (gt_grids[b] - o) * 0.1
                    valid = inside & (tindex[b] == f)
                    ls, lt, _, _ = chamfer_distance(pred[None], gt[None], dst_valid=valid[None],
                                                    src_valid=live[None])
                    has = (valid.sum() > 0).to(ls.dtype)
                    total = total + (ls + lt) / 2. * lw[f] * has
            loss_dict["loss.dense_voxel"] = total / (float(np.sum(loss_weight)) * bs) * self.dense_loss_weight
        return loss_dict

    @torch.no_grad()
    def get_point_cloud_prediction(self, pred_dict, gt_points, start_idx, tgt_bev_h, tgt_bev_w,
                                   tgt_pc_range, img_metas=None, batched_origin_points=None, as_rays=False):
        """arg-max decode (:663-752) -> dict(pred_pcds, gt_pcds, origin); as_rays: the dict of get_rendered_rays
        instead (the device metrics' input: nothing is selected on the host)."""
        rays = self._decode_rays(pred_dict, gt_points, start_idx, tgt_bev_h, tgt_bev_w, tgt_pc_range, img_metas,
                                 batched_origin_points)
        pred, gt, _ = self._decode_dists(ray_ops.ray_argmax, rays)
        if as_rays:
            return self.get_rendered_rays(rays.origin_pts, rays.xyz, rays.tindex, gt, pred, tgt_pc_range)
        return dict(
            pred_pcds=self.get_rendered_pcds(rays.origin_pts, rays.xyz, rays.tindex, gt, pred, tgt_pc_range),
            gt_pcds=self.get_rendered_pcds(rays.origin_pts, rays.xyz, rays.tindex, gt, gt, tgt_pc_range),
            origin=rays.origin_pts)

    def _decode_rays(self, pred_dict, points, start_idx, tgt_bev_h, tgt_bev_w, tgt_pc_range, img_metas=None,
                     batched_origin_points=None):
        """The one place that turns (pred_dict, points) into the rays a decode marches -> DecodeRays.  Which logits and
        which coordinates is the subclass's pair of hooks, _decode_preds and _decode_points; every route below -- the
        decode, render_rays, render_occupancy, measured_occupancy, occupancy_at, render_occupancy_dense (volumes and
        origins only) -- takes its rays from here, so they agree bit for bit."""
        bev_preds = self._decode_preds(pred_dict).float()
        points, batched_origin_points = self._decode_points(pred_dict, points, batched_origin_points, img_metas)
        F_, inter_num, bs, token_num, Z = bev_preds.shape
        H, W = tgt_bev_h, tgt_bev_w
        origin_grids, origin_pts, gt_grids, gt_xyz, tindex = self._process_gt_points(
            bev_preds, points, batched_origin_points, pred_dict["valid_frames"], start_idx, F_, H, W, tgt_pc_range)
        last = bev_preds[:, -1:]
        return DecodeRays(tuple(self._volumes(last, b, Z, H, W) for b in range(bs)), origin_grids,
                          torch.nan_to_num(gt_grids, nan=-1.0e6), tindex, origin_pts, gt_xyz,
                          (tgt_pc_range[3] - tgt_pc_range[0]) / W, (F_, Z, H, W))

    def _march(self, op, rays):
        """op(sigma, origin, pts, tindex, step, K) -- a listed op of ray_ops -- on every sample of `rays`, in order"""
        return [op(rays.volumes[b], rays.origin_grids[b], rays.end_grids[b], rays.tindex[b], self.ray_grid_step,
                   self.ray_grid_num) for b in range(len(rays.volumes))]

    def _decode_dists(self, op, rays):
        """ray_ops.ray_argmax or ray_ops.ray_stats on `rays` -> (pred [bs, N], gt [bs, N] in metres, what else the op
        returned, stacked over the samples)"""
        pred, gt, *more = (torch.stack(t) for t in zip(*self._march(op, rays)))
        return pred * rays.scale, gt * rays.scale, more

    @staticmethod
    def _evidence(pairs):
        """per sample (hit, free), each [F, Z, H, W] -> [bs, F, 2, Z, H, W]"""
        return torch.stack([torch.stack(pair, 1) for pair in pairs])

    def _ray_frame_labels(self, valid_frames):
        """the value the last column of a point holds for each frame slot of `valid_frames`"""
        return [float(f) for f in valid_frames]

    def _decode_preds(self, pred_dict):
        """hook of _decode_rays: the logits to decode, [F, inter, bs, Q, Z]"""
        return pred_dict["next_bev_preds"]

    def _decode_points(self, pred_dict, points, batched_origin_points, img_metas):
        """hook of _decode_rays: (points, batched_origin_points) in the coordinates the decoded volumes live in (here:
        as they are)"""
        return points, batched_origin_points

    def frame_alignment(self, valid_frames, img_metas):
        """[bs, F, 4, 4] fp64, row-vector form: frame slot f's own LiDAR coordinates -> the coordinates its decoded
        volume lives in (the identity here: this head takes its rays as they are)."""
        return np.tile(np.eye(4), (len(img_metas), len(valid_frames), 1, 1))

    @torch.no_grad()
    def render_cameras(self, pred_dict, img_metas, tgt_bev_h, tgt_bev_w, tgt_pc_range, cameras=None, stride=4,
                       return_stats=False):
        """The decode seen from the cameras: one ray per `stride` x `stride` block of every camera's pixels, through the
        block's centre, marched by ray_ops.ray_argmax_cam (the rays are never stored).
        cameras: indices into img_metas[b]["lidar2img"] (None or "all" = all; their images must share one size).
        -> depth [bs, F, C, Hs, Ws], Hs = ceil(H / stride): metres along the ray (voxel units times the BEV cell size, the
        decode's own scale), 0 where the ray meets nothing.  The cameras of a future frame are the current frame's, by the
        rigid-rig assumption of vidar_amd.forecast.pix2vox.
        return_stats: march with ray_ops.ray_stats_cam instead (the same depth bits) -> (depth, stats [bs, F, C, Hs, Ws, 4]):
        (p_max, mean, rms, entropy) of the softmax along each ray, mean and rms in metres, zeros where it meets nothing."""
        scale = (tgt_pc_range[3] - tgt_pc_range[0]) / tgt_bev_w
        decode = ray_ops.ray_stats_cam if return_stats else ray_ops.ray_argmax_cam
        out, stats = [], []
        for args, kw in self._camera_marches(pred_dict, img_metas, tgt_bev_h, tgt_bev_w, tgt_pc_range, cameras, stride):
            d = decode(*args, **kw)
            if return_stats:
                d, s = d
                stats.append(s)
            out.append(d * scale)
        if return_stats:
            return torch.stack(out), _metre_stats(torch.stack(stats), scale)
        return torch.stack(out)

    def _camera_marches(self, pred_dict, img_metas, tgt_bev_h, tgt_bev_w, tgt_pc_range, cameras, stride):
        """per sample, the arguments of a ray_ops.*_cam call on render_cameras' rays: ((sigma, pix2vox, hw), keywords);
        cameras: indices, or None / "all" for every camera"""
        from ...forecast import pix2vox
        stride = int(stride)
        if stride < 1:
            raise ValueError("stride must be >= 1")
        if isinstance(cameras, str) and cameras == "all":
            cameras = None
        bev_preds = self._decode_preds(pred_dict).float()
        F_, inter_num, bs, token_num, Z = bev_preds.shape
        last = bev_preds[:, -1:]
        align = self.frame_alignment(pred_dict["valid_frames"], img_metas)
        for b in range(bs):
            meta = img_metas[b]
            cams = list(range(len(meta["lidar2img"]))) if cameras is None else [int(c) for c in cameras]
            sizes = {tuple(meta["img_shape"][c][:2]) for c in cams}
            if len(sizes) != 1:
                raise ValueError(f"the cameras' images must share one size, got {sorted(sizes)}")
            H, W = sizes.pop()
            m = pix2vox([meta["lidar2img"][c] for c in cams], tgt_pc_range, tgt_bev_h, tgt_bev_w, Z, align[b])
            yield ((self._volumes(last, b, Z, tgt_bev_h, tgt_bev_w), m.to(bev_preds.device),
                    (-(-H // stride), -(-W // stride))),
                   dict(u0=stride / 2.0, v0=stride / 2.0, du=float(stride), dv=float(stride), step=self.ray_grid_step,
                        K=self.ray_grid_num))

    @torch.no_grad()
    def render_rays(self, pred_dict, directions=None, end_points=None, *, tgt_bev_h, tgt_bev_w, tgt_pc_range,
                    img_metas=None, start_idx=0, batched_origin_points=None, return_stats=False):
        """The decode of get_point_cloud_prediction along rays handed in instead of taken from `gt_points`: the same
        origin, voxel mapping, ray_argmax call and masking, because both take their rays from _decode_rays.  Exactly one of
          directions [R, 3]: unit directions in every predicted frame's own sensor coordinates, shared by all samples
                             and frames (vidar_amd.forecast.lidar_pattern); the ray's end point is the point 1 m out;
          end_points list[bs] of [N, >=4]: points in the layout of gt_points (xyz first, the frame label last).
        -> list[bs] of list[frames] of [n, 3] predicted points, ray order kept within a frame.  A ray without a live
        waypoint comes back at waypoint 0 (the reference's decode); with eval_within_grid the end point's own
        membership still selects the ray, as for ground truth.
        return_stats: decode with ray_ops.ray_stats instead (the same points) -> (points, stats): list[bs] of list[frames]
        of [n, 4], row for row the points' (p_max, mean, rms, entropy), mean and rms in metres; a ray without a live
        waypoint has four zeros."""
        end_points = self._listed_end_points(pred_dict, directions, end_points)
        rays = self._decode_rays(pred_dict, end_points, start_idx, tgt_bev_h, tgt_bev_w, tgt_pc_range, img_metas,
                                 batched_origin_points)
        pred, gt, stats = self._decode_dists(ray_ops.ray_stats if return_stats else ray_ops.ray_argmax, rays)
        points = self.get_rendered_pcds(rays.origin_pts, rays.xyz, rays.tindex, gt, pred, tgt_pc_range)
        if not return_stats:
            return points
        return points, self.get_rendered_stats(rays.xyz, rays.tindex, gt, _metre_stats(stats[0], rays.scale),
                                               tgt_pc_range, rays.origin_pts.shape[1])

    def _listed_end_points(self, pred_dict, directions, end_points):
        """render_rays' rays in the layout of gt_points: the end points as they are, or the points 1 m out along
        `directions` in every frame"""
        if (directions is None) == (end_points is None):
            raise ValueError("give either directions or end_points")
        if end_points is None:
            bs = pred_dict["next_bev_preds"].shape[-3]
            d = directions.float()
            cols = [torch.cat([d, d.new_full((d.shape[0], 1), lab)], 1)
                    for lab in self._ray_frame_labels(pred_dict["valid_frames"])]
            end_points = [torch.cat(cols, 0)] * bs
        return end_points

    @torch.no_grad()
    def render_occupancy(self, pred_dict, directions=None, end_points=None, *, cameras=None, stride=4, tgt_bev_h,
                         tgt_bev_w, tgt_pc_range, img_metas=None, start_idx=0, batched_origin_points=None):
        """Occupancy evidence of the decoded volumes -> [bs, F, 2, Z, H, W] fp32, hit and free (ray_ops.ray_occupancy):
        how much softmax mass the marched rays put AT each voxel and how much BEYOND it (the ray passed through).
          directions / end_points: the listed rays, exactly those render_rays would hand to ray_argmax (the same origin,
              voxel mapping and nan_to_num); every marched ray contributes, whatever eval_within_grid later selects;
          cameras: camera indices or "all" -> the rays of render_cameras at `stride` are added (ray_ops.ray_occupancy_cam).
        At least one source; the two sources' grids are summed in torch.  vidar_amd.forecast.occupancy_grid turns the
        pair into an occupied / free / unseen answer."""
        listed = directions is not None or end_points is not None
        if not listed and cameras is None:
            raise ValueError("give directions, end_points or cameras")
        total = None
        if listed:
            end_points = self._listed_end_points(pred_dict, directions, end_points)
            rays = self._decode_rays(pred_dict, end_points, start_idx, tgt_bev_h, tgt_bev_w, tgt_pc_range, img_metas,
                                     batched_origin_points)
            total = self._evidence(self._march(ray_ops.ray_occupancy, rays))
        if cameras is not None:
            cam = self._evidence(ray_ops.ray_occupancy_cam(*args, **kw) for args, kw in self._camera_marches(
                pred_dict, img_metas, tgt_bev_h, tgt_bev_w, tgt_pc_range, cameras, stride))
            total = cam if total is None else total + cam
        return total

    @torch.no_grad()
    def measured_occupancy(self, pred_dict, gt_points, *, tgt_bev_h, tgt_bev_w, tgt_pc_range, img_metas=None,
                           start_idx=0, batched_origin_points=None):
        """Occupancy evidence of a MEASURED sweep -> [bs, F, 2, Z, H, W] fp32, hit and free (ray_ops.sweep_evidence):
        where the rays of `gt_points` returned and which voxels they passed on the way.  The rays are exactly those
        get_point_cloud_prediction decodes (the same origin, voxel mapping, nan_to_num and tindex), so the grids compare
        cell for cell with render_occupancy(end_points=gt_points); pred_dict only gives the grid its shape and frames.
        vidar_amd.forecast.occupancy_score holds the two against each other."""
        rays = self._decode_rays(pred_dict, gt_points, start_idx, tgt_bev_h, tgt_bev_w, tgt_pc_range, img_metas,
                                 batched_origin_points)
        return self._evidence(self._march(
            lambda sigma, origin, pts, tindex, step, K: ray_ops.sweep_evidence(origin, pts, tindex, rays.shape, step, K),
            rays))

    @torch.no_grad()
    def occupancy_at(self, pred_dict, points, *, extent=1.0, tgt_bev_h, tgt_bev_w, tgt_pc_range, img_metas=None,
                     start_idx=0, batched_origin_points=None):
        """The occupancy forecast at listed points (ray_ops.point_occupancy): for each point, how likely a return is within
        `extent` voxel units of it along the ray from the sensor (hit), and how likely the ray goes on past it (free).
        points: list[bs] of [N, >=4] in the layout of gt_points (xyz first, the frame label last); the rays are those
        get_point_cloud_prediction would decode for them (_decode_rays).
        -> list[bs] of [N, 2] (hit, free), row for row; two zeros for a point of a frame that is not predicted."""
        rays = self._decode_rays(pred_dict, points, start_idx, tgt_bev_h, tgt_bev_w, tgt_pc_range, img_metas,
                                 batched_origin_points)
        out = self._march(lambda *a: ray_ops.point_occupancy(*a, extent=extent), rays)
        return [o[:p.shape[0]] for o, p in zip(out, points)]

    @torch.no_grad()
    def render_occupancy_dense(self, pred_dict, *, extent=1.0, tgt_bev_h, tgt_bev_w, tgt_pc_range, img_metas=None,
                               start_idx=0, batched_origin_points=None):
        """Occupancy evidence of the decoded volumes without a ray set -> [bs, F, 2, Z, H, W] fp32, hit and free
        (ray_ops.voxel_occupancy): one ray per voxel, from the frame's origin through the voxel's centre.  The volumes and
        origins are those of every other decode (_decode_rays).  Reads like render_occupancy's result --
        vidar_amd.forecast.occupancy_grid -- but hit + free is a probability in [0, 1]: the softmax mass the ray still
        has when it reaches the voxel."""
        none = [pred_dict["next_bev_preds"].new_zeros((0, 4))] * pred_dict["next_bev_preds"].shape[-3]
        rays = self._decode_rays(pred_dict, none, start_idx, tgt_bev_h, tgt_bev_w, tgt_pc_range, img_metas,
                                 batched_origin_points)
        return self._evidence(ray_ops.voxel_occupancy(rays.volumes[b], rays.origin_grids[b], self.ray_grid_step,
                                                      self.ray_grid_num, extent) for b in range(len(rays.volumes)))
