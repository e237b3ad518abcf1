"""4d-occ ray-error metrics (L1 / AbsRel along GT rays) with the names and semantics of
projects/mmdet3d_plugin/bevformer/utils/eval_utils.py:8-225 (host-side evaluation code of the
reference, numpy).  The per-ray python loops of `_clamp` (:79-173) are vectorised over rays (six
passes over the sorted plane hits instead of a loop per ray); the nearest-neighbour match in
spherical coordinates (:199-203) runs on the gfx950 KNN kernel through chamferdist."""
from __future__ import annotations

import numpy as np
import torch

PC_RANGE = [-70.0, -70.0, -4.5, 70.0, 70.0, 4.5]     # eval_utils.py:8 (fixed, not the model's range)
MAX_VALUE = 1e8


def inside_volume(xyz):
    lo = np.array(PC_RANGE[:3]) - 0.02
    hi = np.array(PC_RANGE[3:]) + 0.02
    return np.logical_and(xyz >= lo, xyz <= hi).all(-1)


def _first_hit(start, direction, dist_to_planes):
    """first plane crossing (in ascending distance, distance >= -1e-4) whose point lies in the
    volume; -> (found [N] bool, point [N,3], distance [N])"""
    order = np.argsort(dist_to_planes, axis=0)
    n = start.shape[0]
    found = np.zeros(n, bool)
    point = np.full((n, 3), np.inf)
    dist = np.full(n, np.inf)
    cols = np.arange(n)
    for i in range(order.shape[0]):
        t = dist_to_planes[order[i], cols]
        inter = start + t[:, None] * direction
        hit = (~found) & (t + 1e-4 >= 0.0) & inside_volume(inter)
        point[hit] = inter[hit]
        dist[hit] = t[hit]
        found |= hit
    return found, point, dist


def _plane_distances(p, d, sign):
    out = []
    for a in range(3):
        da = sign * d[:, a]
        near0 = np.isclose(d[:, a], 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            out.append(np.where(near0, MAX_VALUE, (PC_RANGE[a] - p[:, a]) / da))
            out.append(np.where(near0, MAX_VALUE, (PC_RANGE[a + 3] - p[:, a]) / da))
    return np.stack(out)


def _clamp(points, origin):
    """clip rays origin->points to PC_RANGE (:79-173). -> (new_origin [N,3], points [N,3]);
    rays that miss the volume become points at infinity."""
    points = points.astype(float).copy()
    origin = origin.reshape(1, 3).astype(float)
    new_origin = np.zeros_like(points) + origin
    v = points - origin
    if (v == 0).all(1).any():
        raise RuntimeError("Origin and the end point should not be identical")
    l = np.sqrt((v ** 2).sum(1))
    d = v / l[:, None]
    intersects = np.ones(len(points), bool)
    if not inside_volume(origin)[0]:
        found, hit, t = _first_hit(np.repeat(origin, len(points), 0), d, _plane_distances(
            np.repeat(origin, len(points), 0), d, 1.0))
        intersects = found
        new_origin[found] = hit[found]
        beyond = found & (t > l)
        points[beyond] = new_origin[beyond]
    outside = intersects & ~inside_volume(points)
    if outside.any():
        found, hit, _ = _first_hit(points[outside], -d[outside], _plane_distances(points[outside], d[outside], -1.0))
        assert found.all()
        points[outside] = hit
    new_origin[~intersects] = np.inf
    points[~intersects] = np.inf
    return new_origin, points


def clamp(pcd_, org_, return_invalid_mask=False):
    pcd = pcd_.cpu().numpy().copy() if torch.is_tensor(pcd_) else np.array(pcd_, copy=True)
    org = org_.cpu().numpy().copy() if torch.is_tensor(org_) else np.array(org_, copy=True)
    inner = ((np.array(PC_RANGE[:3]) <= pcd) & (pcd <= np.array(PC_RANGE[3:]))).all(1)
    origins = np.zeros_like(pcd) + org.reshape(1, 3)
    if (~inner).any():
        o, p = _clamp(pcd[~inner], org.reshape(1, 3))
        pcd[~inner] = p.astype(float)
        origins[~inner] = o
    invalid = np.isinf(pcd).all(1) | np.isnan(pcd).all(1)
    if return_invalid_mask:
        return origins, pcd, invalid
    return origins[~invalid], pcd[~invalid]


def spherical_projection(pcd):
    x, y, z = pcd.T
    return np.arctan2(x, y), np.arctan2(z, y), np.sqrt(x * x + y * y + z * z)


def compute_ray_errors(pred_pcd, gt_pcd, origin, device, return_interpolated_pcd=False, savename="",
                       chamfer=None):
    """-> (l1_error, absrel_error) averaged over GT rays (:185-225).  `chamfer` defaults to the HIP
    ChamferDistance; tests inject a CPU implementation."""
    if chamfer is None:
        from ...third_lib.chamferdist import ChamferDistance
        chamfer = ChamferDistance()
    theta_hat, phi_hat, d_hat = spherical_projection(pred_pcd - origin[None, :])
    theta, phi, d = spherical_projection(gt_pcd - origin[None, :])
    mh, m = d_hat > 1e-2, d > 1e-2
    theta_hat, phi_hat, d_hat, pred_pcd = theta_hat[mh], phi_hat[mh], d_hat[mh], pred_pcd[mh]
    theta, phi, d, gt_pcd = theta[m], phi[m], d[m], gt_pcd[m]
    count = theta.shape[0]
    ps = np.stack([theta_hat, phi_hat, np.ones_like(theta_hat)], 1)
    gs = np.stack([theta, phi, np.ones_like(theta)], 1)
    _, info = chamfer(torch.from_numpy(ps[None]).float().to(device), torch.from_numpy(gs[None]).float().to(device),
                      reverse=True, reduction="mean")
    pred_idx = info[1].cpu().numpy()
    v = gt_pcd - origin[None, :]
    unit = v / np.sqrt((v ** 2).sum(1, keepdims=True))
    interp = origin[None, :] + d_hat[pred_idx].T * unit
    if return_interpolated_pcd:
        return interp
    g_origin, g_pcd, invalid = clamp(gt_pcd, origin, return_invalid_mask=True)
    _, p_pcd, _ = clamp(interp, origin, return_invalid_mask=True)
    keep = ~invalid
    g_pcd, p_pcd, g_origin = g_pcd[keep], p_pcd[keep], g_origin[keep]
    dc = np.sqrt(((g_pcd - g_origin) ** 2).sum(1))
    valid = dc > 0.01
    eucl = np.sqrt(((g_pcd[valid] - p_pcd[valid]) ** 2).sum(1))
    return eucl.sum() / count, (eucl / dc[valid]).sum() / count


# ---- the same metric on the device (csrc/ray_eval.hip) ------------------------------------------------------------------
_device_metrics = None      # None: follow VIDAR_DEVICE_METRICS


def set_device_metrics(on):
    """Route ViDAR.forward_test's metric tail (chamfer distance, l1_error, absrel_error) through the device path: one
    chamfer call, one ray-error call and one host read per batch.  Off by default; `None` returns the decision to the
    environment variable VIDAR_DEVICE_METRICS.  -> the previous setting"""
    global _device_metrics
    prev, _device_metrics = _device_metrics, (None if on is None else bool(on))
    return prev


def device_metrics():
    if _device_metrics is not None:
        return _device_metrics
    import os
    return os.environ.get("VIDAR_DEVICE_METRICS", "0") not in ("", "0")


# ---- the occupancy score (csrc/occ_score.hip; vidar_amd.forecast.occupancy_score) --------------------------------------
_occupancy_metrics = None   # None: follow VIDAR_OCC_METRICS
_occupancy_options = {}
_OCC_OPTIONS = ("thresholds", "min_evidence", "min_meas_evidence", "min_hits", "bins")


def set_occupancy_metrics(on, source="rays", **options):
    """Make ViDAR.forward_test also score the occupancy forecast against the measured sweep: the predicted evidence of the
    very rays it decodes, the measured evidence of those rays (ViDARHeadBase.measured_occupancy) and
    forecast.occupancy_score's table, whose columns join every frame.k dictionary as additive `occ.*` entries.
    source: where the PREDICTED evidence comes from -- "rays": the measured sweep's own ray directions
    (render_occupancy(end_points=gt_points)); "dense": one ray per voxel (render_occupancy_dense), the grid a user of
    ViDAR.forecast(occupancy="dense") gets, whose evidence is a probability: min_evidence is then a floor under the mass
    the ray still has at the voxel.  The measured side is the same under both.
    options: thresholds, min_evidence, min_meas_evidence, min_hits, bins -- occupancy_score's keywords; what is not given
    keeps occupancy_score's default.  Off by default; `None` returns the decision to the environment variable
    VIDAR_OCC_METRICS.  -> the previous setting"""
    global _occupancy_metrics, _occupancy_options
    unknown = sorted(set(options) - set(_OCC_OPTIONS))
    if unknown:
        raise TypeError(f"set_occupancy_metrics: unknown option {unknown[0]!r}; the options are {', '.join(_OCC_OPTIONS)}")
    if source not in ("rays", "dense"):
        raise ValueError(f'set_occupancy_metrics: source must be "rays" or "dense", not {source!r}')
    prev, _occupancy_metrics = _occupancy_metrics, (None if on is None else bool(on))
    _occupancy_options = {k: v for k, v in options.items() if v is not None}
    if source != "rays":
        _occupancy_options["source"] = source      # ViDAR._occupancy_table takes it out before occupancy_score sees them
    return prev


def occupancy_metrics():
    """None while the occupancy score is off, else the keywords forward_test hands to forecast.occupancy_score"""
    on = _occupancy_metrics
    if on is None:
        import os
        on = os.environ.get("VIDAR_OCC_METRICS", "0") not in ("", "0")
    return dict(_occupancy_options) if on else None


def ray_errors_device(pred, pred_start, gt, gt_start, origin, max_gt, *, return_per_ray=False):
    """compute_ray_errors for S segments -- (sample, frame) pairs -- in one call, on the device, in fp64.
    pred [P,3] / gt [G,3] f32 grouped by segment, pred_start / gt_start [S+1] i32 DEVICE tensors (segment s owns rows
    start[s] .. start[s+1]; they are never read back), origin [S,3] f32, max_gt: a host bound on the longest ground-truth
    segment (it sizes the grid only; a cloud's padded length will do).
    -> [S,3] f64 device tensor (sum of L1, sum of AbsRel, count): l1_error = [:, 0] / [:, 2], absrel_error = [:, 1] / [:, 2].
    A segment with counted rays and no kept prediction gives NaN (compute_ray_errors raises there).
    return_per_ray: -> (sums, dict(nn_idx [G] i32 -- the row relative to the segment's start, -1 for an uncounted ray --,
    ray_err [G,2] f64, interp [G,3] f64 -- compute_ray_errors(..., return_interpolated_pcd=True), NaN where nn_idx is -1 --,
    partial [S,tiles,3] f64)).  There is no CPU path."""
    from ..._lib import check, lib, ptr, stream_of
    tensors = (pred, pred_start, gt, gt_start, origin)
    if not all(torch.is_tensor(t) and t.is_cuda for t in tensors):
        raise RuntimeError("ray_errors_device needs device tensors: the product has no CPU path "
                           "(compute_ray_errors is the host form)")
    if any(t.device != pred.device for t in tensors):
        raise RuntimeError("ray_errors_device: all tensors must live on one device")
    S = origin.shape[0]
    if (pred.dtype, gt.dtype, origin.dtype) != (torch.float32,) * 3 or (pred_start.dtype, gt_start.dtype) != (torch.int32,) * 2:
        raise TypeError("ray_errors_device: pred / gt / origin must be float32 and the start tables int32")
    if pred.dim() != 2 or pred.shape[1] != 3 or gt.dim() != 2 or gt.shape[1] != 3 or tuple(origin.shape) != (S, 3) \
            or tuple(pred_start.shape) != (S + 1,) or tuple(gt_start.shape) != (S + 1,):
        raise ValueError("ray_errors_device: pred [P,3], gt [G,3], origin [S,3], pred_start / gt_start [S+1]")
    pred, gt, origin = pred.contiguous(), gt.contiguous(), origin.contiguous()
    pred_start, gt_start = pred_start.contiguous(), gt_start.contiguous()
    P, G, max_gt = pred.shape[0], gt.shape[0], int(max_gt)
    tiles = (max(max_gt, 0) + 255) // 256
    f64 = dict(dtype=torch.float64, device=pred.device)
    partial = torch.zeros(S, tiles, 3, **f64) if S == 0 or G == 0 else torch.empty(S, tiles, 3, **f64)
    per_ray = None
    if return_per_ray:
        per_ray = dict(nn_idx=torch.full((G,), -1, dtype=torch.int32, device=pred.device),
                       ray_err=torch.zeros(G, 2, **f64), interp=torch.full((G, 3), float("nan"), **f64), partial=partial)
    import ctypes
    nbytes = ctypes.c_int64(0)
    check(lib().vidar_ray_eval_workspace_bytes(P, ctypes.addressof(nbytes)), "vidar_ray_eval_workspace_bytes")
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=pred.device) if nbytes.value else None
    check(lib().vidar_ray_eval_f64(ptr(pred), ptr(pred_start), ptr(gt), ptr(gt_start), ptr(origin), ptr(partial),
                                   ptr(per_ray and per_ray["nn_idx"]), ptr(per_ray and per_ray["ray_err"]),
                                   ptr(per_ray and per_ray["interp"]), P, G, S, max_gt, ptr(ws), nbytes.value,
                                   stream_of(pred)), "vidar_ray_eval_f64")
    sums = partial.sum(1)
    return (sums, per_ray) if return_per_ray else sums


def forecast_metrics_device(pred, gt, frame, origin, pc_range):
    """The forecasting metrics of every (sample, frame) segment without a host read.
    pred / gt [bs,N,3]: the rendered points of the predicted and of the ground-truth depth of every ray, frame [bs,N] int64:
    the frame a ray belongs to, -1 for a ray that takes no part (its points may hold anything), origin [bs,F,3]
    (dense_heads get_rendered_rays), pc_range: the model's range, which crops the chamfer distance.
    -> [bs,F,4] f64 device tensor: chamfer distance (compute_chamfer_distance_inner), l1_error, absrel_error
    (compute_ray_errors) and the number of rays of the segment."""
    from . import e2e_predictor_utils
    bs, N = frame.shape
    F_ = origin.shape[1]
    S = bs * F_
    # chamfer distance inside the model's range: segment (b, f) sees cloud b under the mask frame == f
    in_seg = (frame.unsqueeze(1) == torch.arange(F_, device=frame.device).view(1, F_, 1)).reshape(S, N)
    expand = lambda x: x.unsqueeze(1).expand(bs, F_, N, 3).reshape(S, N, 3)
    cd = e2e_predictor_utils.chamfer_inner_device(expand(pred), in_seg, expand(gt), in_seg, pc_range)
    # ray errors: rows sorted by segment (the rays that take no part last, owned by no segment), starts found on the device
    key = torch.where(frame >= 0, torch.arange(bs, device=frame.device).view(bs, 1) * F_ + frame,
                      torch.full_like(frame, S)).reshape(-1)
    key, order = torch.sort(key, stable=True)
    start = torch.searchsorted(key, torch.arange(S + 1, device=key.device)).to(torch.int32)
    take = lambda x: x.reshape(-1, 3).float()[order]
    sums = ray_errors_device(take(pred), start, take(gt), start, origin.reshape(S, 3).float(), N)
    rows = (start[1:] - start[:-1]).to(sums.dtype)
    # a segment without rays scores 0 (the host path skips it); rays but no counted one is 0 / 0, as on the host
    err = torch.where(rows.unsqueeze(1) > 0, sums[:, :2] / sums[:, 2:3], torch.zeros_like(sums[:, :2]))
    return torch.cat([cd.to(sums.dtype).unsqueeze(1), err, rows.unsqueeze(1)], 1).view(bs, F_, 4)
