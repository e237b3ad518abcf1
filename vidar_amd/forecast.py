"""A forecast without ground truth: the geometry and the pictures around `ViDAR.forecast` / `ViDARHeadBase.render_rays`.

  pix2vox        camera pixel -> voxel coordinates of a predicted volume (input of ray_ops.ray_argmax_cam)
  lidar_pattern  unit directions of a spinning LiDAR, for a sweep nobody measured
  bev_image      bird's-eye picture of labelled points; a restatement of the reference's `_dbg_draw_pc_function`
                 (utils/e2e_predictor_utils.py:188-224), NOT a pixel copy of what matplotlib renders
  depth_overlay  per-pixel depth laid over the camera frame
  confidence_mask / confidence_overlay  which rays pass a threshold on ray_ops.ray_stats' statistics; p_max as a picture
  occupancy_grid / occupancy_bev  occupied / free / unseen voxels from ray_ops.ray_occupancy's evidence; as a picture
  occupancy_score / occupancy_metrics  the predicted evidence held against a measured sweep's (ray_ops.sweep_evidence):
                 counts per (sample, frame) on the device (csrc/occ_score.hip), then IoU / precision / recall / calibration
torch + PIL only; occupancy_score is the one function here that launches a kernel of its own."""
from __future__ import annotations

import math
import os

import numpy as np
import torch

LABEL_COLOURS = ((0, 0, 230), (219, 112, 147), (255, 0, 0))      # detectors/vidar.py:523-525: prediction, ground truth, ego


def pix2vox(lidar2img, pc_range, bev_h, bev_w, pillar_num, align=None):
    """[F, C, 4, 4] fp32 maps of the homogeneous pixel (u*d, v*d, d, 1) to voxel coordinates of each frame's volume.

    lidar2img [C, 4, 4]: the CURRENT frame's camera matrices (img_metas[...]["lidar2img"]), affine (last row 0 0 0 1).
    align [F, 4, 4] or None: per frame, the row-vector transform (p_row @ M) from the frame's own LiDAR coordinates to
    the coordinates its volume is predicted in -- what the head applies to the ground-truth rays of that frame
    (ViDARHeadV1._get_reference_gt_points); None = identity for one frame.
    The metric -> voxel map is e2e_predictor_utils.coords_to_voxel_grids.  Everything is composed in fp64 and rounded to
    fp32 once.

    ASSUMPTION (rigid rig): the cameras are fixed to the ego vehicle, so the current frame's lidar2img also describes
    where the cameras sit in every FUTURE frame's own LiDAR coordinates; the depth of future frame f is therefore what
    the rig would see from where the vehicle will be, not from where it is now."""
    l2i = np.asarray([np.asarray(m, dtype=np.float64) for m in lidar2img], dtype=np.float64)
    if l2i.ndim != 3 or l2i.shape[1:] != (4, 4):
        raise ValueError("lidar2img must be [C, 4, 4]")
    if not np.allclose(l2i[:, 3], [0.0, 0.0, 0.0, 1.0]):
        raise ValueError("lidar2img must be affine (last row 0 0 0 1)")
    align = np.eye(4)[None] if align is None else np.asarray(align, dtype=np.float64)
    pc = [float(v) for v in pc_range]
    to_vox = np.eye(4)
    for axis, n in enumerate((bev_w, bev_h, pillar_num)):
        to_vox[axis, axis] = n / (pc[axis + 3] - pc[axis])
        to_vox[axis, 3] = -pc[axis] * n / (pc[axis + 3] - pc[axis])
    inv = np.linalg.inv(l2i)                                          # [C, 4, 4] pixel -> LiDAR, column vectors
    out = np.einsum("ij,fjk,ckl->fcil", to_vox, np.transpose(align, (0, 2, 1)), inv)
    out[..., 3, :] = [0.0, 0.0, 0.0, 1.0]
    return torch.from_numpy(out.astype(np.float32))


def lidar_pattern(beams=32, azimuths=1080, elevation_deg=(-30.67, 10.67)):
    """Unit directions [beams * azimuths, 3] (x forward, y left, z up) of a spinning LiDAR: `beams` elevations evenly
    spaced over `elevation_deg` (both ends included), `azimuths` evenly spaced turns in [-pi, pi), beam-major.

    The defaults are the Velodyne HDL-32E's figures (32 beams over -30.67 .. +10.67 degrees; 1080 columns a turn is about
    its horizontal resolution at 10 Hz) as RECALLED from its data sheet, not pinned against a file of this repository
    or the nuScenes sweeps: they make a plausible sweep, not that sensor's calibrated beam table."""
    if beams < 1 or azimuths < 1:
        raise ValueError("beams and azimuths must be >= 1")
    lo, hi = (math.radians(float(e)) for e in elevation_deg)
    el = torch.linspace(lo, hi, beams, dtype=torch.float64)
    az = -math.pi + torch.arange(azimuths, dtype=torch.float64) * (2.0 * math.pi / azimuths)
    el, az = el[:, None], az[None, :]
    d = torch.stack([el.cos() * az.cos(), el.cos() * az.sin(), el.sin().expand(beams, azimuths)], -1).reshape(-1, 3)
    d = d / d.norm(dim=1, keepdim=True)
    return d.float()


def _cross(img, row, col, arm, colour):
    size = img.shape[0]
    k = torch.arange(-arm, arm + 1, device=img.device)
    for rr, cc in ((row + k, col + k), (row + k, col - k)):
        ok = (rr >= 0) & (rr < size) & (cc >= 0) & (cc < size)
        img[rr[ok], cc[ok]] = colour


def _to_pixel(xy, size_px, limit_m):
    """metric (x, y) fp64 -> (row, col, inside): a square of +-limit_m, x to the right, y up; the pixel is the floor of
    the position in pixel units, so the window is closed at -limit_m and open at +limit_m; NaN is outside."""
    col = torch.floor((xy[..., 0] + limit_m) / (2.0 * limit_m) * size_px)
    up = torch.floor((xy[..., 1] + limit_m) / (2.0 * limit_m) * size_px)
    inside = (col >= 0) & (col < size_px) & (up >= 0) & (up < size_px)        # False for NaN
    col = torch.where(inside, col, torch.zeros_like(col)).long()
    row = size_px - 1 - torch.where(inside, up, torch.zeros_like(up)).long()
    return row, col, inside


def bev_image(points, labels, centre=None, size_px=720, limit_m=40):
    """Bird's-eye picture [size_px, size_px, 3] uint8 of points [N, >=2] (metres) coloured by labels [N] (indices into
    LABEL_COLOURS) on white ground: one pixel per point, a later point paints over an earlier one, NaN points and points
    outside the +-limit_m window are skipped; then a diagonal cross in label 0's colour at every `centre` [M, >=2] and a
    red one at (0, 0).  A restatement of the reference's matplotlib scatter (its window, its colours, its markers' places
    and its draw order), not a copy of its pixels."""
    dev = points.device
    n = points.shape[0]
    colours = torch.tensor(LABEL_COLOURS, dtype=torch.uint8, device=dev)
    img = torch.full((size_px * size_px, 3), 255, dtype=torch.uint8, device=dev)
    if n:
        row, col, inside = _to_pixel(points[:, :2].double(), size_px, float(limit_m))
        pix = (row * size_px + col)[inside]
        order = torch.arange(n, device=dev)[inside]
        # the last point of every pixel: max of the point index (index_put_ with duplicate pixels has no defined winner)
        last = torch.full((size_px * size_px,), -1, dtype=torch.int64, device=dev)
        last = last.scatter_reduce(0, pix, order, reduce="amax", include_self=True)
        hit = last >= 0
        img[hit] = colours[labels.to(dev).long()[last[hit]]]
    img = img.view(size_px, size_px, 3)
    arm = max(2, size_px // 64)
    marks = [] if centre is None else [(c, colours[0]) for c in centre.to(dev).double().view(-1, centre.shape[-1])]
    marks.append((torch.zeros(2, dtype=torch.float64, device=dev), colours[2]))
    for xy, colour in marks:
        row, col, inside = _to_pixel(xy[:2], size_px, float(limit_m))
        if bool(inside):
            _cross(img, int(row), int(col), arm, colour)
    return img


def colour_table(device="cpu"):
    """[256, 3] uint8, a piecewise-linear blue - cyan - green - yellow - red ramp in integer arithmetic"""
    i = torch.arange(256, dtype=torch.int64, device=device)
    ch = [(384 - (4 * i - peak).abs()).clamp(0, 255) for peak in (768, 512, 256)]
    return torch.stack(ch, 1).to(torch.uint8)


def depth_overlay(depth, frame_u8, near=1.0, far=60.0, alpha=160):
    """depth [Hs, Ws] (metres, 0 or NaN = no return) over frame_u8 [H, W, 3] uint8 -> [H, W, 3] uint8.

    The stride is s = ceil(H / Hs) (it must reproduce Hs and Ws): image pixel (y, x) takes depth[y // s, x // s].  Colour
    index = clamp(floor((far - d) / (far - near) * 255 + 0.5), 0, 255) into colour_table (near = red end, computed in
    fp64); out = (alpha * colour + (255 - alpha) * image + 127) // 255 in integers where there is a return, the image
    elsewhere."""
    if not far > near:
        raise ValueError("alpha must be 0..255 and far > near")
    return _ramp_overlay(depth, frame_u8, alpha, lambda d: (far - d) / (far - near))


def _ramp_overlay(value, frame_u8, alpha, unit):
    """depth_overlay's strided grid, colour ramp and blend; `unit` maps the fp64 values to [0, 1] of the ramp (1 = red)"""
    H, W = frame_u8.shape[:2]
    Hs, Ws = value.shape
    s = -(-H // Hs)
    if s < 1 or -(-H // s) != Hs or -(-W // s) != Ws:
        raise ValueError(f"depth {tuple(value.shape)} is no strided grid of a {H} x {W} frame")
    a = int(alpha)
    if not 0 <= a <= 255:
        raise ValueError("alpha must be 0..255 and far > near")
    dev = frame_u8.device
    d = value.to(dev).double()
    idx = torch.floor(unit(d) * 255.0 + 0.5)
    live = (d > 0) & torch.isfinite(d)
    idx = torch.where(live, idx, torch.zeros_like(idx)).clamp(0, 255).long()
    ys = torch.arange(H, device=dev) // s
    xs = torch.arange(W, device=dev) // s
    colour = colour_table(dev)[idx][ys][:, xs].to(torch.int32)           # [H, W, 3]
    live = live[ys][:, xs]
    img = frame_u8.to(torch.int32)
    mixed = (a * colour + (255 - a) * img + 127) // 255
    return torch.where(live[..., None], mixed, img).to(torch.uint8)


def confidence_mask(stats, min_prob=None, max_rms=None):
    """stats [..., 4] = (p_max, mean, rms, entropy) of ray_ops.ray_stats -> bool [...]: True where the ray is kept, i.e.
    p_max >= min_prob and rms <= max_rms for each threshold that is given (rms in the unit of `stats`: metres for what
    the head and ViDAR.forecast return).  A NaN statistic fails the threshold it is held against; with both thresholds
    None every ray is kept, NaN or not.  Pure torch, any device."""
    keep = torch.ones(stats.shape[:-1], dtype=torch.bool, device=stats.device)
    if min_prob is not None:
        keep = keep & (stats[..., 0] >= float(min_prob))
    if max_rms is not None:
        keep = keep & (stats[..., 2] <= float(max_rms))
    return keep


def confidence_overlay(p_max, frame_u8, alpha=160):
    """p_max [Hs, Ws] (0 or NaN = no return) over frame_u8 [H, W, 3] uint8 -> [H, W, 3] uint8: depth_overlay's strided
    grid, integer colour ramp and blend with the colour index clamp(floor(p * 255 + 0.5), 0, 255), so that p = 1 is the
    red end and p -> 0 the blue one."""
    return _ramp_overlay(p_max, frame_u8, alpha, lambda p: p)


UNSEEN_COLOUR = (176, 196, 222)      # occupancy_bev: a column without a seen voxel


def occupancy_grid(hit, free, min_evidence=0.5):
    """hit, free [..., Z, H, W] of ray_ops.ray_occupancy (the softmax mass the marched rays put AT a voxel / BEYOND it)
    -> (occ, evidence), both of that shape: evidence = hit + free; occ = hit / evidence where evidence >= min_evidence,
    NaN elsewhere -- never seen, or occluded (every ray that came by had already spent its mass).
    Evidence is counted in waypoints: 1.0 is one waypoint of one ray wholly attributed to the voxel and certainly not
    occluded; half of one is the default floor.  The grids of ray_ops.voxel_occupancy (one ray per voxel) read the same
    way, with the evidence a probability in [0, 1] -- the softmax mass the voxel's own ray still has when it gets there --
    and the floor a bound under that.  min_evidence is a parameter of the answer, not a tolerance.  A NaN
    evidence fails the floor (and 0 / 0 under a floor of 0 is NaN as well).  Pure torch, any device."""
    evidence = hit + free
    occ = torch.where(evidence >= float(min_evidence), hit / evidence, torch.full_like(evidence, float("nan")))
    return occ, evidence


OCC_FIXED_COLUMNS = ("n_pred", "n_meas", "n_both", "n_occ", "brier")
OCC_THRESHOLDS, OCC_BINS = (0.25, 0.5), 10      # the defaults of occupancy_score and of what reads its table


def _thresholds(thresholds):
    t = [float(v) for v in (thresholds if hasattr(thresholds, "__iter__") else (thresholds,))]
    if not 1 <= len(t) <= 8 or any(math.isnan(v) for v in t):
        raise ValueError("occupancy thresholds: 1 to 8 numbers, none of them NaN")
    return t


def occupancy_columns(thresholds=OCC_THRESHOLDS, bins=OCC_BINS):
    """names of the columns of occupancy_score's table, in order: n_pred, n_meas, n_both, n_occ, brier, then tp@t, fp@t,
    fn@t per threshold t (printed with %g) and cnt.b, pos.b per reliability bin b"""
    cols = list(OCC_FIXED_COLUMNS)
    for t in _thresholds(thresholds):
        cols += [f"tp@{t:g}", f"fp@{t:g}", f"fn@{t:g}"]
    for b in range(int(bins)):
        cols += [f"cnt.{b}", f"pos.{b}"]
    return cols


def occupancy_score(pred_evidence, meas_evidence, thresholds=OCC_THRESHOLDS, min_evidence=0.5, min_meas_evidence=0.5,
                    min_hits=0.125, bins=OCC_BINS):
    """Score a predicted occupancy evidence against a measured one, on the device, without a host read.
    pred_evidence / meas_evidence [..., 2, Z, H, W] (or [S, 2, V]) fp32 device tensors of one shape: hit and free of
    ViDARHeadBase.render_occupancy / ray_ops.ray_occupancy and of ViDARHeadBase.measured_occupancy / ray_ops.sweep_evidence.
    Per voxel (fp32): ev = hit + free on both sides, o_p = hit_p / ev_p; the voxel is scored where
    ev_p >= min_evidence and ev_m >= min_meas_evidence (both grids speak), and its label is y = hit_m >= min_hits -- a
    return was measured in the cell; the cell that holds a lone return always receives at least 1/8 of it.
    -> fp64 device table [..., 5 + 3 T + 2 bins] with the leading dimensions of the input and the columns of
    occupancy_columns: exact counts, and brier = sum (o_p - y)^2 in a fixed order (include/vidar_hip.h:
    vidar_occ_score_f32).  occupancy_metrics turns it into IoU / precision / recall / coverage / calibration.
    There is no CPU path."""
    import ctypes
    from ._lib import check, lib, ptr, stream_of
    if not (torch.is_tensor(pred_evidence) and torch.is_tensor(meas_evidence) and pred_evidence.is_cuda
            and meas_evidence.device == pred_evidence.device):
        raise RuntimeError("occupancy_score needs two tensors on one GPU: the product has no CPU path")
    if pred_evidence.shape != meas_evidence.shape:
        raise ValueError(f"occupancy_score: the grids differ in shape, {tuple(pred_evidence.shape)} against "
                         f"{tuple(meas_evidence.shape)}")
    tail = 2 if pred_evidence.dim() == 3 else 4
    if pred_evidence.dim() < 3 or pred_evidence.shape[-tail] != 2:
        raise ValueError("occupancy_score: evidence must be [..., 2, Z, H, W] or [S, 2, V], hit and free")
    if (pred_evidence.dtype, meas_evidence.dtype) != (torch.float32, torch.float32):
        raise TypeError("occupancy_score: evidence must be float32")
    th = _thresholds(thresholds)
    T, B = len(th), int(bins)
    lead = tuple(pred_evidence.shape[:-tail])
    S, V = math.prod(lead), math.prod(pred_evidence.shape[-tail + 1:])
    pred, meas = pred_evidence.contiguous(), meas_evidence.contiguous()
    ncols = 5 + 3 * T + 2 * B
    nbytes = ctypes.c_int64(0)
    check(lib().vidar_occ_score_workspace_bytes(S, V, T, B, ctypes.addressof(nbytes)), "occupancy_score")
    empty = S == 0 or V == 0
    table = (torch.zeros if empty else torch.empty)((S, ncols), dtype=torch.float64, device=pred.device)
    ws = torch.empty(max(nbytes.value, 8), dtype=torch.uint8, device=pred.device)
    th_host = (ctypes.c_float * T)(*th)
    check(lib().vidar_occ_score_f32(ptr(pred), ptr(meas), ctypes.addressof(th_host), ptr(table), S, V, T, B,
                                    float(min_evidence), float(min_meas_evidence), float(min_hits), ptr(ws),
                                    nbytes.value, stream_of(pred)), "occupancy_score")
    return table.view(*lead, ncols)


def _ratio(num, den):
    return float(num) / float(den) if float(den) != 0.0 else float("nan")


def occupancy_metrics(table, thresholds=OCC_THRESHOLDS, bins=OCC_BINS):
    """occupancy_score's table [..., 5 + 3 T + 2 bins] (a tensor on any device, or anything numpy reads) summed over its
    leading dimensions -> dict of host numbers:
      n_pred, n_meas, n_both, n_occ;  coverage = n_both / n_meas;  brier = brier sum / n_both;
      thresholds [T];  tp, fp, fn, iou = tp / (tp + fp + fn), precision = tp / (tp + fp), recall = tp / (tp + fn), each [T];
      reliability: dict(cnt [bins], freq [bins] = pos / cnt) -- of the voxels the forecast puts in a bin of o_p, how many
      held a return.
    NaN where a denominator is 0.  Ratios of counts: a table whose every entry was divided by one number gives the same."""
    th = _thresholds(thresholds)
    T, B = len(th), int(bins)
    t = table.detach().double().cpu().numpy() if torch.is_tensor(table) else np.asarray(table, dtype=np.float64)
    if t.shape[-1] != 5 + 3 * T + 2 * B:
        raise ValueError(f"occupancy_metrics: {t.shape[-1]} columns, {5 + 3 * T + 2 * B} expected for {T} thresholds and "
                         f"{B} bins")
    t = t.reshape(-1, t.shape[-1]).sum(0)
    out = {k: float(t[i]) for i, k in enumerate(OCC_FIXED_COLUMNS[:4])}
    out["coverage"] = _ratio(t[2], t[1])
    out["brier"] = _ratio(t[4], t[2])
    out["thresholds"] = th
    tp, fp, fn = (t[5 + i:5 + 3 * T:3] for i in range(3))
    out["tp"], out["fp"], out["fn"] = ([float(v) for v in x] for x in (tp, fp, fn))
    out["iou"] = [_ratio(a, a + b + c) for a, b, c in zip(tp, fp, fn)]
    out["precision"] = [_ratio(a, a + b) for a, b in zip(tp, fp)]
    out["recall"] = [_ratio(a, a + c) for a, c in zip(tp, fn)]
    cnt, pos = t[5 + 3 * T::2], t[6 + 3 * T::2]
    out["reliability"] = dict(cnt=[float(v) for v in cnt], freq=[_ratio(p, c) for p, c in zip(pos, cnt)])
    return out


def occupancy_bev(occ, size_px=None):
    """occ [Z, H, W] of occupancy_grid (NaN = unseen) -> bird's-eye picture [size_px, size_px, 3] uint8 ([H, W, 3] for
    size_px None): per column the max over Z among the seen voxels, as the integer grey
    255 - clamp(floor(occ * 255 + 0.5), 0, 255) (free white, occupied black); UNSEEN_COLOUR where no voxel of the column
    was seen.  bev_image's orientation: x to the right, y up (row 0 is y = H - 1).  A size_px other than H / W picks
    the nearest cell: picture pixel (r, c) shows cell (y, x) = (((size_px - 1 - r) * H) // size_px, (c * W) // size_px)."""
    if occ.dim() != 3:
        raise ValueError("occ must be [Z, H, W]")
    seen = ~torch.isnan(occ)
    top = torch.where(seen, occ, torch.full_like(occ, -float("inf"))).max(0)[0].double()
    any_seen = seen.any(0)
    level = torch.floor(torch.where(any_seen, top, torch.zeros_like(top)) * 255.0 + 0.5).clamp(0, 255).long()
    grey = (255 - level).to(torch.uint8)
    unseen = torch.tensor(UNSEEN_COLOUR, dtype=torch.uint8, device=occ.device)
    img = torch.where(any_seen[..., None], grey[..., None].expand(-1, -1, 3), unseen.expand(*grey.shape, 3))
    H, W = grey.shape
    rows, cols = (H, W) if size_px is None else (int(size_px), int(size_px))
    if rows < 1:
        raise ValueError("size_px must be >= 1")
    ys = ((rows - 1 - torch.arange(rows, device=occ.device)) * H) // rows
    xs = (torch.arange(cols, device=occ.device) * W) // cols
    return img[ys][:, xs].contiguous()


def save_png(img_u8, path):
    """[H, W, 3] uint8 tensor -> PNG file (its directory is created)"""
    from PIL import Image
    root = os.path.dirname(str(path))
    if root:
        os.makedirs(root, exist_ok=True)
    Image.fromarray(img_u8.cpu().numpy(), "RGB").save(str(path))


def sweep_bev(pred, gt=None, centre=None, size_px=720, limit_m=40):
    """the reference's `_viz_pcd` (detectors/vidar.py:521-536): the prediction as label 0, then the ground truth as
    label 1 painted over it, the sensor origin as the centre cross"""
    pts = pred[:, :3] if gt is None else torch.cat([pred[:, :3], gt[:, :3].to(pred.device)], 0)
    lab = torch.zeros(pts.shape[0], dtype=torch.int64, device=pts.device)
    lab[pred.shape[0]:] = 1
    return bev_image(pts, lab, centre, size_px, limit_m)
