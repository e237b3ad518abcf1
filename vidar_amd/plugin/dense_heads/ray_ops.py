"""Autograd wrappers of the fused head ray-march kernels (csrc/ray_march.hip).  They replace the
tensor programs inside ViDARHeadBase (dense_heads/vidar_head_base.py:420-509, :575-592, :697-731,
:754-773); per-ray results come back and the (cheap) weighting / reductions stay in torch.
K = ray_grid_num is any value in 1..max_k(); 512 (K_SAMPLES, the released configs) runs the register-resident
kernels, every other value the streamed ones."""
from __future__ import annotations

import contextlib
import ctypes

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from ..._lib import lib, check, ptr, stream_of, workspace, TIMER
from ... import deterministic

K_SAMPLES = 512


def max_k():
    return lib().vidar_ray_max_k()


@contextlib.contextmanager
def force_streamed(on=True):
    """Test / benchmark hook: K == 512 runs the streamed kernels too inside the block (same bits)."""
    was = lib().vidar_ray_force_streamed(bool(on))
    try:
        yield
    finally:
        lib().vidar_ray_force_streamed(was)


def _f(t):
    return t.float().contiguous()


def _dims(sigma, pts):
    F_, Z, Y, X = sigma.shape
    return F_, pts.shape[0], Z, Y, X


def _ray_bwd(ctx, grad, entry, name, per_ray):
    """d loss / d sigma of the three ray losses: `entry` on what the forward saved (the rays and lse / aux) and the
    per-ray gradient; `per_ray`: fp32 values moved per ray, for the span's byte count"""
    sigma, origin, pts, tindex, saved = ctx.saved_tensors
    step, K = ctx.cfg
    F_, R, Z, Y, X = _dims(sigma, pts)
    g = torch.empty_like(sigma)
    deterministic.sync()
    ws, wsp, wsn = workspace(lib().vidar_ray_bwd_workspace_bytes, F_, Z, Y, X, like=sigma)
    with TIMER.span(name, 4 * (2 * sigma.numel() + R * per_ray)):
      check(entry(ptr(sigma), ptr(origin), ptr(pts), ptr(tindex), ptr(saved), ptr(_f(grad)), ptr(g),
                  F_, R, Z, Y, X, K, step, wsp, wsn, stream_of(sigma)), name)
    return g


class _RayCE(Function):
    @staticmethod
    def forward(ctx, sigma, origin, gt, tindex, step, K):
        sigma, origin, gt, tindex = _f(sigma), _f(origin), _f(gt), _f(tindex)
        F_, R, Z, Y, X = _dims(sigma, gt)
        ce = torch.empty(R, device=sigma.device); lse = torch.empty_like(ce); valid = torch.empty_like(ce)
        with TIMER.span("ray_ce_fwd", 4 * (sigma.numel() + R * 7)):
          check(lib().vidar_ray_ce_fwd_f32(ptr(sigma), ptr(origin), ptr(gt), ptr(tindex), ptr(ce),
                                         ptr(lse), ptr(valid), F_, R, Z, Y, X, K, step, stream_of(sigma)), "ray_ce_fwd")
        ctx.save_for_backward(sigma, origin, gt, tindex, lse)
        ctx.cfg = (step, K)
        ctx.mark_non_differentiable(valid)
        return ce, valid

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_ce, _grad_valid):
        return (_ray_bwd(ctx, grad_ce, lib().vidar_ray_ce_bwd_f32, "ray_ce_bwd", 6),) + (None,) * 5


class _RayGumbel(Function):
    @staticmethod
    def forward(ctx, sigma, origin, pts, tindex, noise, step, K):
        sigma, origin, pts, tindex, noise = _f(sigma), _f(origin), _f(pts), _f(tindex), _f(noise)
        F_, R, Z, Y, X = _dims(sigma, pts)
        if noise.shape != (R, K):
            raise RuntimeError(f"noise must be [{R},{K}]")
        dist = torch.empty(R, device=sigma.device); aux = torch.empty((R, 3), device=sigma.device)
        with TIMER.span("ray_gumbel_fwd", 4 * (sigma.numel() + R * (K + 8))):
          check(lib().vidar_ray_gumbel_fwd_f32(ptr(sigma), ptr(origin), ptr(pts), ptr(tindex),
                                             ptr(noise), ptr(dist), ptr(aux), F_, R, Z, Y, X, K, step,
                                             stream_of(sigma)), "ray_gumbel_fwd")
        ctx.save_for_backward(sigma, origin, pts, tindex, aux)
        ctx.cfg = (step, K)
        return dist

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_dist):
        return (_ray_bwd(ctx, grad_dist, lib().vidar_ray_gumbel_bwd_f32, "ray_gumbel_bwd", 8),) + (None,) * 6


class _RayDist(Function):
    @staticmethod
    def forward(ctx, sigma, origin, gt, tindex, noise, step, K):
        sigma, origin, gt, tindex, noise = _f(sigma), _f(origin), _f(gt), _f(tindex), _f(noise)
        F_, R, Z, Y, X = _dims(sigma, gt)
        if noise.shape != (R, K + 1):
            raise RuntimeError(f"noise must be [{R},{K + 1}]")
        dist = torch.empty(R, device=sigma.device); gt_len = torch.empty_like(dist); valid = torch.empty_like(dist)
        aux = torch.empty((R, 3), device=sigma.device)
        with TIMER.span("ray_dist_fwd", 4 * (sigma.numel() + R * (K + 11))):
          check(lib().vidar_ray_dist_fwd_f32(ptr(sigma), ptr(origin), ptr(gt), ptr(tindex), ptr(noise),
                                           ptr(dist), ptr(gt_len), ptr(aux), ptr(valid), F_, R, Z, Y, X, K, step,
                                           stream_of(sigma)), "ray_dist_fwd")
        ctx.save_for_backward(sigma, origin, gt, tindex, aux)
        ctx.cfg = (step, K)
        ctx.mark_non_differentiable(gt_len, valid)
        return dist, gt_len, valid

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_dist, _grad_len, _grad_valid):
        return (_ray_bwd(ctx, grad_dist, lib().vidar_ray_dist_bwd_f32, "ray_dist_bwd", 8),) + (None,) * 6


def ray_ce(sigma, origin, gt, tindex, step=1.0, K=K_SAMPLES):
    """sigma [F,Z,Y,X], origin [F,3], gt [R,3], tindex [R] -> (ce [R], valid [R])"""
    return _RayCE.apply(sigma, origin, gt, tindex, float(step), int(K))


def gumbel_noise(R, K=K_SAMPLES, device="cuda", generator=None):
    """F.gumbel_softmax's noise: -log(Exponential(1)) (torch/nn/functional.py gumbel_softmax)."""
    e = torch.empty((R, K), device=device, dtype=torch.float32).exponential_(generator=generator)
    return -e.log()


def ray_gumbel(sigma, origin, pts, tindex, noise=None, step=1.0, K=K_SAMPLES):
    """-> differentiable rendered distance [R] of _custom_gumbel_softmax_distance."""
    if noise is None:
        noise = gumbel_noise(pts.shape[0], K, sigma.device)
    return _RayGumbel.apply(sigma, origin, pts, tindex, noise, float(step), int(K))


def ray_dist(sigma, origin, gt, tindex, noise=None, step=1.0, K=K_SAMPLES):
    """_custom_gumbel_softmax_distance on the GT rays (use_dist_loss): noise [R, K+1], entry 0 the end point.
    -> (dist [R] differentiable, gt_len [R] = |gt - origin|, valid [R]); dropped rays give 0, 0, 0."""
    if noise is None:
        noise = gumbel_noise(gt.shape[0], int(K) + 1, sigma.device)
    return _RayDist.apply(sigma, origin, gt, tindex, noise, float(step), int(K))


def _listed(sigma, origin, pts, tindex, *outs):
    """the prologue of the no-grad ops on listed rays -> ((sigma, origin, pts, tindex) as contiguous fp32,
    (F, R, Z, Y, X), one empty output per entry of `outs`: [R, *entry], or like sigma for None)"""
    rays = _f(sigma.detach()), _f(origin), _f(pts), _f(tindex)
    dims = _dims(rays[0], rays[2])
    return rays, dims, tuple(torch.empty_like(rays[0]) if o is None else torch.empty((dims[1], *o), device=rays[0].device)
                             for o in outs)


def ray_argmax(sigma, origin, pts, tindex, step=1.0, K=K_SAMPLES):
    """test-time decode -> (pred_dist [R], gt_dist [R]) in voxel units, no grad."""
    rays, dims, out = _listed(sigma, origin, pts, tindex, (), ())
    check(lib().vidar_ray_argmax_f32(*map(ptr, rays), *map(ptr, out), *dims, int(K), step, stream_of(rays[0])),
          "ray_argmax")
    return out


def _cam_args(pix2vox, hw, u0, v0, du, dv):
    if pix2vox.dim() != 4 or pix2vox.shape[-2:] != (4, 4):
        raise ValueError("pix2vox must be [F, C, 4, 4]")
    F_, C = pix2vox.shape[:2]
    return F_, C, int(hw[0]), int(hw[1]), float(u0), float(v0), float(du), float(dv)


def _cam(sigma, pix2vox, hw, u0, v0, du, dv):
    """the prologue of the camera-view ops -> (sigma, pix2vox as contiguous fp32, _cam_args' geometry, (Z, Y, X))"""
    sigma, pix2vox = _f(sigma.detach()), _f(pix2vox)
    geom = _cam_args(pix2vox, hw, u0, v0, du, dv)
    F_, Z, Y, X = sigma.shape
    if geom[0] != F_:
        raise ValueError(f"pix2vox holds {geom[0]} frames, sigma {F_}")
    if pix2vox.device != sigma.device:
        raise RuntimeError(f"pix2vox is on {pix2vox.device}, sigma on {sigma.device}")
    return sigma, pix2vox, geom, (Z, Y, X)


def ray_argmax_cam(sigma, pix2vox, hw, u0=0.5, v0=0.5, du=1.0, dv=1.0, step=1.0, K=K_SAMPLES):
    """camera-view decode: sigma [F,Z,Y,X], pix2vox [F,C,4,4] (homogeneous pixel -> voxel, affine), one ray per pixel
    (x, y) of the hw = (Hs, Ws) grid at u = u0 + x*du, v = v0 + y*dv -> dist [F,C,Hs,Ws] in voxel units, 0 where the
    ray meets nothing.  The rays are never stored (vidar_ray_argmax_cam_f32); no grad."""
    sigma, pix2vox, geom, zyx = _cam(sigma, pix2vox, hw, u0, v0, du, dv)
    dist = torch.empty(geom[:4], device=sigma.device)
    check(lib().vidar_ray_argmax_cam_f32(ptr(sigma), ptr(pix2vox), ptr(dist), *geom, *zyx, int(K), step,
                                         stream_of(sigma)), "ray_argmax_cam")
    return dist


def ray_stats(sigma, origin, pts, tindex, step=1.0, K=K_SAMPLES):
    """ray_argmax with its confidence -> (pred_dist [R], gt_dist [R], stats [R, 4]) in voxel units, no grad.  The two
    distances are ray_argmax's bits; stats = (p_max, mean, rms, entropy) of the softmax over the ray's live waypoints
    (include/vidar_hip.h: vidar_ray_stats_f32), four zeros for a skipped ray or one without a live waypoint."""
    rays, dims, out = _listed(sigma, origin, pts, tindex, (), (), (4,))
    check(lib().vidar_ray_stats_f32(*map(ptr, rays), *map(ptr, out), *dims, int(K), step, stream_of(rays[0])),
          "ray_stats")
    return out


def ray_stats_cam(sigma, pix2vox, hw, u0=0.5, v0=0.5, du=1.0, dv=1.0, step=1.0, K=K_SAMPLES):
    """ray_argmax_cam with its confidence -> (dist [F,C,Hs,Ws], stats [F,C,Hs,Ws,4]) in voxel units, no grad: dist is
    ray_argmax_cam's bits, stats as in ray_stats (four zeros where the ray meets nothing)."""
    sigma, pix2vox, geom, zyx = _cam(sigma, pix2vox, hw, u0, v0, du, dv)
    dist = torch.empty(geom[:4], device=sigma.device)
    stats = torch.empty((*geom[:4], 4), device=sigma.device)
    check(lib().vidar_ray_stats_cam_f32(ptr(sigma), ptr(pix2vox), ptr(dist), ptr(stats), *geom, *zyx, int(K), step,
                                        stream_of(sigma)), "ray_stats_cam")
    return dist, stats


def occupancy_workspace_bytes(F_, Z, Y, X):
    """bytes of caller-owned scratch for ray_occupancy / ray_occupancy_cam under the library's current mode"""
    nbytes = ctypes.c_int64(0)
    check(lib().vidar_ray_occupancy_workspace_bytes(F_, Z, Y, X, ctypes.addressof(nbytes)), "ray_occupancy")
    return nbytes.value


def ray_occupancy(sigma, origin, pts, tindex, step=1.0, K=K_SAMPLES):
    """occupancy evidence of the rays ray_argmax marches -> (hit, free), both [F,Z,Y,X] fp32, no grad: the softmax of
    every ray's live waypoints splatted through the trilinear weights its logits were read with -- hit takes p_k (the
    return lies at k), free takes b_k = the mass beyond k (the ray passed k); include/vidar_hip.h:
    vidar_ray_occupancy_f32.  Under the deterministic mode both volumes are accumulated in fixed point."""
    rays, (F_, R, Z, Y, X), out = _listed(sigma, origin, pts, tindex, None, None)
    deterministic.sync()
    ws, wsp, wsn = workspace(occupancy_workspace_bytes, F_, Z, Y, X, like=rays[0])
    check(lib().vidar_ray_occupancy_f32(*map(ptr, rays), *map(ptr, out), F_, R, Z, Y, X, int(K), step, wsp, wsn,
                                        stream_of(rays[0])), "ray_occupancy")
    return out


def ray_occupancy_cam(sigma, pix2vox, hw, u0=0.5, v0=0.5, du=1.0, dv=1.0, step=1.0, K=K_SAMPLES):
    """ray_occupancy on the rays ray_argmax_cam marches (one per pixel of the hw grid, never stored) -> (hit, free)
    [F,Z,Y,X], no grad."""
    sigma, pix2vox, geom, zyx = _cam(sigma, pix2vox, hw, u0, v0, du, dv)
    hit = torch.empty_like(sigma); free = torch.empty_like(sigma)
    deterministic.sync()
    ws, wsp, wsn = workspace(occupancy_workspace_bytes, geom[0], *zyx, like=sigma)
    check(lib().vidar_ray_occupancy_cam_f32(ptr(sigma), ptr(pix2vox), ptr(hit), ptr(free), *geom, *zyx, int(K), step,
                                            wsp, wsn, stream_of(sigma)), "ray_occupancy_cam")
    return hit, free


def sweep_evidence(origin, pts, tindex, shape, step=1.0, K=K_SAMPLES):
    """measured evidence of a sweep -> (hit, free), both [F,Z,Y,X] = `shape` fp32, no grad: the rays of ray_occupancy
    (origin [F,3], pts [R,3], tindex [R], voxel units) with pts the MEASURED returns; no volume is read.  free takes
    a_k = clamp((L - (k + 0.5) step) / step, 0, 1) at every waypoint before the return (L = |p - o|), hit the trilinear
    weights of the end point itself; include/vidar_hip.h: vidar_sweep_evidence_f32.  The grids compare cell for cell with
    ray_occupancy's.  Under the deterministic mode both volumes are accumulated in fixed point."""
    origin, pts, tindex = _f(origin), _f(pts), _f(tindex)
    F_, Z, Y, X = (int(n) for n in shape)
    if not (origin.is_cuda and pts.device == origin.device and tindex.device == origin.device):
        raise RuntimeError("sweep_evidence needs its rays on one GPU: there is no CPU path")
    if tuple(origin.shape) != (F_, 3) or pts.dim() != 2 or pts.shape[1] != 3 or tuple(tindex.shape) != (pts.shape[0],):
        raise ValueError(f"sweep_evidence: origin [{F_},3], pts [R,3], tindex [R]")
    if min(F_, Z, Y, X) <= 0:
        raise ValueError("sweep_evidence: shape must be four positive sizes (F, Z, Y, X)")
    hit = torch.empty((F_, Z, Y, X), device=origin.device); free = torch.empty_like(hit)
    deterministic.sync()
    ws, wsp, wsn = workspace(occupancy_workspace_bytes, F_, Z, Y, X, like=origin)
    check(lib().vidar_sweep_evidence_f32(ptr(origin), ptr(pts), ptr(tindex), ptr(hit), ptr(free), F_, pts.shape[0],
                                         Z, Y, X, int(K), step, wsp, wsn, stream_of(origin)), "sweep_evidence")
    return hit, free


def point_occupancy(sigma, origin, pts, tindex, step=1.0, K=K_SAMPLES, extent=1.0):
    """occupancy at listed points -> [R, 2] fp32 (hit, free), no grad: the decode's softmax along the ray from the origin
    through pts[r], asked two questions about the stretch [L - extent/2, L + extent/2] of that ray (L = |pts[r] - origin|,
    extent in voxel units): hit = the probability that the return lies in it, free = that it lies beyond it -- the ray
    reached the point and went on.  hit + free <= 1 is the mass the ray still has when it gets there; two zeros for a
    skipped ray, one without a live waypoint, and pts[r] == origin.  include/vidar_hip.h: vidar_point_occupancy_f32.
    No atomics: equal inputs give equal bits in every mode."""
    rays, dims, (out,) = _listed(sigma, origin, pts, tindex, (2,))
    check(lib().vidar_point_occupancy_f32(*map(ptr, rays), ptr(out), *dims, int(K), step, float(extent),
                                          stream_of(rays[0])), "point_occupancy")
    return out


def voxel_occupancy(sigma, origin, step=1.0, K=K_SAMPLES, extent=1.0):
    """point_occupancy at every voxel's centre, one ray per voxel from its frame's origin [F,3] -> (hit, free), both
    [F,Z,Y,X] fp32, no grad, the listed form's bits; the rays are never stored (vidar_voxel_occupancy_f32).  The grids
    read like ray_occupancy's -- forecast.occupancy_grid(hit, free, min_evidence) -- with the evidence hit + free a
    probability in [0, 1] instead of a count of waypoints, and they depend on no ray set."""
    sigma, origin = _f(sigma.detach()), _f(origin)
    F_, Z, Y, X = sigma.shape
    if tuple(origin.shape) != (F_, 3) or origin.device != sigma.device:
        raise ValueError(f"voxel_occupancy: origin must be [{F_},3] on sigma's device")
    hit = torch.empty_like(sigma); free = torch.empty_like(sigma)
    check(lib().vidar_voxel_occupancy_f32(ptr(sigma), ptr(origin), ptr(hit), ptr(free), F_, Z, Y, X, int(K), step,
                                          float(extent), stream_of(sigma)), "voxel_occupancy")
    return hit, free


def cam_rays(pix2vox, hw, u0=0.5, v0=0.5, du=1.0, dv=1.0):
    """the rays ray_argmax_cam marches, written out: -> (origin [F,C,3], pts [F,C,Hs,Ws,3]) in voxel units."""
    pix2vox = _f(pix2vox)
    geom = _cam_args(pix2vox, hw, u0, v0, du, dv)
    origin = torch.empty((*geom[:2], 3), device=pix2vox.device)
    pts = torch.empty((*geom[:4], 3), device=pix2vox.device)
    check(lib().vidar_cam_rays_f32(ptr(pix2vox), ptr(origin), ptr(pts), *geom, stream_of(pix2vox)), "cam_rays")
    return origin, pts
