"""Shared inputs and the torch-CPU restatement of tests/test_voxel_occupancy_{cpu,gpu}.py: the occupancy query at listed
points and at every voxel's centre (vidar_point_occupancy_f32 / vidar_voxel_occupancy_f32, include/vidar_hip.h).
torch + numpy only, no GPU, no kernel of the product.

The restatement takes the decode's logits exactly as ray_stats_cases.logits does (oracle.head._waypoints / _normalise,
F.grid_sample(align_corners=False), == 0 -> dead) for the ray from the frame's origin through the query q, forms
p_k = exp(z_k - m) / S over the live waypoints and, with L = |q - o|,
    c_near(k) = clamp((L - extent/2 - k step) / step, 0, 1)        c_far(k) = clamp((L + extent/2 - k step) / step, 0, 1)
    hit = sum p_k (c_far(k) - c_near(k))                            free = sum p_k (1 - c_far(k))
in the dtype of sigma: fp32 is the yardstick, fp64 the reference.  A query at the origin itself (a NaN direction: every
waypoint dead), a skipped ray and a ray without a live waypoint give two zeros.

Inputs: the 18 cases of ray_stats_cases unchanged ([2, 4, 10, 96] volumes randn / const / plane, K / step of (512, 1.0),
(512, 0.2), (37, 1.0), (64, 0.5), (65, 0.25), (1026, 0.125)), queried at the end points of its 130 listed rays with
extent 0.3, 1.0 and 2.5, and at the 7 680 voxel centres with extent 1.0.  A query whose fp32 and fp64 live sets differ
is left out of the precision comparison, as in ray_stats_cases.Case.compared: at most 2 of the listed rays and at most
0.1 % of the voxels of a case (tests/test_voxel_occupancy_cpu.py asserts both; measured: no listed ray, 0 or 1 voxel).

The yardstick of the GPU test is this restatement in fp32 against itself in fp64: the largest absolute error over the
compared queries, per output and per case.  Measured on the CPU: the listed rays hit 1.8e-8 .. 2.5e-6, free 7.0e-8 ..
1.8e-6 over the three extents; the voxels hit 1.4e-7 .. 1.1e-5, free 2.6e-7 .. 1.1e-5 (values up to 1).

On an MI355X the kernels' own error was between 0.18 and 1.85 times the yardstick's on the listed rays (hit 0.18 .. 1.58,
free 0.38 .. 1.85 over 18 cases x 3 extents) and between 0.85 and 1.25 times on the voxels (hit 0.96 .. 1.25, free 0.85 ..
1.15); tests/test_voxel_occupancy_gpu.py prints both figures and holds the ratio to 4.
"""
import math

import torch

import ray_stats_cases as RS

CASES, CASE_IDS = RS.CASES, RS.CASE_IDS
EXTENTS = (0.3, 1.0, 2.5)                      # the listed form; the dense form runs at 1.0
MAX_EXCLUDED_RAYS = 2                          # of the 130 listed rays of a case
MAX_EXCLUDED_VOXELS = 0.001                    # of the voxels of a case


def voxel_centres(shape):
    """(F, Z, Y, X) -> pts [F*Z*Y*X, 3] fp32: the centre (x + 0.5, y + 0.5, z + 0.5) of every voxel, x fastest, frame
    slowest -- the order of a flattened [F, Z, Y, X] grid --, and tindex [F*Z*Y*X] fp32: the voxel's frame"""
    Fn, Z, Y, X = shape
    z, y, x = torch.meshgrid(torch.arange(Z), torch.arange(Y), torch.arange(X), indexing="ij")
    c = torch.stack([x, y, z], -1).reshape(-1, 3).float() + 0.5
    return c.repeat(Fn, 1), torch.arange(Fn).repeat_interleave(Z * Y * X).float()


def lengths(origin, pts, tindex, dtype):
    """L [R] = |pts - origin[frame]| in `dtype` (frame clamped for a skipped ray, whose L is not used)"""
    o = origin.to(dtype)[tindex.clamp(0, origin.shape[0] - 1).long()]
    return torch.sqrt(((pts.to(dtype) - o) ** 2).sum(-1))


def query_logits(sigma, origin, pts, tindex, K, step):
    """ray_stats_cases.logits for the rays through `pts` -> (z [R, K], L [R], marched [R]) in sigma's dtype.  A query
    at its origin has no direction: its row is dead (the kernel's NaN coordinates sample as 0)."""
    L = lengths(origin, pts, tindex, sigma.dtype)
    at_origin = L == 0
    moved = torch.where(at_origin.view(-1, 1), pts + 1.0, pts)           # any direction will do: the row is overwritten
    z, _, marched = RS.logits(sigma, origin, moved, tindex, K, step)
    z[at_origin] = -math.inf
    return z, L, marched


def weights(L, K, step, extent, dtype):
    """(w_hit, w_free) [R, K] in `dtype`, every operation in the order of csrc/occ_at_math.h"""
    k = torch.arange(K, dtype=dtype).view(1, -1)
    L = L.to(dtype).view(-1, 1)
    half = extent / 2
    c_near = ((L - half - k * step) / step).clamp(0, 1)
    c_far = ((L + half - k * step) / step).clamp(0, 1)
    return c_far - c_near, 1 - c_far


def query(z, L, step, extent):
    """z [R, K] (-inf = dead), L [R] -> [R, 2] (hit, free) in z's dtype; rows without a live waypoint are zeros"""
    live = z != -math.inf
    has = live.any(1, keepdim=True)
    m = z.max(1, keepdim=True)[0]
    m = torch.where(has, m, torch.zeros_like(m))
    e = torch.where(live, torch.exp(torch.where(live, z - m, torch.zeros_like(z))), torch.zeros_like(z))
    S = e.sum(1, keepdim=True)
    p = e / torch.where(has, S, torch.ones_like(S))
    w_hit, w_free = weights(L, z.shape[1], step, extent, z.dtype)
    out = torch.stack([(p * w_hit).sum(1), (p * w_free).sum(1)], 1)
    return torch.where(has, out, torch.zeros_like(out))


def point_occupancy(sigma, origin, pts, tindex, K, step, extent=1.0):
    """-> [R, 2] (hit, free) in sigma's dtype"""
    z, L, _ = query_logits(sigma, origin, pts, tindex, K, step)
    return query(z, L, step, extent)


class Queries:
    """the restatement of one set of queries in one (volume, K, step), fp32 and fp64, for several extents; the logits are
    dropped once the answers are formed (7 680 x 1 026 of them in the dense form)"""
    def __init__(self, sigma, origin, pts, tindex, K, step, extents):
        self.origin, self.pts, self.tindex, self.K, self.step = origin, pts, tindex, K, step
        z32, L32, self.marched = query_logits(sigma, origin, pts, tindex, K, step)
        z64, L64, _ = query_logits(sigma.double(), origin, pts, tindex, K, step)
        live32, live64 = z32 > -math.inf, z64 > -math.inf
        self.same_live = (live32 == live64).all(1)
        self.has_live = live64.any(1)
        self.L64 = L64
        self.want32 = {e: query(z32, L32, step, e) for e in extents}
        self.want64 = {e: query(z64, L64, step, e) for e in extents}

    def candidates(self):
        return self.has_live & self.marched

    def compared(self):
        return self.same_live & self.has_live & self.marched

    def excluded(self):
        return int((self.candidates() & ~self.compared()).sum())

    def yardstick(self, extent):
        """max |fp32 - fp64| over the compared queries, (hit, free)"""
        d = (self.want32[extent].double() - self.want64[extent])[self.compared()].abs()
        return tuple(d.max(0)[0].tolist())


_LISTED, _DENSE = {}, {}


def listed(kind, K, step):
    """the 130 listed rays of ray_stats_cases at EXTENTS"""
    key = (kind, K, step)
    if key not in _LISTED:
        origin, pts, tindex = RS.rays()
        _LISTED[key] = Queries(RS.volume(kind), origin, pts, tindex, K, step, EXTENTS)
    return _LISTED[key]


def dense(kind, K, step):
    """every voxel centre of the volume at extent 1.0; answers [F*Z*Y*X, 2], view(F, Z, Y, X, 2) is the grid"""
    key = (kind, K, step)
    if key not in _DENSE:
        sigma = RS.volume(kind)
        pts, tindex = voxel_centres(sigma.shape)
        _DENSE[key] = Queries(sigma, RS.rays()[0], pts, tindex, K, step, (1.0,))
    return _DENSE[key]
