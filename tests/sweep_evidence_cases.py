"""Shared inputs and the torch-CPU restatement of tests/test_sweep_evidence_gpu.py and tests/test_occ_score_{cpu,gpu}.py:
the measured evidence of a sweep (vidar_sweep_evidence_f32, include/vidar_hip.h).  torch + numpy only, no GPU, no kernel
of the product.

With L = |p - o| and a_k = clamp((L - (k + 0.5) step) / step, 0, 1), for every ray that is not skipped and has a finite
L > 0:
    free = ray_occupancy_cases.splat with the weights a_k           (the adjoint of the zero-padded sample at the waypoints)
    hit  = the autograd adjoint of F.grid_sample at the END POINTS  (d/d vol of the sum of the samples)
in the dtype that is asked for: fp32 is the yardstick, fp64 the reference.  Nothing here shares code with the kernel.

Inputs: the rays of ray_stats_cases.rays() (130 rays in a 2 x 4 x 10 x 96 volume, two skipped, two reversed, lengths
0.5 - 30.5) and its six marches.  At (65, 0.25) the return of 58 rays (56 of them marched) lies beyond K * step = 16.25:
their hit is splatted all the same, and all their waypoints have a_k = 1.

The yardstick of the GPU test is this restatement in fp32 against itself in fp64, max abs over the voxels.  Measured on
the CPU over the six marches: hit 1.5e-6 .. 1.7e-6 (values up to 3.1), free 3.0e-5 .. 2.1e-4 (values up to 336).
"""
import math

import torch
import torch.nn.functional as F

from oracle import head as H
import ray_occupancy_cases as RO
import ray_stats_cases as RS

MARCHES = RS.MARCHES
MARCH_IDS = [f"K{K}-step{step}" for K, step in MARCHES]
SHAPE = (RS.F_, RS.Z, RS.Y, RS.X)


def beam_weights(shape, origin, pts, tindex, K, step, dt):
    """-> (a [R, K] in dt, marched [R] bool): a_k of every ray, zeros for a ray that adds nothing (skipped, L == 0, L not
    finite)"""
    Fn = shape[0]
    origin, pts = origin.to(dt), pts.to(dt)
    inside = (tindex >= 0) & (tindex < Fn)
    f = torch.where(inside, tindex, torch.zeros_like(tindex)).long()
    r = pts - origin[f]
    L = torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2])
    marched = inside & torch.isfinite(L) & (L > 0)
    d = (torch.arange(K, dtype=dt) + 0.5) * step
    a = ((L.view(-1, 1) - d.view(1, -1)) / step).clamp(0, 1)
    return torch.where(marched.view(-1, 1), a, torch.zeros_like(a)), marched


def end_point_splat(shape, pts, tindex, marched, dt):
    """sum over the marched rays of the trilinear weights of their end point, corners outside the volume dropped
    -> [F, Z, Y, X] in dt"""
    Fn, Z, Y, X = shape
    out = torch.zeros(shape, dtype=dt)
    for f in range(Fn):
        sel = ((tindex == f) & marched).nonzero().squeeze(-1)
        if sel.numel() == 0:
            continue
        gn = H._normalise(pts[sel].to(dt).view(-1, 1, 3), Z, Y, X)
        vol = torch.zeros(1, 1, Z, Y, X, dtype=dt, requires_grad=True)
        F.grid_sample(vol, gn.view(1, 1, *gn.shape), align_corners=False).sum().backward()
        out[f] = vol.grad[0, 0]
    return out


def evidence(shape, origin, pts, tindex, K, step, dt):
    """-> (hit, free) [F, Z, Y, X] in dt"""
    a, marched = beam_weights(shape, origin, pts, tindex, K, step, dt)
    # a ray that adds nothing may hold anything (NaN): it is handed to the splat as a skipped ray, never as 0 * NaN
    keep = torch.where(marched, tindex, torch.full_like(tindex, -1.0))
    free = RO.splat(shape, origin, pts, keep, K, step, a)
    return end_point_splat(shape, pts, tindex, marched, dt), free


class Case:
    """one march of ray_stats_cases' rays: the two grids in fp32 and fp64, once"""
    def __init__(self, K, step):
        self.K, self.step = K, step
        self.origin, self.pts, self.tindex = RS.rays()
        rays = (SHAPE, self.origin, self.pts, self.tindex, K, step)
        self.want32 = evidence(*rays, torch.float32)
        self.want64 = evidence(*rays, torch.float64)
        L = (self.pts.double() - self.origin.double()[self.tindex.clamp(0, RS.F_ - 1).long()]).norm(dim=1)
        self.beyond = int(((L > K * step) & beam_weights(*rays, torch.float64)[1]).sum())

    def yardstick(self):
        """max |fp32 - fp64| over the voxels, (hit, free)"""
        return tuple(float((a.double() - b).abs().max()) for a, b in zip(self.want32, self.want64))


_CASES = {}


def case(K, step):
    key = (K, step)
    if key not in _CASES:
        _CASES[key] = Case(*key)
    return _CASES[key]
