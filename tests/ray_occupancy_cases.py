"""Shared inputs and the torch-CPU restatement of tests/test_ray_occupancy_{cpu,gpu}.py: the occupancy evidence of the
decode's softmax (vidar_ray_occupancy_f32, include/vidar_hip.h).  torch + numpy only, no GPU, no kernel of the product.

The restatement takes the decode's logits exactly as ray_stats_cases.logits does (oracle.head._waypoints / _normalise,
F.grid_sample(align_corners=False), == 0 -> dead), forms over the live waypoints of a ray
    p_k = exp(z_k - m) / S          b_k = (reversed cumulative sum of p)_k - p_k, 0 at a dead waypoint
and splats them with autograd: hit[f] = d/d vol sum(p * grid_sample(vol)) with p detached, free likewise with b.  That IS
the trilinear splat with the corners outside the volume dropped (the adjoint of the zero-padded sample), and it shares
no code with the kernel.  Everything runs in the dtype of sigma: fp32 is the yardstick, fp64 the reference.

Inputs: the 18 cases of ray_stats_cases unchanged ([2, 4, 10, 96] volumes randn / const / plane, 130 rays of which two are
skipped, K / step of (512, 1.0), (512, 0.2), (37, 1.0), (64, 0.5), (65, 0.25), (1026, 0.125)).  The fp32 and fp64 live
sets of these cases are equal (tests/test_ray_stats_cpu.py asserts it), so every voxel is compared.

The yardstick of the GPU test is this restatement in fp32 against itself in fp64: the largest absolute error over the
voxels, per output and per case.  Measured on the CPU: hit 3.9e-7 .. 6.1e-6 (values up to 3.4), free 2.0e-5 .. 3.5e-4
(values up to 338); 482 - 4555 of the 7680 voxels are touched.

On an MI355X the kernels' own error was between 0.17 and 1.87 times the yardstick's, in the default (fp32 atomics into
private copies) and in the deterministic mode alike (hit 0.34 .. 1.75, free 0.17 .. 1.87 over the 18 cases; the camera
form 0.17 .. 0.26); tests/test_ray_occupancy_gpu.py prints both figures and holds the ratio to 4.
"""
import math

import torch
import torch.nn.functional as F

from oracle import head as H
import ray_stats_cases as RS

CASES, CASE_IDS = RS.CASES, RS.CASE_IDS


def weights(z):
    """z [R, K] (-inf = dead) -> (p, b) [R, K] in z's dtype; rows without a live waypoint are zeros"""
    live = z != -math.inf
    has = live.any(1, keepdim=True)
    m = z.max(1, keepdim=True)[0]
    m = torch.where(has, m, torch.zeros_like(m))
    e = torch.where(live, torch.exp(torch.where(live, z - m, torch.zeros_like(z))), torch.zeros_like(z))
    S = e.sum(1, keepdim=True)
    p = e / torch.where(has, S, torch.ones_like(S))
    b = torch.flip(torch.cumsum(torch.flip(p, (1,)), 1), (1,)) - p
    return p, torch.where(live, b, torch.zeros_like(b))


def splat(shape, origin, pts, tindex, K, step, w):
    """sum over rays r and waypoints k of w[r, k] * (trilinear weights of waypoint k, outside corners dropped)
    -> [F, Z, Y, X] in w's dtype; skipped rays (tindex outside 0..F-1) add nothing"""
    dt = w.dtype
    Fn, Z, Y, X = shape
    origin, pts = origin.to(dt), pts.to(dt)
    out = torch.zeros(shape, dtype=dt)
    for f in range(Fn):
        sel = (tindex == f).nonzero().squeeze(-1)
        if sel.numel() == 0:
            continue
        g, _ = H._waypoints(origin[f:f + 1], pts[sel], K, step, with_end=False)
        gn = H._normalise(g, Z, Y, X)
        vol = torch.zeros(1, 1, Z, Y, X, dtype=dt, requires_grad=True)
        s = F.grid_sample(vol, gn.view(1, 1, *gn.shape), align_corners=False).view(gn.shape[0], -1)
        (s * w[sel].detach()).sum().backward()
        out[f] = vol.grad[0, 0]
    return out


def counts(shape, origin, pts, tindex, K, step, live):
    """[F, Z, Y, X] int64: how many (ray, live waypoint, corner inside the volume) triples land on each voxel -- the
    number of terms of the voxel's sum, for the any-order bound of an fp32 sum.  fp64 geometry."""
    Fn, Z, Y, X = shape
    origin, pts = origin.double(), pts.double()
    out = torch.zeros(Fn * Z * Y * X, dtype=torch.int64)
    for f in range(Fn):
        sel = (tindex == f).nonzero().squeeze(-1)
        if sel.numel() == 0:
            continue
        g, _ = H._waypoints(origin[f:f + 1], pts[sel], K, step, with_end=False)
        base = torch.floor(g - 0.5).long()                              # pixel = voxel coordinate - 0.5
        for c in range(8):
            x, y, z = base[..., 0] + (c & 1), base[..., 1] + ((c >> 1) & 1), base[..., 2] + (c >> 2)
            ok = live[sel] & (x >= 0) & (x < X) & (y >= 0) & (y < Y) & (z >= 0) & (z < Z)
            out += torch.bincount((((f * Z + z) * Y + y) * X + x)[ok], minlength=out.numel())
    return out.view(shape)


def occupancy(sigma, origin, pts, tindex, K, step):
    """-> (hit, free) [F, Z, Y, X] in sigma's dtype"""
    z, _, _ = RS.logits(sigma, origin, pts, tindex, K, step)
    p, b = weights(z)
    return (splat(sigma.shape, origin, pts, tindex, K, step, p), splat(sigma.shape, origin, pts, tindex, K, step, b))


class Case:
    """one (volume, K, step): ray_stats_cases' inputs and logits, (p, b) and the two grids in fp32 and fp64, once"""
    def __init__(self, kind, K, step):
        self.rs = c = RS.case(kind, K, step)
        self.kind, self.K, self.step = kind, K, step
        self.sigma, self.origin, self.pts, self.tindex = c.sigma, c.origin, c.pts, c.tindex
        self.p32, self.b32 = weights(c.z32)
        self.p64, self.b64 = weights(c.z64)
        rays = (c.origin, c.pts, c.tindex, K, step)
        self.want32 = tuple(splat(c.sigma.shape, *rays, w) for w in (self.p32, self.b32))
        self.want64 = tuple(splat(c.sigma.shape, *rays, w) for w in (self.p64, self.b64))

    def yardstick(self):
        """max |fp32 - fp64| over the voxels, (hit, free)"""
        return tuple(float((a.double() - b).abs().max()) for a, b in zip(self.want32, self.want64))


_CASES = {}


def case(kind, K, step):
    key = (kind, K, step)
    if key not in _CASES:
        _CASES[key] = Case(*key)
    return _CASES[key]
