"""Shared inputs and the torch-CPU restatement of tests/test_ray_stats_{cpu,gpu}.py: the decode's confidence statistics
(vidar_ray_stats_f32, include/vidar_hip.h).  torch + numpy only, no GPU, no kernel of the product.

The restatement takes the decode's logits exactly as oracle.head.argmax_decode does (oracle.head._waypoints / _normalise,
F.grid_sample(align_corners=False), masked_fill(s == 0, -inf)) and computes, about a depth `d` that is HANDED IN,
    p_max = exp(z_argmax - m) / S,  mean = d + sum e (l - d) / S,  rms = sqrt(sum e (l - d)^2 / S),
    entropy = log S - sum_live e (z - m) / S
in the dtype of its inputs.  `d` is never recomputed here: on a constant volume most waypoints tie for the maximum, and
which of them fp32 and fp64 call the first differs from ray to ray.

Inputs: a [2, 4, 10, 96] volume, 130 rays (no multiple of the 4 rays of a workgroup) mostly along +-x from two origins
inside it, alternating between the two frames, end points 0.5 - 30.5 voxels out; the y slopes take about half the rays out
through a side before the far end.  Rays 7 and 8 are reversed and leave the volume within three voxels; tindex[5] = -1 and
tindex[6] = 2 are skipped (their rows hold no live waypoint: the two "dead" rays of every case -- a marched ray from an
origin inside the volume always has a live first waypoint; marched rays without one are in the camera test).  Ray 11 is
aimed: its waypoint 264 of step 0.2 lies on the centre surface of the plane volume's layer.
Three volumes: randn * 2, constant 0.75, and constant -2 with the layer x = 40 set to 14.

The yardstick of the GPU test is this restatement in fp32 against itself in fp64 about one depth: the largest absolute
error over the 128 marched rays, per statistic and per case.  Measured on the CPU about the fp32 restatement's own arg-max
depth (the GPU test recomputes it about the device's depth and holds the kernel to 4 x it; the figures are for the reader;
mean and rms reach some 60 and 54 voxels):

    volume  (K, step)       p_max     mean      rms       entropy
    randn   (512, 1.0)      2.1e-06   1.0e-04   7.4e-05   7.5e-06
    randn   (512, 0.2)      2.8e-06   2.8e-05   5.6e-05   9.3e-06
    randn   (37, 1.0)       2.8e-06   3.6e-05   2.8e-05   6.0e-06
    randn   (64, 0.5)       8.8e-06   2.2e-05   5.1e-05   2.7e-05
    randn   (65, 0.25)      4.4e-06   2.3e-05   1.9e-05   8.2e-06
    randn   (1026, 0.125)   2.9e-06   1.8e-05   1.9e-05   8.3e-06
    const   (512, 1.0)      1.3e-07   9.4e-06   5.5e-06   4.9e-07
    const   (512, 0.2)      2.6e-09   1.3e-05   6.4e-06   4.4e-07
    const   (37, 1.0)       1.3e-07   3.8e-06   3.3e-06   2.8e-07
    const   (64, 0.5)       2.7e-08   2.9e-06   2.8e-06   3.5e-07
    const   (65, 0.25)      3.9e-08   1.9e-06   1.5e-06   2.9e-07
    const   (1026, 0.125)   6.6e-09   1.1e-05   8.8e-06   6.7e-07
    plane   (512, 1.0)      1.4e-05   5.4e-05   8.5e-05   1.8e-05
    plane   (512, 0.2)      3.6e-05   2.0e-05   1.8e-05   3.2e-05
    plane   (37, 1.0)       6.3e-07   8.5e-06   5.2e-06   7.3e-07
    plane   (64, 0.5)       1.3e-06   7.9e-06   4.8e-06   1.9e-06
    plane   (65, 0.25)      1.2e-06   3.9e-06   2.5e-06   2.4e-06
    plane   (1026, 0.125)   2.4e-05   9.0e-06   2.5e-05   4.8e-05

On an MI355X the kernels' own error was between 0.6 and 2.6 times the yardstick's (tests/test_ray_stats_gpu.py prints both).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import head as H

F_, Z, Y, X = 2, 4, 10, 96
R = 130
ORIGINS = ((2.5, 5.2, 2.1), (93.2, 4.6, 1.7))
MARCHES = [(512, 1.0), (512, 0.2), (37, 1.0), (64, 0.5), (65, 0.25), (1026, 0.125)]
VOLUMES = ["randn", "const", "plane"]
PLANE_X = 40
CASES = [(vol, K, step) for vol in VOLUMES for K, step in MARCHES]
CASE_IDS = [f"{vol}-K{K}-step{step}" for vol, K, step in CASES]
REVERSED, SKIPPED, AIMED = (7, 8), (5, 6), 11


def volume(kind, seed=0):
    if kind == "randn":
        return torch.randn(F_, Z, Y, X, generator=torch.Generator().manual_seed(seed)) * 2
    if kind == "const":
        return torch.full((F_, Z, Y, X), 0.75)
    if kind == "plane":
        v = torch.full((F_, Z, Y, X), -2.0)
        v[..., PLANE_X] = 14.0
        return v
    raise ValueError(kind)


def rays(seed=1):
    """-> origin [F,3], pts [R,3], tindex [R] (fp32)"""
    rng = np.random.default_rng(seed)
    origin = np.array(ORIGINS, np.float64)
    tindex = (np.arange(R) % F_).astype(np.float64)
    f = tindex.astype(int)
    # into the volume: +x from origin 0, -x from origin 1; y slopes that take about half the rays out through a side
    # before the far end, a small z component
    d = np.stack([np.where(f == 0, 1.0, -1.0), rng.uniform(-0.25, 0.25, R), rng.uniform(-0.015, 0.015, R)], 1)
    for r in REVERSED:
        d[r, 0] = -d[r, 0]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    # AIMED: its waypoint 264 of step 0.2 (52.9 voxels out) lies on the centre surface x = 40.5 of the plane volume's layer
    dx = (ORIGINS[1][0] - (PLANE_X + 0.5)) / 52.9
    d[AIMED] = [-dx, 0.085, math.sqrt(1.0 - dx * dx - 0.085 ** 2)]
    length = 0.5 + 30.0 * rng.uniform(0.0, 1.0, R)
    pts = origin[f] + d * length[:, None]
    tindex[SKIPPED[0]] = -1.0
    tindex[SKIPPED[1]] = float(F_)
    return (torch.from_numpy(origin).float(), torch.from_numpy(pts).float(), torch.from_numpy(tindex).float())


def logits(sigma, origin, pts, tindex, K, step):
    """the decode's logits and lengths in sigma's dtype: z [R, K] (-inf = dead), length [R, K], marched [R] bool (the ray
    is not skipped).  Rows of skipped rays are all -inf / 0."""
    dt = sigma.dtype
    origin, pts = origin.to(dt), pts.to(dt)
    n = pts.shape[0]
    z = torch.full((n, K), -math.inf, dtype=dt)
    length = torch.zeros(n, K, dtype=dt)
    marched = torch.zeros(n, dtype=torch.bool)
    for f in range(sigma.shape[0]):
        sel = (tindex == f).nonzero().squeeze(-1)
        if sel.numel() == 0:
            continue
        g, ln = H._waypoints(origin[f:f + 1], pts[sel], K, step, with_end=False)
        gn = H._normalise(g, *sigma.shape[1:])
        s = F.grid_sample(sigma[f].view(1, 1, *sigma.shape[1:]), gn.view(1, 1, *gn.shape),
                          align_corners=False).view(gn.shape[0], -1)
        z[sel] = s.masked_fill(s == 0, -math.inf)
        length[sel] = ln
        marched[sel] = True
    return z, length, marched


def plane_offsets(origin, pts, tindex, K, step):
    """fp64, from the rays alone: (delta [R]: distance in x from the plane layer's centre surface x = PLANE_X + 0.5 to the
    ray's nearest waypoint, crosses [R] bool: that waypoint is within one waypoint spacing of the surface and so far from the
    volume's y / z faces that no sample within a voxel of it touches the padding)"""
    origin, pts = origin.double(), pts.double()
    delta = torch.full((pts.shape[0],), math.inf, dtype=torch.float64)
    crosses = torch.zeros(pts.shape[0], dtype=torch.bool)
    for f in range(origin.shape[0]):
        sel = (tindex == f).nonzero().squeeze(-1)
        g, _ = H._waypoints(origin[f:f + 1], pts[sel], K, step, with_end=False)
        a, k = (g[..., 0] - (PLANE_X + 0.5)).abs().min(1)
        at = torch.gather(g, 1, k.view(-1, 1, 1).expand(-1, 1, 3)).squeeze(1)
        delta[sel] = a
        crosses[sel] = (a <= step) & (at[:, 1] >= 0.8) & (at[:, 1] <= Y - 0.8) & (at[:, 2] >= 0.7) & (at[:, 2] <= Z - 0.7)
    return delta, crosses


def stats_about(z, length, d):
    """(p_max, mean, rms, entropy) [R, 4] about the depth d [R], in z's dtype; rows without a live waypoint are zeros"""
    dt = z.dtype
    live = z != -math.inf
    has = live.any(1)
    m = z.max(1, keepdim=True)[0]                                       # z_argmax: the arg-max's own logit
    m = torch.where(has.view(-1, 1), m, torch.zeros_like(m))
    dz = torch.where(live, z - m, torch.zeros_like(z))                  # dead waypoints never meet 0 * -inf
    e = torch.where(live, torch.exp(dz), torch.zeros_like(z))
    S = e.sum(1)
    S1 = torch.where(has, S, torch.ones_like(S))
    dl = length - d.to(dt).view(-1, 1)
    p_max = torch.exp(m.squeeze(1) - m.squeeze(1)) / S1
    mean = d.to(dt) + (e * dl).sum(1) / S1
    rms = torch.sqrt((e * dl * dl).sum(1) / S1)
    ent = torch.log(S1) - (e * dz).sum(1) / S1
    out = torch.stack([p_max, mean, rms, ent], 1)
    return torch.where(has.view(-1, 1), out, torch.zeros_like(out))


def argmax_depth(z, length):
    """length of the first arg-max waypoint (torch.max), waypoint 0 for an all-dead row"""
    return torch.gather(length, 1, z.max(1)[1].view(-1, 1)).squeeze(1)


class Case:
    """one (volume, K, step): inputs, the fp32 and fp64 logits, and what the tests need of them, computed once"""
    def __init__(self, kind, K, step):
        self.kind, self.K, self.step = kind, K, step
        self.sigma = volume(kind)
        self.origin, self.pts, self.tindex = rays()
        self.z32, self.len32, self.marched = logits(self.sigma, self.origin, self.pts, self.tindex, K, step)
        self.z64, self.len64, _ = logits(self.sigma.double(), self.origin, self.pts, self.tindex, K, step)
        self.live32, self.live64 = self.z32 > -math.inf, self.z64 > -math.inf
        self.same_live = (self.live32 == self.live64).all(1)
        self.has_live = self.live64.any(1)
        self.n_live = self.live64.sum(1)

    def yardstick(self, d):
        """fp32 and fp64 restatement about the depths d [R] -> (stats64 [R,4], |stats32 - stats64| max per statistic
        [4] over the rays that are compared)"""
        s64 = stats_about(self.z64, self.len64, d.double())
        s32 = stats_about(self.z32, self.len32, d.float())
        use = self.compared()
        return s64, (s32.double() - s64)[use].abs().max(0)[0]

    def compared(self):
        return self.same_live & self.has_live & self.marched


_CASES = {}


def case(kind, K, step):
    key = (kind, K, step)
    if key not in _CASES:
        _CASES[key] = Case(*key)
    return _CASES[key]
