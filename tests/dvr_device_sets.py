"""The ray sets that go to the reference's DEVICE kernels (oracle/_ref/ref_*_hip.so), in one place.

The reference kernels check none of their arguments, so a set is sent to them on a GPU only after the CPU suite has
run the very same set through the host build of the same kernel bodies and has seen every emitted voxel index inside
the grid and every per-ray count within MAX_D (tests/test_ref_device_build_cpu.py).  tests/test_reference_device_gpu.py
takes its inputs from here and nowhere else."""
import numpy as np

from dvr_cases import CASES, case
from test_fullsize_parity_gpu import SHAPES
from test_oracle_dvr_edge import FIXED_VOLUMES, edge_case, random_volume

DVR_MAX_D, DVXLR_MAX_D = 1446, 1026                  # dvr.cu:9, dvxlr.cu:10 / dvxlr_v2.cu:10
BASELINE = list(SHAPES)
SMALL = [*CASES, "edge", *(f"vol{i:02d}" for i in range(len(FIXED_VOLUMES)))]
SET_NAMES = [*SMALL, *BASELINE]
LOSSES = ["l1", "l2", "absrel", "bce"]
PHASES = ["train", "test"]


def load(name):
    """-> sigma [N,T,Z,Y,X], origin [N,T',3], points [N,M,3], tindex [N,M], sigma_regul (all float32)."""
    if name in CASES:
        s = case(name)
    elif name == "edge":
        s = edge_case()
    elif name.startswith("vol"):
        return random_volume(*FIXED_VOLUMES[int(name[3:])])
    elif name == "noshare":
        s = noshare_case()
    else:
        from vidar_amd.synthetic import ray_set
        s = ray_set(seed=21, N=1, **SHAPES[name])
    return (*s, np.random.default_rng(7).standard_normal(s[0].shape).astype(np.float32))


def init_grid(sigma, origin):
    return [origin.shape[1], *sigma.shape[2:]]


def scatter_inputs(o):
    """(elementwise_mult, grad_ray_pred) for get_grad_sigma(_v2) from a dvxlr_v2 render result."""
    rng = np.random.default_rng(8)
    em = rng.standard_normal(o[0].shape).astype(np.float32)[..., None] * o[2]
    return em, rng.standard_normal(o[4].shape).astype(np.float32)


def assert_in_grid(sigma, idx, indicator):
    """every emitted voxel index inside the grid, every per-ray count at most MAX_D.  The march moves one voxel
    along one axis per step and never turns, so no ray (of dvr.cu either, whose lists are not emitted) holds more
    than Z + Y + X samples: that sum is bounded too."""
    Z, Y, X = sigma.shape[2:]
    assert Z + Y + X <= DVXLR_MAX_D <= DVR_MAX_D
    if idx.size == 0:
        return
    for axis, size in enumerate((Z, Y, X)):
        a = idx[..., axis]
        assert np.all((a >= 0) & (a < size) & (a == np.floor(a))), f"index axis {axis} leaves the grid"
    count = (indicator >= 0).sum(-1)
    assert int(count.max()) <= min(DVXLR_MAX_D, Z + Y + X)
    live = np.arange(idx.shape[2])[None, None, :] < count[..., None]
    assert not idx[~live].any(), "samples beyond the count"


# ---- rays that share no voxel: the only place where dvr.render's grad_sigma has one value on a device -----------
def dvr_path(origin, point, grid):
    """voxels (z, y, x) that dvr.cu:430-570 visits for one ray, in the same double arithmetic."""
    Z, Y, X = grid
    xo, yo, zo = (float(v) for v in origin)
    xe, ye, ze = (float(v) for v in point)
    v = [int(xo), int(yo), int(zo)]
    r = (xe - xo, ye - yo, ze - zo)
    gt_d = float(np.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]))
    d = [c / gt_d for c in r]
    step = [1 if c >= 0 else -1 for c in d]
    o = (xo, yo, zo)
    tmax = [((v[a] + (0 if step[a] < 0 else 1)) - o[a]) / d[a] if d[a] != 0 else np.finfo(np.float64).max for a in range(3)]
    tdelta = [step[a] / d[a] if d[a] != 0 else np.finfo(np.float64).max for a in range(3)]
    size = (X, Y, Z)
    path, was_inside, last_d = [], False, 0.0
    while True:
        inside = all(0 <= v[a] < size[a] for a in range(3))
        if inside:
            was_inside = True
            path.append((v[2], v[1], v[0]))
        elif was_inside or last_d > gt_d:
            break
        if tmax[0] < tmax[1]:
            a = 0 if tmax[0] < tmax[2] else 2
        else:
            a = 1 if tmax[1] < tmax[2] else 2
        last_d = tmax[a]
        v[a] += step[a]
        tmax[a] += tdelta[a]
    return path


def _dilate(path):
    return {(z + a, y + b, x + c) for z, y, x in path for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)}


def noshare_case(want=48):
    """rays of `two_frames`, thinned greedily (in ray order) until no two of one (batch, frame) come within one
    voxel of each other anywhere along their dvr.cu paths; the other rays become padding (tindex -1)."""
    sigma, origin, points, tindex = case("two_frames")
    tindex = tindex.copy()
    grid = sigma.shape[2:]
    taken, kept = {}, 0
    for n in range(points.shape[0]):
        for c in range(points.shape[1]):
            t = int(tindex[n, c])
            if t < 0:
                continue
            path = dvr_path(origin[n, t], points[n, c], grid) if kept < want else []
            near = _dilate(path)
            if not path or near & taken.setdefault((n, t), set()):
                tindex[n, c] = -1
                continue
            taken[(n, t)] |= near
            kept += 1
    return sigma, origin, points, tindex


def assert_no_shared_voxel(sigma, origin, points, tindex, idx):
    """no voxel of one (batch, frame) volume is on two rays: by the dvr.cu paths and by the dvxlr index lists
    (`idx` [N,M,L,3] of the same rays).  Returns the number of live rays."""
    grid = sigma.shape[2:]
    live = 0
    for n in range(points.shape[0]):
        seen = {}
        for c in range(points.shape[1]):
            t = int(tindex[n, c])
            if t < 0:
                continue
            live += 1
            own = set(dvr_path(origin[n, t], points[n, c], grid))
            own |= {tuple(int(k) for k in row) for row in idx[n, c][(idx[n, c] != 0).any(-1)]}
            assert own, "a kept ray misses the grid"
            bucket = seen.setdefault(t if sigma.shape[1] > 1 else 0, set())
            assert not (own & bucket), f"ray {n},{c} shares a voxel with an earlier ray"
            bucket |= own
    return live
