"""Shared geometry of tests/test_forecast_view_{cpu,gpu}.py: pin-hole cameras stated directly in voxel coordinates of a
4 x 12 x 14 volume, two frames of two cameras each, and the two pixel grids.  torch + numpy only, no GPU."""
import numpy as np
import torch

Z, Y, X = 4, 12, 14
F_, C = 2, 2
# (Hs, Ws, u0, v0, du, dv): a 12 x 20 image at stride 1, and every 4th pixel of a 52 x 84 one (13 x 21: ragged edges for
# the wave-per-ray kernel's 4 rays per block and for the thread-per-pixel kernel's blocks of 256)
GRIDS = [(12, 20, 0.5, 0.5, 1.0, 1.0), (13, 21, -30.0, -18.0, 4.0, 4.0)]


def camera(centre, forward, up=(0.0, 0.0, 1.0), focal=10.0, principal=(10.0, 6.0)):
    """pix2vox [4, 4] fp64 of a pin-hole camera at `centre` (voxel coordinates) looking along `forward`: the pixel
    (u d, v d, d, 1) lands at centre + d * (right * (u - cx) / f + down * (v - cy) / f + forward)"""
    fwd = np.asarray(forward, np.float64); fwd = fwd / np.linalg.norm(fwd)
    right = np.cross(fwd, np.asarray(up, np.float64)); right = right / np.linalg.norm(right)
    down = np.cross(fwd, right)
    k_inv = np.array([[1 / focal, 0, -principal[0] / focal], [0, 1 / focal, -principal[1] / focal], [0, 0, 1.0]])
    m = np.eye(4)
    m[:3, :3] = np.stack([right, down, fwd], 1) @ k_inv
    m[:3, 3] = centre
    return m


def camera_set():
    """[F, C, 4, 4] fp32: (0,0) outside the volume, looking into it; (0,1) INSIDE the volume; (1,0) outside and looking
    away, so that every ray misses; (1,1) above a corner, looking down at the centre"""
    cams = [[camera((-6.0, 6.3, 2.2), (1.0, 0.05, -0.02)), camera((7.3, 5.6, 1.9), (0.3, 1.0, 0.05))],
            [camera((-6.0, 6.3, 2.2), (-1.0, 0.1, 0.0)), camera((-3.0, -4.0, 9.0), (10.0, 10.0, -7.0))]]
    return torch.from_numpy(np.array(cams)).float()


def volume(seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(F_, Z, Y, X, generator=g)
