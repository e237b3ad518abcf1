"""The tiny heads, logits, clouds and metas shared by tests/test_head_decode_routes_cpu.py and the route tests of
tests/test_forecast_view_gpu.py: F = 2 frames, bs = 2, a 4 x 8 x 8 volume, two clouds of 23 and 31 points (so one is
NaN-padded), some points of a frame outside valid_frames, one NaN coordinate."""
import numpy as np
import torch

import vidar_amd.plugin as P
from test_head_options_cpu import head_cfg

CLASSES = ["ViDARHeadBase", "ViDARHeadV1"]
F_, BS, Z, H, W = 2, 2, 4, 8, 8
VALID_FRAMES = [0, 1]
LENGTHS = (23, 31)


def build_head(cls, ray_grid_num=37):
    torch.manual_seed(0)
    return P.HEADS.build(head_cfg(cls, ray_grid_num=ray_grid_num)).eval()


def geom(head):
    return dict(tgt_bev_h=H, tgt_bev_w=W, tgt_pc_range=head.pc_range)


def pred_dict(head):
    """a bare pred_dict of seeded logits: [F, inter, bs, Q, Z], with the pred_frame_num axis in front of bs for V1"""
    g = torch.Generator().manual_seed(1)
    lead = (F_, 2) + ((head.pred_frame_num,) if hasattr(head, "pred_frame_num") else ())
    return dict(next_bev_preds=torch.randn(*lead, BS, H * W, Z, generator=g), valid_frames=list(VALID_FRAMES))


def clouds(head):
    """list[bs] of [N, 4]: xyz inside the range, the frame label last (the head's own numbering); every fifth point
    belongs to a frame that is not decoded, point 3 of the first cloud has a NaN coordinate"""
    g = torch.Generator().manual_seed(2)
    labels = head._ray_frame_labels(VALID_FRAMES)
    lo, hi = torch.tensor(head.pc_range[:3]), torch.tensor(head.pc_range[3:])
    out = []
    for n in LENGTHS:
        xyz = lo + (hi - lo) * (0.1 + 0.8 * torch.rand(n, 3, generator=g))
        lab = torch.tensor([labels[i % 2] if i % 5 else labels[-1] + 2.0 for i in range(n)])
        out.append(torch.cat([xyz, lab[:, None]], 1))
    out[0][3, 1] = float("nan")
    return out


def rigid(angle, shift):
    m = np.eye(4)
    c, s = np.cos(angle), np.sin(angle)
    m[:2, :2] = [[c, s], [-s, c]]                     # row-vector form
    m[3, :3] = shift
    return m


def metas(n_frames=8):
    """per sample, transforms whose (cur2ref[t], ref2cur[t]) pairs do not multiply to the identity, and two cameras of
    different image sizes"""
    return [dict(total_cur2ref_lidar_transform=[rigid(0.05 * (t + b), (1.0 + t, -2.0 + b, 0.1 * t)) for t in range(n_frames)],
                 total_ref2cur_lidar_transform=[rigid(-0.03 * t, (0.5 * b, 0.25 * t, -0.1)) for t in range(n_frames)],
                 lidar2img=[np.eye(4), np.eye(4)], img_shape=[(12, 20, 3), (13, 21, 3)]) for b in range(BS)]


def origin_points():
    """batched_origin_points [bs, F, 3] for the base head (V1 takes its origins from the metas)"""
    return torch.tensor([[[1.0, -2.0, 0.5], [3.0, 4.0, -0.5]], [[-5.0, 6.0, 0.0], [7.0, -8.0, 1.0]]])


def to(device, x):
    if torch.is_tensor(x):
        return x.to(device)
    if isinstance(x, dict):
        return {k: to(device, v) for k, v in x.items()}
    if isinstance(x, list):
        return [to(device, v) for v in x]
    return x
