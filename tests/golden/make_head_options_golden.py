"""Golden vectors for the head's constructor options -- ray_grid_num, ray_grid_step, use_dist_loss -- from the
REFERENCE's own ViDARHeadBase methods (imported in place with mmcv/mmdet/mmdet3d stubbed, see ref_import.py):
    python tests/golden/make_head_options_golden.py
Inputs are those of head_small.npz (volume 8 x 20 x 24).  F.gumbel_softmax is replaced by the seeded stand-in of
make_head_golden.py; every call draws from a fresh torch.Generator().manual_seed(SEED), and instead of the noise
itself ([49, K+1] + [120, K] floats per option set, 0.7 MB at K = 1026) the fixture keeps the seed, the shape of each
call in call order and the noise's sum, so tests regenerate it with `noise_of` below and check they got the same."""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
HERE = Path(__file__).parent
SEED = 5
# (ray_grid_num, ray_grid_step, use_dist_loss)
OPTIONS = [(512, 1.0, True), (1026, 1.0, True), (1024, 0.5, True), (37, 1.0, True), (64, 1.0, False)]
Fn, Z, Y, X = 2, 8, 20, 24


def tag(K, step, dist):
    return f"k{K}_s{str(step).replace('.', 'p')}_{'dist' if dist else 'nodist'}"


def noise_of(shape, seed=SEED):
    """The stand-in's gumbel noise: -log(Exponential(1)) from a fresh CPU generator (F.gumbel_softmax's formula)."""
    return -torch.empty(tuple(int(s) for s in shape)).exponential_(generator=torch.Generator().manual_seed(int(seed))).log()


def main():
    sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(HERE))
    import ref_import
    head, e2e = ref_import.head_modules()
    G = np.load(HERE / "head_small.npz")
    pc_range = [float(v) for v in G["pc_range"]]
    pts = torch.from_numpy(G["gt_points"])
    origin_pts = torch.from_numpy(G["origin_pts"])
    out = dict(seed=np.array(SEED))
    for K, step, dist in OPTIONS:
        obj = object.__new__(head.ViDARHeadBase)
        obj.__dict__.update(ray_grid_num=K, ray_grid_step=step, use_ce_loss=True, use_dist_loss=dist,
                            use_dense_loss=True, dense_loss_weight=1.0, eval_within_grid=False,
                            loss_weight=G["loss_weight"], _modules={}, _parameters={}, _buffers={})
        bev_preds = torch.from_numpy(G["bev_preds"]).clone().requires_grad_(True)
        calls = []

        def fake_gumbel(logits, tau=1, hard=False, eps=1e-10, dim=-1):
            g = noise_of(logits.shape)
            calls.append(g)
            idx = torch.softmax(logits + g, dim).max(dim, keepdim=True)[1]
            return torch.zeros_like(logits).scatter_(dim, idx, 1.0)
        head.F.gumbel_softmax = fake_gumbel

        loss = head.ViDARHeadBase.loss(obj, dict(next_bev_preds=bev_preds, valid_frames=[0, 1]), [pts], 0, Y, X,
                                       pc_range, Fn, batched_origin_points=origin_pts.clone())
        keys = list(loss.keys())
        total = sum(loss[k] * (2.0 if k == "loss.dense_voxel" else 1.0) for k in keys)
        gsig, = torch.autograd.grad(total, bev_preds)
        (og, op, gg, gp, gti) = head.ViDARHeadBase._process_gt_points(
            obj, bev_preds.detach()[:, -1:], [pts], origin_pts.clone(), [0, 1], 0, Fn, Y, X, pc_range)
        sigma = bev_preds.detach()[:, 0].permute(1, 0, 3, 2).contiguous().view(1, Fn, Z, Y, X)
        mask, feat, w, length = head.ViDARHeadBase._get_grid_features(
            obj, og, gg, gti, [sigma], obj.loss_weight, ray_grid_step=step)
        decode = head.ViDARHeadBase.get_point_cloud_prediction(
            obj, dict(next_bev_preds=bev_preds.detach(), valid_frames=[0, 1]), [pts], 0, Y, X, pc_range,
            batched_origin_points=origin_pts.clone())
        t = tag(K, step, dist)
        out.update({
            f"{t}/loss_keys": np.array(keys), f"{t}/loss_values": np.array([float(loss[k]) for k in keys], np.float64),
            f"{t}/grad_bev_preds": gsig.numpy(),
            f"{t}/noise_shapes": np.array([list(c.shape)[-2:] for c in calls], np.int64),
            f"{t}/noise_sums": np.array([float(c.double().sum()) for c in calls], np.float64),
            f"{t}/feat": feat.numpy(), f"{t}/length": length.numpy(), f"{t}/weight": w.numpy(),
            f"{t}/pred_pcd0": decode["pred_pcds"][0][0].numpy(), f"{t}/pred_pcd1": decode["pred_pcds"][0][1].numpy(),
            f"{t}/gt_pcd0": decode["gt_pcds"][0][0].numpy(), f"{t}/gt_pcd1": decode["gt_pcds"][0][1].numpy()})
        print(t, dict(zip(keys, out[f"{t}/loss_values"])), [tuple(c.shape) for c in calls], feat.shape, length.shape)
    path = HERE / "head_options_small.npz"
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size)


if __name__ == "__main__":
    main()
