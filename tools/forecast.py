"""Forecast without ground truth: what the model expects a LiDAR and the cameras to see in the coming frames.

    python tools/forecast.py vidar_1_8_nusc_3future synthetic --out-dir work_dirs/forecast --samples 2
    python tools/forecast.py vidar_1_8_nusc_3future --checkpoint work_dirs/demo/latest.pth \
        --ann-file data/nuscenes/nuscenes_infos_temporal_val.pkl --device-images --out-dir work_dirs/forecast

Per sample i and frame k (0 = the current frame, 1.. the futures) it writes into --out-dir
    sweep_{i}_{k}.npy        [n, 3] float32: the forecast along `vidar_amd.forecast.lidar_pattern` (--beams, --azimuths),
                             in frame k's own LiDAR coordinates, cropped to the point-cloud range
    bev_{i}_{k}.png          bird's-eye picture of that sweep
    depth_{i}_{k}_cam{c}.png the depth of every --stride-th pixel of camera c (ViDAR.forecast, rigid-rig assumption) over
                             the CURRENT frame of that camera; skipped with --no-depth
with --stats, --min-prob P or --max-rms M (metres; a ray below P or above M is dropped from the sweep and its pixel from
the depth picture) also
    sweep_stats_{i}_{k}.npy  [n, 4] float32, row for row with sweep_{i}_{k}.npy: peak probability, mean depth (m), spread
                             about the decoded depth (m) and entropy (nats) of the softmax along the ray
    conf_{i}_{k}_cam{c}.png  the peak probability of camera c's pixels over the same frame (blue = 0 .. red = 1)
with --occupancy [sweep|cameras|both|dense] (the rays that are marched: the sweep's, the cameras' at --stride, both, or one
ray per voxel through its centre; --min-evidence E is the floor under hit + free, default 0.5 -- waypoints of the marched
rays, or with dense the probability the voxel's own ray still has when it reaches the voxel) also
    occ_{i}_{k}.npy          [Z, H, W] float32: hit / (hit + free) of the forecast volume's voxels, NaN = never seen or
                             occluded (ViDAR.forecast(occupancy=...), vidar_amd.forecast.occupancy_grid)
    occ_bev_{i}_{k}.png      its bird's-eye picture: the most occupied seen voxel of every column, free white, occupied
                             black, unseen columns in one fixed colour
and prints one JSON line per sample with its wall time (device drained).  The frame under the overlay is the network's own
input de-normalised (with --device-images that input comes from the device image pipeline); without a backbone
(--no-backbone: synthetic feature pyramids) the overlay is drawn on black.  No ground truth is read."""
import argparse
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import numpy as np  # noqa: E402
import torch  # noqa: E402


def denormalise(img, mean, std, to_rgb, hw):
    """network input [3, Hp, Wp] fp32 -> the frame [H, W, 3] uint8 in RGB order (padding cropped away)"""
    x = img[:, :hw[0], :hw[1]].float() * torch.tensor(std, device=img.device).view(3, 1, 1) \
        + torch.tensor(mean, device=img.device).view(3, 1, 1)
    x = x.round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0)
    return x if to_rgb else x.flip(-1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("config")
    ap.add_argument("source", nargs="?", choices=["synthetic"], help="`synthetic`: generated samples instead of --ann-file")
    ap.add_argument("--checkpoint")
    ap.add_argument("--ann-file", help="info pkl read by vidar_amd.data in test mode")
    ap.add_argument("--data-root", default="")
    ap.add_argument("--device-images", action="store_true", help="with --ann-file: run the image pipeline in HIP kernels")
    ap.add_argument("--out-dir", required=True)
    ap.add_argument("--samples", type=int, default=1)
    ap.add_argument("--stride", type=int, default=4)
    ap.add_argument("--no-depth", action="store_true")
    ap.add_argument("--no-backbone", action="store_true", help="synthetic feature pyramids instead of images")
    ap.add_argument("--bev", type=int, nargs=2, help="a reduced BEV (plumbing runs)")
    ap.add_argument("--beams", type=int, default=32)
    ap.add_argument("--azimuths", type=int, default=1080)
    ap.add_argument("--near", type=float, default=1.0)
    ap.add_argument("--far", type=float, default=60.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--stats", action="store_true", help="also write the decode's confidence (sweep_stats_*, conf_*)")
    ap.add_argument("--min-prob", type=float, metavar="P", help="drop rays whose peak probability is below P")
    ap.add_argument("--max-rms", type=float, metavar="M", help="drop rays whose spread about the depth exceeds M metres")
    ap.add_argument("--occupancy", nargs="?", const="sweep", choices=["sweep", "cameras", "both", "dense"],
                    help="also write the occupancy grid (occ_*, occ_bev_*) from the sweep's rays, the cameras', both, or "
                         "from one ray per voxel (dense)")
    ap.add_argument("--min-evidence", type=float, default=0.5, metavar="E",
                    help="a voxel with hit + free below E is unseen (NaN): E waypoints of the marched rays, or with "
                         "--occupancy dense the probability the voxel's own ray still has when it gets there")
    args = ap.parse_args(argv)
    if args.occupancy in ("cameras", "both") and args.no_depth:
        raise SystemExit("--occupancy cameras / both marches the cameras' rays: drop --no-depth")
    if (args.source == "synthetic") == bool(args.ann_file):
        raise SystemExit("give either `synthetic` or --ann-file")
    if not torch.cuda.is_available():
        raise SystemExit("tools/forecast.py needs a GPU (the product has no CPU path)")

    from vidar_amd import checkpoint as C
    from vidar_amd import forecast as FC
    from vidar_amd import train as T
    from vidar_amd.configs import get_config
    from vidar_amd.data.reader import IMG_NORM
    from vidar_amd.synthetic import fpn_features, make_sample

    dev = torch.device("cuda", 0)
    kw = dict(bev_h=args.bev[0], bev_w=args.bev[1]) if args.bev else {}
    meta = get_config(args.config, with_backbone=not args.no_backbone, **kw)
    torch.manual_seed(args.seed); np.random.seed(args.seed)
    model = T.build_model(meta["model"]).to(dev).eval()
    if args.checkpoint:
        C.load_checkpoint(model, args.checkpoint, map_location=dev)
    T_img = meta["queue_length"] + 1

    if args.ann_file:
        from vidar_amd.configs import dataset_kwargs
        from vidar_amd.data import ViDARSequenceDataset
        from vidar_amd.data.device_prep import DeviceImagePrep
        from vidar_amd.data.loader import collate, finish_batch
        dkw = dataset_kwargs(meta, test_mode=True)
        dkw["future_length"] = meta["model"]["test_future_frame_num"]
        prep = DeviceImagePrep() if args.device_images else None
        ds = ViDARSequenceDataset(args.ann_file, data_root=args.data_root, device_images=args.device_images, **dkw)
        n_samples = len(ds) if args.samples <= 0 else min(args.samples, len(ds))

        def batch(i):
            s_ = ds[i]
            img = finish_batch(collate([s_]), dev, prep)["img"] if args.device_images else s_["img"][None].to(dev)
            return dict(img=img, img_metas=[s_["img_metas"]])
    else:
        n_samples = args.samples

        def batch(i):
            metas, _ = make_sample(50000 + i, queue_length=meta["queue_length"],
                                   future_frames=meta["model"]["test_future_frame_num"], rays_per_frame=1,
                                   num_cams=meta["num_cams"], img_hw=meta["img_hw"])
            if args.no_backbone:
                return dict(img_metas=[metas], img_feats=fpn_features(i, T_img, num_cams=meta["num_cams"],
                                                                      shapes=meta["fpn_shapes"], device=dev))
            g = torch.Generator().manual_seed(50000 + i)
            return dict(img_metas=[metas], img=torch.randn(1, T_img, meta["num_cams"], 3, *meta["img_hw"], generator=g).to(dev))

    out_dir = Path(args.out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    rays = FC.lidar_pattern(args.beams, args.azimuths).to(dev)
    confidence = {}                                                    # without the flags: the call and the files of before
    if args.stats or args.min_prob is not None or args.max_rms is not None:
        confidence = dict(stats=True, min_prob=args.min_prob, max_rms=args.max_rms)
    occupancy = dict(occupancy=args.occupancy, min_evidence=args.min_evidence) if args.occupancy else {}
    for i in range(n_samples):
        b = batch(i)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = model.forecast(rays=rays, cameras=None if args.no_depth else "all", stride=args.stride, **confidence, **occupancy,
                             **b)
        torch.cuda.synchronize(); t_model = time.perf_counter() - t0
        cur = b["img_metas"][0][T_img - 1] if isinstance(b["img_metas"][0], (list, tuple)) else b["img_metas"][0]
        files = 0
        for k, pts in enumerate(out["sweep"][0]):
            np.save(out_dir / f"sweep_{i}_{k}.npy", pts.cpu().numpy().astype(np.float32))
            FC.save_png(FC.sweep_bev(pts, centre=pts.new_zeros(1, 3)), out_dir / f"bev_{i}_{k}.png")
            files += 2
            if confidence:
                np.save(out_dir / f"sweep_stats_{i}_{k}.npy", out["sweep_stats"][0][k].cpu().numpy().astype(np.float32))
                files += 1
        if occupancy:
            for k, occ in enumerate(out["occupancy"][0]):
                np.save(out_dir / f"occ_{i}_{k}.npy", occ.cpu().numpy().astype(np.float32))
                FC.save_png(FC.occupancy_bev(occ, size_px=720), out_dir / f"occ_bev_{i}_{k}.png")
                files += 2
        if not args.no_depth:
            depth = out["depth"][0]                                    # [F, C, Hs, Ws]
            for c in range(depth.shape[1]):
                hw = tuple(cur["img_shape"][c][:2])
                frame = denormalise(b["img"][0, -1, c], IMG_NORM["mean"], IMG_NORM["std"], IMG_NORM["to_rgb"], hw) \
                    if "img" in b else torch.zeros(*hw, 3, dtype=torch.uint8, device=dev)
                for k in range(depth.shape[0]):
                    FC.save_png(FC.depth_overlay(depth[k, c], frame, args.near, args.far), out_dir / f"depth_{i}_{k}_cam{c}.png")
                    files += 1
                    if confidence:
                        # the peak probability of the pixels that are left: a dropped pixel shows the frame, as in depth_*
                        p_max = out["depth_stats"][0, k, c, ..., 0] * (depth[k, c] > 0)
                        FC.save_png(FC.confidence_overlay(p_max, frame), out_dir / f"conf_{i}_{k}_cam{c}.png")
                        files += 1
        torch.cuda.synchronize()
        print(json.dumps(dict(sample=i, sample_idx=str(cur.get("sample_idx")), frames=len(out["sweep"][0]),
                              sweep_points=[int(p.shape[0]) for p in out["sweep"][0]], files=files,
                              model_s=round(t_model, 3), wall_s=round(time.perf_counter() - t0, 3))), flush=True)


if __name__ == "__main__":
    main()
