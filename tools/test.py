"""Thin evaluation launcher (the reference: tools/test.py + tools/dist_test.sh around
`custom_multi_gpu_test`, projects/mmdet3d_plugin/bevformer/apis/test.py:45-114):

    python tools/test.py vidar_1_8_nusc_3future --samples 8 [--checkpoint work_dirs/demo/latest.pth]
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 tools/test.py \
        vidar_1_8_nusc_3future --samples 64 --submission submission/model

Every rank evaluates samples rank, rank+W, ... (synthetic generator, or with --ann-file the validation info pkl
read by vidar_amd.data in test mode: full history required, key-frame cloud only, no augmentation), the
per-sample `frame.k` dicts are gathered over the process group (RCCL) and rank 0 prints the
reference's summary (chamfer distance, L1 and AbsRel ray errors per future frame).  --occupancy-metrics
[--occ-thresholds T ...] [--min-evidence E] also scores the occupancy forecast against the measured sweep of every frame
(vidar_amd.forecast.occupancy_score): rank 0 prints IoU / precision / recall per threshold, coverage, Brier score and
reliability per frame and writes them under "occupancy" in --out.

A detection recipe (finetune/...) runs the BEVFormer detector in video mode instead: the frames of each synthetic sequence go
through forward_test one by one (the previous frame's BEV carried along, reset at a scene change) and the decoded boxes of
every frame are printed -- count, best scores, labels.  The boxes of the current (last) frame of every sequence are then
scored against the sequence's synthetic ground truth (num_pts = 1, no attributes, so attr_err is 1) with
vidar_amd.det_evaluate -- nuScenes mAP, the five true-positive errors and NDS, computed on the device without the
devkit: rank 0 gathers the boxes of all ranks, prints the devkit's closing table and writes the result under "metrics"
in --out, next to the per-frame records ("frames").

With --ann-file a detection recipe runs video mode over the frames of a validation info pkl instead, in dataset order
(vidar_amd.data.DetectionSequenceDataset in test mode; every rank takes a contiguous shard, so its frames stay in scene
order), and scores the boxes of EVERY frame against the file's own annotations (det_evaluate.ground_truth_from_infos: all
annotated boxes with their lidar + radar point counts, no attributes), both sides in the ego frame of their sample;
--results-json PATH also writes the boxes in the nuScenes detection submission layout (global frame), --eval-stride N keeps
every N-th SCENE whole.

    python tools/test.py finetune/vidar_1_8_nusc_1future --checkpoint work_dirs/fine-tune/latest.pth \
        --ann-file data/nuscenes/nuscenes_infos_temporal_val.pkl --samples 0 --results-json work_dirs/results_nusc.json"""
import argparse
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("config")
    ap.add_argument("--checkpoint")
    ap.add_argument("--samples", type=int, default=4, help="size of the synthetic evaluation set")
    ap.add_argument("--no-backbone", action="store_true")
    ap.add_argument("--rays-per-frame", type=int, default=30000)
    ap.add_argument("--bev", type=int, nargs=2, help="evaluate at a reduced BEV (plumbing runs)")
    ap.add_argument("--submission", help="directory for the per-sample depth files (vidar.py:503-519)")
    ap.add_argument("--out", help="write the summary as JSON")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--ann-file", help="validation info pkl (data/nuscenes/nuscenes_infos_temporal_val.pkl)")
    ap.add_argument("--data-root", default="")
    ap.add_argument("--eval-stride", type=int, default=None,
                    help="evaluate every N-th usable val index (quick subset; a detection recipe: every N-th scene, whole, "
                         "so that the temporal input stays what the model expects); default: the whole split, as the "
                         "reference's data.test does")
    ap.add_argument("--results-json", help="detection recipes with --ann-file: also write the decoded boxes in the nuScenes "
                                           "detection submission layout (global frame) to this file")
    ap.add_argument("--cams", type=int, help="cameras per frame of the info file when it is not the recipe's (plumbing "
                                             "runs on reduced files; nuScenes: 6)")
    ap.add_argument("--device-images", action="store_true",
                    help="with --ann-file: ship uint8 frames and run the image pipeline in HIP kernels (same tensor)")
    ap.add_argument("--device-metrics", action="store_true",
                    help="score the forecast on the device: one chamfer call, one ray-error call and one host read per "
                         "batch instead of a dozen round trips per (sample, frame) (same figures; off by default)")
    ap.add_argument("--occupancy-metrics", action="store_true",
                    help="also score the occupancy forecast against the measured future sweep: IoU / precision / recall "
                         "per threshold, coverage, Brier score and reliability per future frame (off by default)")
    ap.add_argument("--occ-thresholds", type=float, nargs="+", metavar="T",
                    help="with --occupancy-metrics: the thresholds on the predicted occupancy (1 to 8; default 0.25 0.5)")
    ap.add_argument("--min-evidence", type=float, metavar="E",
                    help="with --occupancy-metrics: floor on the predicted evidence of a scored voxel (default 0.5)")
    ap.add_argument("--occ-source", choices=["rays", "dense"], default="rays",
                    help="with --occupancy-metrics: the predicted evidence comes from the measured sweep's own ray "
                         "directions (rays) or from one ray per voxel, the grid forecast(occupancy=\"dense\") returns (dense)")
    args = ap.parse_args(argv)
    if args.occupancy_metrics:
        from vidar_amd.plugin.utils import eval_utils
        eval_utils.set_occupancy_metrics(True, source=args.occ_source, thresholds=args.occ_thresholds,
                                         min_evidence=args.min_evidence)
    if args.device_metrics:
        from vidar_amd.plugin.utils import eval_utils
        eval_utils.set_device_metrics(True)

    from vidar_amd import checkpoint as C
    from vidar_amd import evaluate as E
    from vidar_amd import train as T
    from vidar_amd.configs import get_config
    from vidar_amd.synthetic import fpn_features, make_sample

    rank, local, world = T.init_distributed()
    if not torch.cuda.is_available():
        raise SystemExit("tools/test.py needs a GPU (the product has no CPU path)")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    kw = dict(bev_h=args.bev[0], bev_w=args.bev[1]) if args.bev else {}
    meta = get_config(args.config, with_backbone=not args.no_backbone, **kw)
    if args.cams:
        from vidar_amd.configs import set_num_cams
        set_num_cams(meta["model"], args.cams)
    if args.submission:
        meta["model"]["_submission"] = True
        meta["model"]["_submission_path"] = args.submission
    torch.manual_seed(args.seed); np.random.seed(args.seed)
    model = T.build_model(meta["model"]).to(dev)
    if args.checkpoint:
        C.load_checkpoint(model, args.checkpoint, map_location=dev)
    if meta.get("task") == "detection":
        return video_detection(model, meta, args, dev, rank, world)
    n_future = meta["model"]["test_future_frame_num"]

    def batch(i):
        metas, gt = make_sample(50000 + i, queue_length=meta["queue_length"], future_frames=n_future,
                                rays_per_frame=args.rays_per_frame, num_cams=meta["num_cams"],
                                img_hw=meta["img_hw"])
        b = dict(img_metas=[metas], gt_points=[torch.from_numpy(gt).to(dev)])
        T_img = meta["queue_length"] + 1
        if args.no_backbone:
            b["img_feats"] = fpn_features(i, T_img, num_cams=meta["num_cams"], shapes=meta["fpn_shapes"],
                                          device=dev)
        else:
            g = torch.Generator().manual_seed(50000 + i)
            b["img"] = torch.randn(1, T_img, meta["num_cams"], 3, *meta["img_hw"], generator=g).to(dev)
        return b

    n_samples = args.samples
    if args.ann_file:
        from vidar_amd.configs import dataset_kwargs
        from vidar_amd.data import ViDARSequenceDataset
        # the whole val split, like the reference's data.test (no load_frame_interval there); --eval-stride N opts into
        # a 1/N subset for a quick look
        kw = dataset_kwargs(meta, test_mode=True, test_stride=args.eval_stride)
        kw["future_length"] = n_future
        from vidar_amd.data.device_prep import DeviceImagePrep
        from vidar_amd.data.loader import collate, finish_batch
        prep = DeviceImagePrep() if args.device_images else None
        ds = ViDARSequenceDataset(args.ann_file, data_root=args.data_root, device_images=args.device_images, **kw)
        n_samples = len(ds) if args.samples <= 0 else min(args.samples, len(ds))

        def batch(i):                                                  # noqa: F811  (real data replaces the generator)
            s_ = ds[i]
            img = finish_batch(collate([s_]), dev, prep)["img"] if args.device_images else s_["img"][None].to(dev)
            return dict(img=img, img_metas=[s_["img_metas"]], gt_points=[s_["gt_points"].to(dev)])
    results = E.multi_gpu_test(model, batch, n_samples)
    if rank == 0:
        summary = E.summarize(results)
        print(E.format_summary(summary), flush=True)
        occupancy = E.occupancy_summary(summary)
        if occupancy:
            print(E.format_occupancy(occupancy), flush=True)
            summary = dict(summary, occupancy=occupancy)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(json.dumps(summary, indent=1))
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


def video_detection(model, meta, args, dev, rank, world):
    import copy
    from vidar_amd import evaluate as E
    from vidar_amd.det_evaluate import DetectionEval, format_summary
    from vidar_amd.synthetic import fpn_features, make_sample
    if args.submission:
        raise SystemExit("--submission writes the forecasting depth files and does not apply to a detection recipe; its "
                         "boxes go to --results-json (with --ann-file)")
    if args.results_json and not args.ann_file:
        raise SystemExit("--results-json needs --ann-file: the submission layout names the samples of an info file")
    model.eval()
    if args.ann_file:
        return info_detection(model, meta, args, dev, rank, world)
    T_img = meta["queue_length"] + 1
    part = []                                        # per sequence: its frame records, the last frame's boxes, its ground truth
    for i in range(rank, args.samples, world):
        metas, _, gt_boxes, gt_labels = make_sample(50000 + i, queue_length=meta["queue_length"], future_frames=0,
                                                    rays_per_frame=1, num_cams=meta["num_cams"], img_hw=meta["img_hw"],
                                                    with_boxes=True)
        if args.no_backbone:
            feats = fpn_features(i, T_img, num_cams=meta["num_cams"], shapes=meta["fpn_shapes"], device=dev)
        else:
            g = torch.Generator().manual_seed(50000 + i)
            img = torch.randn(1, T_img, meta["num_cams"], 3, *meta["img_hw"], generator=g).to(dev)
        pose = np.zeros(4)
        records = []
        for t in range(T_img):
            m = copy.deepcopy(metas[t])
            pose += [*m["can_bus"][:3], m["can_bus"][-1]]               # forward_test expects absolute ego poses
            m["can_bus"][:3], m["can_bus"][-1] = pose[:3], pose[3]
            kw = dict(img_feats=[[f[:, t] for f in feats]]) if args.no_backbone else dict(img=[img[:, t]])
            box = model(return_loss=False, img_metas=[[m]], **kw)[0]["pts_bbox"]
            records.append(dict(sample=m["sample_idx"], frame=t, boxes=len(box["boxes_3d"]),
                                top_scores=[round(float(v), 4) for v in box["scores_3d"][:3]],
                                top_labels=[int(v) for v in box["labels_3d"][:3]],
                                top_box=[round(float(v), 3) for v in box["boxes_3d"].tensor[0]] if len(box["boxes_3d"]) else None))
            print(json.dumps(records[-1]), flush=True)
        part.append(dict(records=records, boxes=box["boxes_3d"].tensor.numpy(), scores=box["scores_3d"].numpy(),
                         labels=box["labels_3d"].numpy(), gt_boxes=gt_boxes, gt_labels=gt_labels))
    part = E.collect_results(part, args.samples)     # rank 0: every sequence, in dataset order
    if rank == 0:
        def dv(a, dtype):
            return torch.as_tensor(a, dtype=dtype, device=dev)
        pred = [dict(boxes=dv(s["boxes"], torch.float32).reshape(-1, 9), scores=dv(s["scores"], torch.float32),
                     labels=dv(s["labels"], torch.int64)) for s in part]
        gt = [dict(boxes=dv(s["gt_boxes"], torch.float32).reshape(-1, 9), labels=dv(s["gt_labels"], torch.int64),
                   num_pts=torch.ones(len(s["gt_labels"]), dtype=torch.int64, device=dev)) for s in part]
        metrics = DetectionEval(meta.get("class_names") or DetectionEval().class_names).evaluate(pred, gt)
        print(format_summary(metrics), flush=True)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(json.dumps(dict(frames=[r for s in part for r in s["records"]], metrics=metrics),
                                                 indent=1))
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


def whole_scene_subset(infos, stride):
    """indices of the frames of every `stride`-th scene (scenes in order of first appearance)"""
    scenes = list(dict.fromkeys(info["scene_token"] for info in infos))
    keep = set(scenes[::stride or 1])
    return [i for i, info in enumerate(infos) if info["scene_token"] in keep]


@torch.no_grad()
def info_detection(model, meta, args, dev, rank, world):
    """video mode over the frames of an info pkl, scored against its own annotations"""
    from vidar_amd.configs import dataset_kwargs
    from vidar_amd.data import DetectionSequenceDataset, DistributedSampler
    from vidar_amd.data.device_prep import DeviceImagePrep
    from vidar_amd.data.loader import collate, finish_batch
    from vidar_amd.det_evaluate import (DetectionEval, boxes_to_ego, format_summary, ground_truth_from_infos,
                                        write_results_json)
    ds = DetectionSequenceDataset(args.ann_file, data_root=args.data_root, device_images=args.device_images,
                                  **dataset_kwargs(meta, test_mode=True))
    frames = whole_scene_subset([ds.infos[i] for i in ds.usable_index], args.eval_stride)
    if args.samples > 0:                                         # as on the forecasting route: --samples 0 = the whole file
        frames = frames[:args.samples]
    prep = DeviceImagePrep() if args.device_images else None
    part = []
    for pos in DistributedSampler(frames, world, rank):           # contiguous shard: this rank's frames in scene order
        s_ = ds[frames[pos]]
        img = finish_batch(collate([s_]), dev, prep)["img"] if args.device_images else s_["img"][None].to(dev)
        m = s_["img_metas"]
        box = model(return_loss=False, img_metas=[[m]], img=[img])[0]["pts_bbox"]
        rec = dict(sample=m["sample_idx"], scene=m["scene_token"], boxes=len(box["boxes_3d"]),
                   top_scores=[round(float(v), 4) for v in box["scores_3d"][:3]],
                   top_labels=[int(v) for v in box["labels_3d"][:3]])
        print(json.dumps(rec), flush=True)
        part.append(dict(pos=pos, record=rec, boxes=box["boxes_3d"].tensor.numpy(), scores=box["scores_3d"].numpy(),
                         labels=box["labels_3d"].numpy()))
    if torch.distributed.is_available() and torch.distributed.is_initialized() and world > 1:
        parts = [None] * world
        torch.distributed.all_gather_object(parts, part)
        part = [s for p in parts for s in p]                     # rank order = dataset order; the tail repeats the head
    part = part[:len(frames)]
    if rank == 0:
        assert [s["pos"] for s in part] == list(range(len(frames)))
        infos = [ds.infos[ds.usable_index[i]] for i in frames]
        class_names = meta.get("class_names") or DetectionEval().class_names
        lidar = [dict(boxes=torch.as_tensor(s["boxes"], dtype=torch.float32, device=dev).reshape(-1, 9),
                      scores=torch.as_tensor(s["scores"], dtype=torch.float32, device=dev),
                      labels=torch.as_tensor(s["labels"], dtype=torch.int64, device=dev)) for s in part]
        # bottom face -> gravity centre, LiDAR frame -> ego frame of each box's sample: one batched transform
        counts = [len(p["labels"]) for p in lidar]
        b = torch.cat([p["boxes"] for p in lidar])
        b = torch.cat([b[:, :2], (b[:, 2] + b[:, 5] * 0.5)[:, None], b[:, 3:]], 1)
        per_box = lambda key: np.repeat(np.asarray([info[key] for info in infos], np.float64), counts, axis=0)
        ego = boxes_to_ego(b, per_box("lidar2ego_rotation"), per_box("lidar2ego_translation")).split(counts)
        pred = [dict(p, boxes=e) for p, e in zip(lidar, ego)]
        metrics = DetectionEval(class_names).evaluate(pred, ground_truth_from_infos(infos, class_names, dev))
        print(format_summary(metrics, gt_attrs=False), flush=True)
        if args.results_json:
            write_results_json(args.results_json, [info["token"] for info in infos], lidar, infos, class_names)
            print(f"results: {args.results_json}", flush=True)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(json.dumps(dict(frames=[s["record"] for s in part], metrics=metrics), indent=1))
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
