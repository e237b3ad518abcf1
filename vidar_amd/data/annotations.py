"""Box annotations of one frame of a nuScenes info pkl, on the host (numpy; a few hundred boxes per frame).

The info layout is the one the reference's converter writes (tools/data_converter/nuscenes_converter.py:305-332):
`gt_boxes [N, 7]` (centre, w l h, yaw = -rot - pi/2, origin at the gravity centre), `gt_names`, `gt_velocity [N, 2]`,
`num_lidar_pts`, `num_radar_pts`, `valid_flag`.

What the fine-tune recipes do with them is three steps of their training pipeline, in this order
(vidar_finetune/nusc_1_4_subset/vidar_1_8_nusc_1future.py:182-184):
  ann_info              LoadAnnotations3D on NuScenesDataset.get_ann_info           [3P mmdet3d]
  object_range_filter   ObjectRangeFilter(point_cloud_range)                        [3P mmdet3d]
  object_name_filter    ObjectNameFilter(classes)                                   [3P mmdet3d]
[3P] mmdet3d 0.17.1 is third party and not part of the reference tree: these are restated from memory and unpinned."""
from __future__ import annotations

import numpy as np
import torch


def ann_info(info, class_names, use_valid_flag, with_velocity=True):
    """-> (boxes [G, 9] float32 with z on the BOTTOM face, labels [G] int64, num_pts [G] int64: lidar + radar points).
    The mask is `valid_flag` when `use_valid_flag` is set, else `num_lidar_pts > 0`; a name outside `class_names` gives
    label -1; NaN velocities become 0; the boxes go through LiDARInstance3DBoxes(..., origin=(0.5, 0.5, 0.5)), which
    moves z from the gravity centre to the bottom face in fp32."""
    from ..plugin.core_bbox import LiDARInstance3DBoxes
    mask = np.asarray(info["valid_flag"], bool) if use_valid_flag else np.asarray(info["num_lidar_pts"]) > 0
    boxes = np.asarray(info["gt_boxes"], np.float64).reshape(-1, 7)[mask]
    names = np.asarray(info["gt_names"])[mask]
    class_names = list(class_names)
    labels = np.array([class_names.index(n) if n in class_names else -1 for n in names], dtype=np.int64)
    if with_velocity:
        vel = np.array(np.asarray(info["gt_velocity"], np.float64).reshape(-1, 2)[mask])
        vel[np.isnan(vel[:, 0])] = [0.0, 0.0]
        boxes = np.concatenate([boxes, vel], axis=-1)
    num_pts = np.asarray(info["num_lidar_pts"], np.int64)[mask]
    if "num_radar_pts" in info:
        num_pts = num_pts + np.asarray(info["num_radar_pts"], np.int64)[mask]
    boxes = LiDARInstance3DBoxes(boxes, box_dim=boxes.shape[-1], origin=(0.5, 0.5, 0.5)).tensor.numpy()
    return boxes, labels, num_pts


def limit_yaw(boxes, offset=0.5, period=2 * np.pi):
    """mmdet3d's limit_period on the yaw column, in fp32 like the tensor it works on: offset 0.5 -> [-pi, pi)"""
    t = torch.from_numpy(np.array(boxes, np.float32))
    t[:, 6] = t[:, 6] - torch.floor(t[:, 6] / period + offset) * period
    return t.numpy()


def object_range_filter(boxes, labels, pc_range):
    """Keep the boxes whose centre lies STRICTLY inside the BEV bounds pc_range[[0, 1, 3, 4]] (compared in fp32, the
    dtype of both sides in mmdet3d), then wrap the yaw of the kept ones into [-pi, pi).  -> (boxes, labels)"""
    r = np.asarray(pc_range, np.float32)[[0, 1, 3, 4]]
    b = np.asarray(boxes, np.float32)
    keep = (b[:, 0] > r[0]) & (b[:, 1] > r[1]) & (b[:, 0] < r[2]) & (b[:, 1] < r[3])
    return limit_yaw(b[keep]), np.asarray(labels)[keep]


def object_name_filter(boxes, labels, num_classes=None):
    """Drop the boxes whose label is not a class index (-1: a name outside the recipe's classes).  -> (boxes, labels)"""
    labels = np.asarray(labels)
    keep = labels >= 0 if num_classes is None else (labels >= 0) & (labels < num_classes)
    return np.asarray(boxes)[keep], labels[keep]


def frame_annotations(info, class_names, pc_range, use_valid_flag=True):
    """the three steps in the recipes' order -> (boxes [G, 9] float32, labels [G] int64)"""
    boxes, labels, _ = ann_info(info, class_names, use_valid_flag)
    boxes, labels = object_range_filter(boxes, labels, pc_range)
    return object_name_filter(boxes, labels, len(class_names))
