"""The detection fine-tune data set: `CustomNuScenesDataset` of projects/mmdet3d_plugin/datasets/nuscenes_dataset.py
with the pipelines of the fine-tune recipes (vidar_finetune/nusc_1_4_subset/vidar_1_8_nusc_1future.py:179-207).

Training item (`prepare_train_data`, :78-103, and `union2one`, :106-132): a queue of `queue_length` frames -- one of the
`queue_length` frames before `index` dropped at random, the rest in order, `index` last --, images stacked, `can_bus` of
every frame turned into the motion since the previous one, and the boxes / labels / metas of the LAST frame.  A queue with
a frame that has no box left after the annotation pipeline is dropped and another index drawn (`filter_empty_gt`,
:229-242 on mmdet3d's `_rand_another` [3P]); unlike the reference that loop is bounded.
Test item: one frame, no annotations, the absolute ego pose in `can_bus` (BEVFormer.forward_test takes the deltas)."""
from __future__ import annotations

import copy
import random

import numpy as np
import torch

from ..configs import CLASS_NAMES
from .annotations import frame_annotations
from .assemble import frame_meta_from_info
from .reader import PC_RANGE, TrainAugment, _FrameImages, load_infos


def pretrain_usable_indices(infos, queue_length, valid_future_length=3, stride=4):
    """`use_pretrain_data=True` (:47-69): frames with `queue_length` frames of their scene behind them (the scene's first
    frame does not count) and `valid_future_length` frames of it ahead, every `stride`-th of those"""
    last_scene, last_frame, out = None, 0, []
    for index, info in enumerate(infos):
        if last_scene != info["scene_token"]:
            last_scene, last_frame = info["scene_token"], 0
            continue
        last_frame += 1
        if last_frame >= queue_length:
            tgt = index + valid_future_length
            if tgt >= len(infos):
                break
            if last_scene != infos[tgt]["scene_token"]:
                continue
            out.append(index)
    return out[::stride]


def queue_indices(index, queue_length):
    """the frames of a training item (:86-93): draws one shuffle from Python's `random`"""
    index_list = list(range(index - queue_length, index))
    random.shuffle(index_list)
    index_list = sorted(index_list[1:])
    index_list.append(index)
    return [max(0, i) for i in index_list]


def union2one(queue):
    """list of frame records -> the training item (:106-132)"""
    metas_map = {}
    prev_scene = prev_pos = prev_angle = None
    for i, each in enumerate(queue):
        meta = metas_map[i] = each["img_metas"]
        if meta["scene_token"] != prev_scene:
            meta["prev_bev_exists"] = False
            prev_scene = meta["scene_token"]
            prev_pos, prev_angle = copy.deepcopy(meta["can_bus"][:3]), copy.deepcopy(meta["can_bus"][-1])
            meta["can_bus"][:3] = 0
            meta["can_bus"][-1] = 0
        else:
            meta["prev_bev_exists"] = True
            pos, angle = copy.deepcopy(meta["can_bus"][:3]), copy.deepcopy(meta["can_bus"][-1])
            meta["can_bus"][:3] -= prev_pos
            meta["can_bus"][-1] -= prev_angle
            prev_pos, prev_angle = pos, angle
    last = queue[-1]
    out = dict(img_metas=metas_map, gt_bboxes_3d=last["gt_bboxes_3d"], gt_labels_3d=last["gt_labels_3d"])
    if "img_raw" in last:                    # device-side image pipeline: raw uint8 frames + what the workers drew
        plans = [each["img_plan"] for each in queue]
        out["img_raw"] = torch.stack([each["img_raw"] for each in queue])
        out["img_plan"] = dict(plans[0], photo=None if plans[0]["photo"] is None else np.stack([p["photo"] for p in plans]))
    else:
        out["img"] = torch.stack([each["img"] for each in queue])
    return out


class DetectionSequenceDataset(_FrameImages):
    """training: `dataset[i]` -> dict(img [T, cams, 3, H, W], img_metas {t: meta}, gt_bboxes_3d LiDARInstance3DBoxes,
    gt_labels_3d int64 [G]) -- the forward_train kwargs of one sample of BEVFormer (collate = add the batch dimension);
    test_mode: dict(img [cams, 3, H, W], img_metas meta) of frame i, in dataset order.
    `device_images=True` ships `img_raw` / `img_plan` instead of `img`, as ViDARSequenceDataset does.
    `queue_length` counts the current frame, like the recipes' (4 = three history frames)."""

    MAX_DRAWS = 64                           # items drawn for one __getitem__ before the file is declared unusable

    def __init__(self, ann_file, data_root="", queue_length=4, test_mode=False, load_interval=1, use_valid_flag=False,
                 class_names=CLASS_NAMES, point_cloud_range=PC_RANGE, use_pretrain_data=False, filter_empty_gt=True,
                 augment=None, device_images=False):
        self.ann_file = str(ann_file)
        self.infos, self.metadata = load_infos(ann_file, load_interval)
        self.data_root, self.queue_length, self.test_mode = str(data_root), queue_length, test_mode
        self.use_valid_flag, self.class_names = use_valid_flag, tuple(class_names)
        self.point_cloud_range, self.filter_empty_gt = point_cloud_range, filter_empty_gt
        # True: the recipes' training augmentation (photometric only, config :181); a callable; None: none
        self.augment = TrainAugment(crop_resize_flip=False) if augment is True else augment
        self.img_scale, self.device_images = None, bool(device_images)
        if self.device_images and self.augment is not None and not hasattr(self.augment, "draw"):
            raise TypeError("device_images=True needs an augmentation with a draw(n_imgs, meta, aug_param) method")
        self.usable_index = pretrain_usable_indices(self.infos, queue_length) if use_pretrain_data \
            else list(range(len(self.infos)))
        self.flag = np.zeros(len(self.usable_index), dtype=np.uint8)       # one group: [3P] mmdet3d _set_group_flag

    def __len__(self):
        return len(self.usable_index)

    def frame(self, index, info=None):
        """one frame through the pipeline -> record dict(img | img_raw + img_plan, img_metas[, gt_bboxes_3d, gt_labels_3d]);
        `info`: a private copy of the frame's info to read (and patch `can_bus` of) instead of a fresh one"""
        info = copy.deepcopy(self.infos[index]) if info is None else info
        meta = frame_meta_from_info(info, "nuscenes", self.data_root)
        rec = dict(img_metas=meta)
        self._frame_images(meta, rec)
        rec.pop("aug_param", None)
        if not self.test_mode:
            from ..plugin.core_bbox import LiDARInstance3DBoxes
            boxes, labels = frame_annotations(info, self.class_names, self.point_cloud_range, self.use_valid_flag)
            rec["gt_bboxes_3d"] = LiDARInstance3DBoxes(boxes, box_dim=boxes.shape[-1])
            rec["gt_labels_3d"] = torch.from_numpy(labels)
        return rec

    def prepare_train_data(self, index):
        # The reference patches and differences `can_bus` in the info's own array.  A frame that the clamp at index 0
        # lists twice therefore shares ONE array between its entries of the queue, and union2one's in-place deltas of the
        # second entry read what the first left behind (items 0 .. queue_length - 2 of a file only; the pre-training scan
        # of the 1/4-subset recipes never lists them).  One copy of the info per frame and item keeps that.
        queue, infos = [], {}
        for i in queue_indices(index, self.queue_length):
            if i not in infos:
                infos[i] = copy.deepcopy(self.infos[i])
            rec = self.frame(i, infos[i])
            if self.filter_empty_gt and not bool((rec["gt_labels_3d"] != -1).any()):
                return None
            queue.append(rec)
        return union2one(queue)

    def __getitem__(self, idx):
        if self.test_mode:
            return self.frame(self.usable_index[idx])
        for _ in range(self.MAX_DRAWS):
            data = self.prepare_train_data(self.usable_index[idx])
            if data is not None:
                return data
            idx = int(np.random.choice(len(self.usable_index)))             # [3P] mmdet3d _rand_another (single group)
        raise RuntimeError(f"{self.ann_file}: {self.MAX_DRAWS} items drawn in a row hold a frame without a box of "
                           f"{list(self.class_names)} inside the point-cloud range")
