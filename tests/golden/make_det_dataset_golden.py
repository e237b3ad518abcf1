"""Golden for vidar_amd.data.DetectionSequenceDataset from the reference's own data set code: the source text of
CustomNuScenesDataset (projects/mmdet3d_plugin/datasets/nuscenes_dataset.py:19-245: the usable-index scan,
prepare_train_data, union2one, get_data_info) executed in place on the fixture of tests/det_data_cases.py, with a seeded
`random`.
mmdet3d / mmcv / nuscenes-devkit / pyquaternion are not installable.  What the executed text needs from them is restated
here and labelled [3P]: the NuScenesDataset base class (load_annotations, get_ann_info, _set_group_flag), the annotation
steps of the recipes' training pipeline (LoadAnnotations3D, ObjectRangeFilter, ObjectNameFilter, the format bundle),
LiDARInstance3DBoxes, DataContainer, Quaternion and quaternion_yaw.  The image steps are replaced by a tensor that holds the
frame index.  Writes data only (det_dataset.npz).
    python tests/golden/make_det_dataset_golden.py"""
import copy
import pickle
import random
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
REF = Path("/root/reference/projects/mmdet3d_plugin/datasets")

from det_data_cases import CLASS_NAMES, N_FRAMES, PC_RANGE, det_mini_nuscenes  # noqa: E402

SEED = 1000                                  # item `index` is drawn after random.seed(SEED + index)


class Quaternion:                            # [3P] pyquaternion, (w, x, y, z)
    def __init__(self, q):
        self.q = np.asarray(q, np.float64)

    @property
    def rotation_matrix(self):
        w, x, y, z = self.q / np.linalg.norm(self.q)
        return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])

    def __array__(self, dtype=None, copy=None):          # assigned into can_bus[3:7]
        return np.asarray(self.q, dtype)

    def __len__(self):
        return 4

    def __getitem__(self, i):
        return self.q[i]


def quaternion_yaw(q):                       # [3P] nuscenes.eval.common.utils
    v = np.dot(q.rotation_matrix, np.array([1, 0, 0]))
    return np.arctan2(v[1], v[0])


class DC:                                    # [3P] mmcv.parallel.DataContainer, as far as the executed text uses it
    def __init__(self, data, cpu_only=False, stack=False):
        self._data = data

    @property
    def data(self):
        return self._data


class LiDARInstance3DBoxes:                  # [3P] mmdet3d, as far as the pipeline below uses it
    def __init__(self, tensor, box_dim=7, origin=(0.5, 0.5, 0)):
        tensor = torch.as_tensor(tensor, dtype=torch.float32).reshape(-1, box_dim).clone()
        if origin != (0.5, 0.5, 0):
            dst = tensor.new_tensor((0.5, 0.5, 0))
            src = tensor.new_tensor(origin)
            tensor[:, :3] += tensor[:, 3:6] * (dst - src)
        self.tensor, self.box_dim = tensor, box_dim

    def in_range_bev(self, box_range):
        return ((self.tensor[:, 0] > box_range[0]) & (self.tensor[:, 1] > box_range[1])
                & (self.tensor[:, 0] < box_range[2]) & (self.tensor[:, 1] < box_range[3]))

    def limit_yaw(self, offset=0.5, period=np.pi):
        val = self.tensor[:, 6]
        self.tensor[:, 6] = val - torch.floor(val / period + offset) * period

    def __getitem__(self, item):
        return LiDARInstance3DBoxes(self.tensor[item], box_dim=self.box_dim)


class NuScenesDataset:                       # [3P] mmdet3d 0.17.1, as far as the executed text uses it
    def __init__(self, ann_file, classes, use_valid_flag=False, test_mode=False, filter_empty_gt=True, load_interval=1,
                 with_velocity=True, modality=None):
        with open(ann_file, "rb") as f:
            data = pickle.load(f)
        self.data_infos = list(sorted(data["infos"], key=lambda e: e["timestamp"]))[::load_interval]
        self.CLASSES, self.use_valid_flag, self.test_mode = list(classes), use_valid_flag, test_mode
        self.filter_empty_gt, self.with_velocity = filter_empty_gt, with_velocity
        self.modality = modality or dict(use_camera=True)
        self.pcd_range = np.array(PC_RANGE, dtype=np.float32)
        self.seen = []

    def _set_group_flag(self):
        self.flag = np.zeros(len(self), dtype=np.uint8)

    def get_ann_info(self, index):
        info = self.data_infos[index]
        mask = info["valid_flag"] if self.use_valid_flag else info["num_lidar_pts"] > 0
        gt_bboxes_3d = info["gt_boxes"][mask]
        gt_names_3d = info["gt_names"][mask]
        gt_labels_3d = []
        for cat in gt_names_3d:
            gt_labels_3d.append(self.CLASSES.index(cat) if cat in self.CLASSES else -1)
        gt_labels_3d = np.array(gt_labels_3d)
        if self.with_velocity:
            gt_velocity = info["gt_velocity"][mask]
            nan_mask = np.isnan(gt_velocity[:, 0])
            gt_velocity[nan_mask] = [0.0, 0.0]
            gt_bboxes_3d = np.concatenate([gt_bboxes_3d, gt_velocity], axis=-1)
        gt_bboxes_3d = LiDARInstance3DBoxes(gt_bboxes_3d, box_dim=gt_bboxes_3d.shape[-1], origin=(0.5, 0.5, 0.5))
        return dict(gt_bboxes_3d=gt_bboxes_3d, gt_labels_3d=gt_labels_3d, gt_names=gt_names_3d)

    def pre_pipeline(self, results):
        self.seen.append(results["sample_idx"])

    def pipeline(self, results):
        """LoadAnnotations3D, ObjectRangeFilter, ObjectNameFilter, DefaultFormatBundle3D, CustomCollect3D of the recipes
        (vidar_finetune/nusc_1_4_subset/vidar_1_8_nusc_1future.py:179-189); the image steps give the frame's index"""
        boxes, labels = results["ann_info"]["gt_bboxes_3d"], results["ann_info"]["gt_labels_3d"]
        mask = boxes.in_range_bev(self.pcd_range[[0, 1, 3, 4]])
        boxes = boxes[mask]
        labels = labels[mask.numpy().astype(bool)]
        boxes.limit_yaw(offset=0.5, period=2 * np.pi)
        keep = np.array([n in range(len(self.CLASSES)) for n in labels], dtype=bool)
        boxes, labels = boxes[keep], labels[keep]
        index = int(results["sample_idx"][3:])
        meta = {k: v for k, v in results.items() if k != "ann_info"}
        return dict(img=DC(torch.full((2, 3, 2, 2), float(index))), img_metas=DC(meta, cpu_only=True),
                    gt_bboxes_3d=DC(boxes, cpu_only=True), gt_labels_3d=DC(torch.from_numpy(labels.astype(np.int64))))


def reference_class():
    src = (REF / "nuscenes_dataset.py").read_text()
    a = src.index("class CustomNuScenesDataset(NuScenesDataset):")
    b = src.index("    def _evaluate_single(self,")
    mmcv = type("mmcv", (), dict(track_iter_progress=staticmethod(lambda x: x)))
    ns = dict(np=np, torch=torch, copy=copy, random=random, mmcv=mmcv, DC=DC, Quaternion=Quaternion,
              quaternion_yaw=quaternion_yaw, NuScenesDataset=NuScenesDataset)
    exec(src[a:b], ns)
    return ns["CustomNuScenesDataset"]


def main():
    cls = reference_class()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        ann = det_mini_nuscenes(Path(tmp))
        for pretrain in (False, True):
            ds = cls(queue_length=4, use_pretrain_data=pretrain, ann_file=ann, classes=CLASS_NAMES, use_valid_flag=True)
            out[f"usable_pretrain{int(pretrain)}"] = np.array(ds.usable_index, np.int64)
        ds = cls(queue_length=4, use_pretrain_data=False, ann_file=ann, classes=CLASS_NAMES, use_valid_flag=True)
        assert len(ds) == N_FRAMES
        for index in range(N_FRAMES):
            random.seed(SEED + index)
            ds.seen.clear()
            ret = ds.prepare_train_data(index)
            out[f"i{index}_frames"] = np.array([int(t[3:]) for t in ds.seen], np.int64)   # every frame the call touched
            out[f"i{index}_none"] = np.array(ret is None)
            if ret is None:
                continue
            metas = ret["img_metas"].data
            out[f"i{index}_img"] = ret["img"].data.numpy()
            out[f"i{index}_prev_bev_exists"] = np.array([metas[t]["prev_bev_exists"] for t in sorted(metas)])
            out[f"i{index}_can_bus"] = np.stack([np.asarray(metas[t]["can_bus"], np.float64) for t in sorted(metas)])
            out[f"i{index}_tokens"] = np.array([metas[t]["sample_idx"] for t in sorted(metas)])
            out[f"i{index}_boxes"] = ret["gt_bboxes_3d"].data.tensor.numpy()
            out[f"i{index}_labels"] = ret["gt_labels_3d"].data.numpy()
            out[f"i{index}_lidar2img"] = np.stack(metas[max(metas)]["lidar2img"])
        # the annotations of single frames before the filters (get_data_info -> ann_info)
        for index in (0, 2, 7):
            ann_info = ds.get_data_info(index)["ann_info"]
            out[f"ann{index}_boxes"] = ann_info["gt_bboxes_3d"].tensor.numpy()
            out[f"ann{index}_labels"] = ann_info["gt_labels_3d"].astype(np.int64)
    np.savez_compressed(HERE / "det_dataset.npz", **out)
    print("wrote det_dataset.npz:", {k: v.tolist() for k, v in out.items() if k.startswith("usable")},
          "items without a sample:", [i for i in range(N_FRAMES) if out[f"i{i}_none"]])


if __name__ == "__main__":
    main()
