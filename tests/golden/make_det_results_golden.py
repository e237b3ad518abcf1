"""Golden for vidar_amd.det_evaluate.write_results_json from the reference's own text: output_to_nusc_box_det and
lidar_nusc_box_to_global (UniAD/projects/mmdet3d_plugin/datasets/data_utils/data_utils.py:53-132) and _format_bbox_det
(UniAD/projects/mmdet3d_plugin/datasets/nuscenes_e2e_dataset.py:873-945), executed in place on the predictions and the
calibration of tests/det_data_cases.py.
pyquaternion, the devkit's Box, mmdet3d and mmcv are not installable.  What the executed text needs from them is restated
here and labelled [3P]: Quaternion (axis / radians and element constructors, product, rotation_matrix), Box (rotate,
translate), LiDARInstance3DBoxes (gravity_center, dims, yaw), DefaultAttribute, the class ranges of
detection_cvpr_2019 and mmcv's progress / dump helpers.  Writes data only (det_results.json: the submission document the
reference's text produced, in fp64, and the indices it kept).
    python tests/golden/make_det_results_golden.py"""
import copy
import json
import math
import sys
import tempfile
from os import path as osp
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
REF = Path("/root/reference/UniAD/projects/mmdet3d_plugin/datasets")

from det_data_cases import CLASS_NAMES, N_FRAMES, det_mini_nuscenes, predictions, sorted_infos  # noqa: E402


class Quaternion:                            # [3P] pyquaternion
    def __init__(self, *args, axis=None, radians=None):
        if axis is not None:
            axis = np.asarray(axis, np.float64)
            axis = axis / np.linalg.norm(axis)
            theta = radians / 2.0                # pyquaternion takes cos / sin from `math`: doubles
            self.q = np.concatenate([[math.cos(theta)], axis * math.sin(theta)])
        else:
            self.q = np.asarray(args[0].q if isinstance(args[0], Quaternion) else args[0], np.float64).copy()

    def __mul__(self, other):
        aw, ax, ay, az = self.q
        bw, bx, by, bz = other.q
        return Quaternion([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                           aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])

    @property
    def elements(self):
        return self.q

    @property
    def rotation_matrix(self):
        w, x, y, z = self.q / np.linalg.norm(self.q)
        return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


class NuScenesBox:                           # [3P] nuscenes.utils.data_classes.Box
    def __init__(self, center, size, orientation, label=np.nan, score=np.nan, velocity=(np.nan, np.nan, np.nan)):
        self.center, self.wlh, self.orientation = np.array(center), np.array(size), orientation
        self.label = int(label) if not np.isnan(label) else label
        self.score = float(score) if not np.isnan(score) else score
        self.velocity = np.array(velocity)

    def translate(self, x):
        self.center = self.center + x

    def rotate(self, quaternion):
        self.center = np.dot(quaternion.rotation_matrix, self.center)
        self.orientation = quaternion * self.orientation
        self.velocity = np.dot(quaternion.rotation_matrix, self.velocity)


class LiDARInstance3DBoxes:                  # [3P] mmdet3d, as far as output_to_nusc_box_det reads it
    def __init__(self, tensor):
        self.tensor = torch.as_tensor(tensor, dtype=torch.float32)

    @property
    def gravity_center(self):
        bottom = self.tensor[:, :3]
        gc = torch.zeros_like(bottom)
        gc[:, :2] = bottom[:, :2]
        gc[:, 2] = bottom[:, 2] + self.tensor[:, 5] * 0.5
        return gc

    dims = property(lambda self: self.tensor[:, 3:6])
    yaw = property(lambda self: self.tensor[:, 6])

    def __len__(self):
        return self.tensor.shape[0]


class NuScenesDataset:                       # [3P] mmdet3d
    DefaultAttribute = {"car": "vehicle.parked", "pedestrian": "pedestrian.moving", "trailer": "vehicle.parked",
                        "truck": "vehicle.parked", "bus": "vehicle.moving", "motorcycle": "cycle.without_rider",
                        "construction_vehicle": "vehicle.parked", "bicycle": "cycle.without_rider", "barrier": "",
                        "traffic_cone": ""}


CLASS_RANGE = {"car": 50, "truck": 50, "bus": 50, "trailer": 50, "construction_vehicle": 50, "pedestrian": 40,
               "motorcycle": 40, "bicycle": 40, "traffic_cone": 30, "barrier": 30}      # [3P] detection_cvpr_2019.json


def main():
    usrc = (REF / "data_utils/data_utils.py").read_text()
    a, b = usrc.index("def output_to_nusc_box_det(detection):"), usrc.index("def obtain_map_info(")
    ns = dict(np=np, Quaternion=Quaternion, NuScenesBox=NuScenesBox)
    exec(usrc[a:b], ns)
    kept = []
    to_global = ns["lidar_nusc_box_to_global"]

    def recording(*args, **kw):
        boxes, keep_idx = to_global(*args, **kw)
        kept.append([int(i) for i in keep_idx])
        return boxes, keep_idx
    dsrc = (REF / "nuscenes_e2e_dataset.py").read_text()
    a, b = dsrc.index("    def _format_bbox_det(self, results, jsonfile_prefix=None):"), dsrc.index("    def format_results_det(self,")
    dumped = {}
    mmcv = type("mmcv", (), dict(track_iter_progress=staticmethod(lambda x: x), mkdir_or_exist=staticmethod(lambda p: None),
                                 dump=staticmethod(lambda obj, path: dumped.update(doc=obj))))
    ns.update(copy=copy, osp=osp, mmcv=mmcv, NuScenesDataset=NuScenesDataset, lidar_nusc_box_to_global=recording)
    exec("class E2E:\n" + dsrc[a:b], ns)
    with tempfile.TemporaryDirectory() as tmp:
        infos = sorted_infos(det_mini_nuscenes(Path(tmp)))
    ds = ns["E2E"]()
    ds.CLASSES, ds.data_infos, ds.eval_version = list(CLASS_NAMES), infos, "detection_cvpr_2019"
    ds.eval_detection_configs = type("C", (), dict(class_range=CLASS_RANGE))()
    ds.modality = dict(use_lidar=False, use_camera=True, use_radar=False, use_map=False, use_external=True)
    results = []
    for k in range(N_FRAMES):
        p = predictions(k)
        results.append(dict(boxes_3d=LiDARInstance3DBoxes(p["boxes"]), scores_3d=torch.from_numpy(p["scores"]),
                            labels_3d=torch.from_numpy(p["labels"])))
    ds._format_bbox_det(results, "unused")
    doc = dumped["doc"]
    plain = lambda v: [float(x) for x in v]
    for entries in doc["results"].values():
        for e in entries:
            for key in ("translation", "size", "rotation", "velocity"):
                e[key] = plain(e[key])
            e["detection_score"] = float(e["detection_score"])
    doc["kept"] = {info["token"]: kept[k] for k, info in enumerate(infos)}
    (HERE / "det_results.json").write_text(json.dumps(doc))
    print("wrote det_results.json:", sum(len(v) for v in doc["results"].values()), "of", 40 * N_FRAMES, "boxes kept;",
          sorted({e["attribute_name"] for v in doc["results"].values() for e in v}))


if __name__ == "__main__":
    main()
