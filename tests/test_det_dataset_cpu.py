"""CPU: the detection fine-tune data set (vidar_amd/data/annotations.py, det_dataset.py) on the fixture of
tests/det_data_cases.py.

Against the reference's own CustomNuScenesDataset text (tests/golden/make_det_dataset_golden.py -> det_dataset.npz): the
usable-index scans, and per item the frames of the queue, prev_bev_exists, can_bus, lidar2img and the boxes / labels of the
kept frame -- all compared EXACTLY: boxes are float32 on both sides (mmdet3d's LiDARInstance3DBoxes casts them as this
package does) and can_bus / lidar2img are float64 on both sides, so no field passes through a cast the reference lacks.
The mmdet3d steps themselves ([3P], restated on both sides) are checked against hand-written cases."""
import pickle
import random
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import det_data_cases as F

GOLD = Path(__file__).parent / "golden"
sys.path.insert(0, str(GOLD))
SEED = 1000                                   # make_det_dataset_golden.SEED


@pytest.fixture(scope="module")
def ann(tmp_path_factory):
    return F.det_mini_nuscenes(tmp_path_factory.mktemp("det_mini"))


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD / "det_dataset.npz")


def dataset(ann, **kw):
    from vidar_amd.data import DetectionSequenceDataset
    return DetectionSequenceDataset(ann, **dict(dict(queue_length=4, use_valid_flag=True, class_names=F.CLASS_NAMES), **kw))


def test_usable_indices_match_the_reference_scan(ann, gold):
    assert dataset(ann).usable_index == gold["usable_pretrain0"].tolist() == list(range(F.N_FRAMES))
    ds = dataset(ann, use_pretrain_data=True)
    assert ds.usable_index == gold["usable_pretrain1"].tolist() and len(ds) == 1
    assert ds.flag.tolist() == [0]                         # what the group sampler reads
    assert len(dataset(ann, load_interval=2).infos) == F.N_FRAMES // 2


@pytest.mark.parametrize("index", range(F.N_FRAMES))
def test_training_item_matches_the_reference_text(ann, gold, index):
    from vidar_amd.data.det_dataset import queue_indices
    ds = dataset(ann)
    frames = gold[f"i{index}_frames"].tolist()
    random.seed(SEED + index)
    assert queue_indices(index, 4)[:len(frames)] == frames  # the reference stops at the first frame without a box
    random.seed(SEED + index)
    item = ds.prepare_train_data(index)
    assert (item is None) == bool(gold[f"i{index}_none"])
    if item is None:
        assert frames[-1] == F.EMPTY_FRAME
        return
    metas = item["img_metas"]
    assert sorted(metas) == [0, 1, 2, 3] and [metas[t]["sample_idx"] for t in range(4)] == gold[f"i{index}_tokens"].tolist()
    assert [metas[t]["prev_bev_exists"] for t in range(4)] == gold[f"i{index}_prev_bev_exists"].tolist()
    np.testing.assert_array_equal(np.stack([metas[t]["can_bus"] for t in range(4)]), gold[f"i{index}_can_bus"])
    np.testing.assert_array_equal(np.stack(metas[3]["lidar2img"]), gold[f"i{index}_lidar2img"])
    boxes = item["gt_bboxes_3d"].tensor.numpy()
    assert boxes.dtype == np.float32 and item["gt_labels_3d"].dtype == torch.int64
    np.testing.assert_array_equal(boxes, gold[f"i{index}_boxes"])
    np.testing.assert_array_equal(item["gt_labels_3d"].numpy(), gold[f"i{index}_labels"])
    # the images of the queue are stacked in its order (the golden's stand-in image holds the frame index)
    assert item["img"].shape == (4, 2, 3, 64, 64)
    for t, k in enumerate(gold[f"i{index}_img"][:, 0, 0, 0, 0].astype(int).tolist()):
        assert torch.equal(item["img"][t], ds.frame(k)["img"])


def test_golden_covers_scene_change_clamp_and_both_branches(gold):
    kept = [i for i in range(F.N_FRAMES) if not gold[f"i{i}_none"]]
    assert 0 < len(kept) < F.N_FRAMES
    assert any(not gold[f"i{i}_prev_bev_exists"][1:].all() for i in kept)            # a scene change inside a queue
    assert any(len(set(gold[f"i{i}_frames"].tolist())) < 4 for i in kept)            # the clamp at index 0 repeats a frame
    assert all(not gold[f"i{i}_prev_bev_exists"][0] for i in kept)


@pytest.mark.parametrize("index", [0, 2, 7])
def test_ann_info_matches_the_restated_base_class(ann, gold, index):
    from vidar_amd.data.annotations import ann_info
    info = F.sorted_infos(ann)[index]
    boxes, labels, num_pts = ann_info(info, F.CLASS_NAMES, use_valid_flag=True)
    np.testing.assert_array_equal(boxes, gold[f"ann{index}_boxes"])
    np.testing.assert_array_equal(labels, gold[f"ann{index}_labels"])
    assert boxes.dtype == np.float32 and labels.dtype == np.int64 and len(num_pts) == len(labels)
    if index == F.EMPTY_FRAME:
        assert boxes.shape == (0, 9)


def test_ann_info_by_hand():
    from vidar_amd.data.annotations import ann_info
    info = dict(gt_boxes=np.array([[1.0, 2.0, 0.5, 2.0, 4.0, 1.5, 0.3], [5.0, 6.0, -1.0, 1.0, 1.0, 2.0, -0.2], [9.0, 9.0, 0.0, 1.0, 1.0, 1.0, 0.0]]),
                gt_names=np.array(["car", "animal", "pedestrian"]), gt_velocity=np.array([[np.nan, np.nan], [1.0, -2.0], [0.5, 0.25]]),
                num_lidar_pts=np.array([3, 0, 7]), num_radar_pts=np.array([1, 2, 0]), valid_flag=np.array([True, True, False]))
    boxes, labels, num_pts = ann_info(info, F.CLASS_NAMES, use_valid_flag=True)
    assert labels.tolist() == [0, -1] and num_pts.tolist() == [4, 2]                 # valid_flag mask; unknown name -> -1
    np.testing.assert_array_equal(boxes[0], np.array([1.0, 2.0, 0.5 - 0.75, 2.0, 4.0, 1.5, 0.3, 0.0, 0.0], np.float32))   # NaN -> 0, z to the bottom
    np.testing.assert_array_equal(boxes[1, [2, 7, 8]], np.array([-2.0, 1.0, -2.0], np.float32))
    boxes, labels, num_pts = ann_info(info, F.CLASS_NAMES, use_valid_flag=False)     # num_lidar_pts > 0 instead
    assert labels.tolist() == [0, 8] and num_pts.tolist() == [4, 7]
    assert ann_info(info, F.CLASS_NAMES, True, with_velocity=False)[0].shape == (2, 7)


def test_range_filter_is_strict_and_wraps_the_yaw():
    from vidar_amd.data.annotations import object_name_filter, object_range_filter
    pi = np.float32(np.pi)
    rows = [(51.2, 0.0, 0.1), (-51.2, 0.0, 0.1), (0.0, 51.2, 0.1), (0.0, -51.2, 0.1),          # on a bound: out
            (51.2001, 0.0, 0.1), (0.0, -51.3, 0.1),                                              # beyond: out
            (51.19, 51.19, 3.5), (-51.19, -51.19, -4.0), (1.0, 1.0, np.pi), (2.0, 2.0, -np.pi), (3.0, 3.0, 7.0)]
    boxes = np.zeros((len(rows), 9), np.float32)
    boxes[:, [0, 1, 6]] = np.array(rows, np.float32)
    boxes[:, 3:6] = 1.0
    labels = np.arange(len(rows)) - 7                      # the kept rows get labels -1, 0, 1, 2, 3
    out, lab = object_range_filter(boxes, labels, F.PC_RANGE)
    assert lab.tolist() == [-1, 0, 1, 2, 3] and out.dtype == np.float32
    two_pi = np.float32(2 * np.pi)
    want = [np.float32(3.5) - two_pi, np.float32(-4.0) + two_pi, -pi, -pi, np.float32(7.0) - two_pi]
    np.testing.assert_array_equal(out[:, 6], np.array(want, np.float32))                        # [-pi, pi): +pi wraps, -pi stays
    assert (out[:, 6] >= -pi).all() and (out[:, 6] < pi).all()
    np.testing.assert_array_equal(out[:, :6], boxes[6:, :6])
    out2, lab2 = object_name_filter(out, lab)
    assert lab2.tolist() == [0, 1, 2, 3] and np.array_equal(out2, out[1:])                      # label -1 dropped


def test_getitem_draws_another_index_for_an_empty_frame(ann):
    ds = dataset(ann)
    random.seed(0)
    assert ds.prepare_train_data(F.EMPTY_FRAME) is None
    random.seed(0); np.random.seed(0)
    item = ds[F.EMPTY_FRAME]                               # the filter_empty_gt loop: another index, not None
    assert item is not None and len(item["gt_labels_3d"]) > 0 and bool((item["gt_labels_3d"] >= 0).all())
    assert item["img_metas"][3]["sample_idx"] != f"tok{F.EMPTY_FRAME}"
    assert dataset(ann, filter_empty_gt=False).prepare_train_data(F.EMPTY_FRAME) is not None


def test_a_file_without_boxes_raises_after_a_bounded_number_of_draws(ann, tmp_path):
    with open(ann, "rb") as f:
        data = pickle.load(f)
    for info in data["infos"]:
        info["valid_flag"] = np.zeros_like(info["valid_flag"])
    bad = tmp_path / "no_boxes.pkl"
    with open(bad, "wb") as f:
        pickle.dump(data, f)
    ds = dataset(bad)
    calls = []
    real = ds.prepare_train_data
    ds.prepare_train_data = lambda i: (calls.append(i), real(i))[1]
    np.random.seed(0)
    with pytest.raises(RuntimeError, match="no_boxes.pkl"):
        ds[5]
    assert len(calls) == ds.MAX_DRAWS


def test_test_mode_items_are_single_frames_with_absolute_poses(ann):
    from vidar_amd.data.loader import DistributedSampler, collate
    ds = dataset(ann, test_mode=True)
    assert len(ds) == F.N_FRAMES
    item = ds[7]
    assert sorted(item) == ["img", "img_metas"] and item["img"].shape == (2, 3, 64, 64)
    m = item["img_metas"]
    assert m["sample_idx"] == "tok7" and m["scene_token"] == "scene-b"
    np.testing.assert_array_equal(m["can_bus"][:3], F.ego2global(7)["translation"])
    assert list(DistributedSampler(ds, 2, 1)) == list(range(8, 16))                  # contiguous shards: scene order kept
    b = collate([item])
    assert sorted(b) == ["img", "img_metas"] and b["img"].shape == (1, 2, 3, 64, 64)


def test_collate_carries_boxes_as_per_sample_lists(ann):
    from vidar_amd.data.loader import build_dataloader
    for device_images in (False, True):
        ds = dataset(ann, use_pretrain_data=True, augment=True, device_images=device_images)
        random.seed(0); np.random.seed(0)
        batch = next(iter(build_dataloader(ds, 1, 0, 1, 0, seed=0)))
        assert sorted(batch) == sorted((["img_raw", "img_plan"] if device_images else ["img"]) + ["img_metas", "gt_bboxes_3d", "gt_labels_3d"])
        assert len(batch["gt_bboxes_3d"]) == 1 and batch["gt_bboxes_3d"][0].tensor.shape[1] == 9
        assert batch["gt_labels_3d"][0].dtype == torch.int64 and batch["img_metas"][0][3]["sample_idx"] == "tok10"


def test_recipes_and_released_files_name_the_same_data_set_arguments():
    from vidar_amd.configs import dataset_kwargs, get_config
    k = dataset_kwargs(get_config("finetune/vidar_1_8_nusc_1future"))
    assert k == dict(queue_length=4, test_mode=False, load_interval=1, class_names=F.CLASS_NAMES, point_cloud_range=F.PC_RANGE,
                     use_valid_flag=True, use_pretrain_data=True)
    assert not dataset_kwargs(get_config("finetune/vidar_full_nusc_1future"))["use_pretrain_data"]
    t = dataset_kwargs(get_config("finetune/vidar_1_8_nusc_3future"), test_mode=True)
    assert t["test_mode"] and not t["use_valid_flag"] and not t["use_pretrain_data"] and t["queue_length"] == 4
    ref = Path("/root/reference/projects/configs/vidar_finetune")
    if ref.exists():
        from vidar_amd.plugin.config import Config
        for sub, name, recipe in (("nusc_1_4_subset", "vidar_1_8_nusc_1future", None), ("nusc_1_4_subset", "vidar_1_8_nusc_3future", None),
                                  ("nusc_fullset", "vidar_full_nusc_1future", None),
                                  ("nusc_1_4_subset", "bevformer_1_4_baseline", "vidar_1_8_nusc_1future")):
            cfg = Config.fromfile(str(ref / sub / f"{name}.py"))
            meta = get_config(f"finetune/{recipe or name}")
            for test in (False, True):
                assert dataset_kwargs(meta, test, cfg) == dataset_kwargs(meta, test), (name, test)
        # a key the file leaves out is the data set's default, not the named recipe's
        full = Config.fromfile(str(ref / "nusc_fullset" / "vidar_full_nusc_1future.py"))
        assert not dataset_kwargs(get_config("finetune/vidar_1_8_nusc_1future"), False, full)["use_pretrain_data"]
