"""CPU: the submission file and the frame changes of vidar_amd/det_evaluate.py (boxes_to_ego, ground_truth_from_infos,
write_results_json / read_results_json) on the fixture of tests/det_data_cases.py, whose lidar2ego and ego2global rotate
about all three axes.

Golden: tests/golden/det_results.json is what the reference's own output_to_nusc_box_det + lidar_nusc_box_to_global +
_format_bbox_det text wrote for the same predictions (tests/golden/make_det_results_golden.py), in fp64."""
import json
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import det_data_cases as F
from det_data_cases import gravity, qmul, rot, to_frame, ulp32, yaw_gap

GOLD = Path(__file__).parent / "golden"
EPS64 = 2.0 ** -52


@pytest.fixture(scope="module")
def infos(tmp_path_factory):
    return F.sorted_infos(F.det_mini_nuscenes(tmp_path_factory.mktemp("det_mini")))


@pytest.fixture(scope="module")
def preds():
    return [{k: torch.from_numpy(v) for k, v in F.predictions(k).items()} for k in range(F.N_FRAMES)]


@pytest.fixture(scope="module")
def written(infos, preds, tmp_path_factory):
    from vidar_amd.det_evaluate import write_results_json
    path = tmp_path_factory.mktemp("results") / "sub" / "results_nusc.json"
    kept = write_results_json(path, [i["token"] for i in infos], preds, infos, F.CLASS_NAMES)
    return path, kept


def test_boxes_to_ego_by_hand():
    from vidar_amd.det_evaluate import boxes_to_ego
    a = 0.7
    rows = torch.tensor([[1.0, 2.0, 3.0, 1.5, 4.0, 1.25, 0.3, 2.0, -1.0], [-5.0, 0.5, -1.0, 0.5, 0.5, 1.0, 3.5, 0.0, 0.0]])
    out = boxes_to_ego(rows, [math.cos(a / 2), 0.0, 0.0, math.sin(a / 2)], [10.0, -20.0, 0.5]).numpy().astype(np.float64)
    c, s = math.cos(a), math.sin(a)
    want_xy = np.array([[c * 1.0 - s * 2.0 + 10.0, s * 1.0 + c * 2.0 - 20.0], [c * -5.0 - s * 0.5 + 10.0, s * -5.0 + c * 0.5 - 20.0]])
    assert (np.abs(out[:, :2] - want_xy) <= ulp32(want_xy)).all()
    np.testing.assert_array_equal(out[:, 2], [3.5, -0.5])
    np.testing.assert_array_equal(out[:, 3:6], rows[:, 3:6].numpy())                          # sizes untouched
    # a rotation about z adds its yaw to the heading -yaw - pi/2: the row's yaw goes DOWN by it
    assert (yaw_gap(out[:, 6], rows[:, 6].numpy().astype(np.float64) - a) <= ulp32(3 * np.pi / 2)).all()
    want_v = np.array([[c * 2.0 + s * 1.0, s * 2.0 - c * 1.0], [0.0, 0.0]])
    assert (np.abs(out[:, 7:] - want_v) <= ulp32(want_v) + 1e-300).all()
    assert out.dtype == np.float64 and boxes_to_ego(rows, [1.0, 0, 0, 0], [0, 0, 0]).dtype == torch.float32
    # one rotation / translation per box
    per = boxes_to_ego(rows, [[1.0, 0, 0, 0], [math.cos(a / 2), 0.0, 0.0, math.sin(a / 2)]], [[0.0, 0, 0], [10.0, -20.0, 0.5]])
    np.testing.assert_array_equal(per[0, :6].numpy(), rows[0, :6].numpy())
    np.testing.assert_array_equal(per[1].numpy(), out[1].astype(np.float32))


def test_written_file_equals_the_reference_text(infos, preds, written):
    path, kept = written
    doc, gold = json.loads(path.read_text()), json.loads((GOLD / "det_results.json").read_text())
    assert set(doc) == {"meta", "results"} and doc["meta"] == gold["meta"]
    assert list(doc["results"]) == list(gold["results"]) == [i["token"] for i in infos]
    n = 0
    for k, token in enumerate(doc["results"]):
        got, want = doc["results"][token], gold["results"][token]
        assert kept[k].tolist() == gold["kept"][token] and len(got) == len(want)
        for g, w in zip(got, want):
            assert list(g) == ["sample_token", "translation", "size", "rotation", "velocity", "detection_name",
                               "detection_score", "attribute_name"]
            assert (g["sample_token"], g["detection_name"], g["attribute_name"]) == (token, w["detection_name"], w["attribute_name"])
            assert g["detection_score"] == w["detection_score"] and g["size"] == w["size"]     # fp32 values, carried over
            for key in ("translation", "rotation", "velocity"):                                 # fp64 against fp64: one
                gap = np.abs(np.array(g[key]) - np.array(w[key]))                               # fp32 ulp of the vector
                assert (gap <= ulp32(np.abs(w[key]).max())).all(), (token, key, g[key], w[key])
            n += 1
    assert 200 < n < 40 * F.N_FRAMES                       # the class-range filter dropped some and kept most


def test_read_back_and_inverse_transform_give_the_ego_frame_boxes(infos, preds, written):
    """Bound, from the arithmetic: the file holds fp64 global values; undoing ego2global subtracts a translation of up to
    1700 m, which leaves an absolute error of a few eps64 * 1700 in the centre; both sides are then rounded to fp32, which
    can land two fp64 values that close on neighbouring floats: one fp32 ulp of the value.  Sizes are fp32 values on both
    sides: equal.  The yaw is compared modulo 2 pi at the largest magnitude a row's yaw takes (3 pi / 2).
    The velocity is the one field the layout itself truncates: it keeps two components of the GLOBAL-frame velocity, and
    with a tilted ego2global the dropped vertical component v_z does not come back -- the inverse rotation R^T spreads the
    missing R^T[:, 2] v_z over the ego components, |R[2, j]| |v_z| on component j, which is added to that field's bound."""
    from vidar_amd.det_evaluate import ATTRIBUTES, boxes_to_ego, read_results_json
    path, kept = written
    tokens, glob = read_results_json(path)
    tokens2, ego = read_results_json(path, infos, F.CLASS_NAMES)
    assert tokens == tokens2 == [i["token"] for i in infos]
    slack = 16 * EPS64 * 1700.0
    doc = json.loads(path.read_text())["results"]
    for k, info in enumerate(infos):
        rows = torch.from_numpy(gravity(preds[k]["boxes"].numpy()))
        want = boxes_to_ego(rows, info["lidar2ego_rotation"], info["lidar2ego_translation"])[kept[k]].numpy().astype(np.float64)
        # this package's transform against the numpy restatement above
        mine = to_frame(rows.numpy()[kept[k].numpy()], info["lidar2ego_rotation"], info["lidar2ego_translation"])
        assert (np.abs(want[:, [0, 1, 2, 7, 8]] - mine[:, [0, 1, 2, 7, 8]]) <= ulp32(mine[:, [0, 1, 2, 7, 8]]) + slack).all()
        assert (yaw_gap(want[:, 6], mine[:, 6]) <= ulp32(3 * np.pi / 2)).all()
        # the inverse of ego2global, done here: centres / velocities with R^T, the orientation on quaternions
        g = glob[k]
        conj = np.asarray(info["ego2global_rotation"], np.float64) * [1, -1, -1, -1]
        R = rot(info["ego2global_rotation"])
        c = (np.array([e["translation"] for e in doc[tokens[k]]]).reshape(-1, 3) - info["ego2global_translation"]) @ R
        v = np.array([e["velocity"] + [0.0] for e in doc[tokens[k]]]).reshape(-1, 3) @ R
        v_lidar = np.concatenate([rows.numpy()[kept[k].numpy(), 7:9].astype(np.float64), np.zeros((len(v), 1))], 1)
        v_z = (v_lidar @ rot(info["lidar2ego_rotation"]).T @ R.T)[:, 2]                          # what the file does not hold
        v_slack = slack + np.abs(R[2, :2])[None, :] * np.abs(v_z)[:, None]
        assert v_slack.max() > 1e-4                                                              # the tilt is no rounding matter
        head = np.array([rot(qmul(conj, e["rotation"]))[:, 0] for e in doc[tokens[k]]]).reshape(-1, 3)
        yaw = -np.arctan2(head[:, 1], head[:, 0]) - np.pi / 2
        assert (np.abs(c - want[:, :3]) <= ulp32(want[:, :3]) + slack).all()
        assert (np.abs(v[:, :2] - want[:, 7:]) <= ulp32(want[:, 7:]) + v_slack).all()
        assert (yaw_gap(yaw, want[:, 6]) <= ulp32(3 * np.pi / 2)).all()
        np.testing.assert_array_equal(g["boxes"][:, 3:6].numpy(), rows.numpy()[kept[k].numpy(), 3:6])
        # read_results_json(path, infos) does the same inverse itself
        e = ego[k]["boxes"].numpy().astype(np.float64)
        assert (np.abs(e[:, :3] - want[:, :3]) <= ulp32(want[:, :3]) + slack).all()
        assert (np.abs(e[:, 7:] - want[:, 7:]) <= ulp32(want[:, 7:]) + v_slack).all()
        assert (yaw_gap(e[:, 6], want[:, 6]) <= ulp32(3 * np.pi / 2)).all()
        np.testing.assert_array_equal(e[:, 3:6], want[:, 3:6])
        assert torch.equal(ego[k]["scores"], preds[k]["scores"][kept[k]]) and torch.equal(ego[k]["labels"], preds[k]["labels"][kept[k]])
        assert ego[k]["attrs"].tolist() == [ATTRIBUTES.index(x["attribute_name"]) if x["attribute_name"] else -1 for x in doc[tokens[k]]]
        assert not np.allclose(g["boxes"][:, :2].numpy(), e[:, :2], atol=1.0)                  # the frames really differ


def test_class_range_is_taken_in_the_ego_frame(infos, preds, written):
    """the calibration moves some boxes across their class range: the LiDAR-frame radius would decide them differently"""
    from vidar_amd.det_evaluate import CONFIGS
    _, kept = written
    rng = CONFIGS["detection_cvpr_2019"]["class_range"]
    differ = 0
    for k, info in enumerate(infos):
        rows = gravity(preds[k]["boxes"].numpy())
        ego = to_frame(rows, info["lidar2ego_rotation"], info["lidar2ego_translation"])
        limit = np.array([rng[F.CLASS_NAMES[l]] for l in preds[k]["labels"].tolist()], np.float64)
        inside = np.hypot(ego[:, 0], ego[:, 1]) <= limit
        assert np.flatnonzero(inside).tolist() == kept[k].tolist()
        differ += int((inside != (np.hypot(rows[:, 0].astype(np.float64), rows[:, 1].astype(np.float64)) <= limit)).sum())
    assert differ > 0


def test_ground_truth_from_infos(infos):
    from vidar_amd.det_evaluate import ground_truth_from_infos
    gt = ground_truth_from_infos(infos, F.CLASS_NAMES, device="cpu")
    assert len(gt) == len(infos)
    for info, g in zip(infos, gt):
        keep = np.array([n in F.CLASS_NAMES for n in info["gt_names"]])
        assert keep.sum() == len(info["gt_names"]) - 2 == len(g["labels"])                      # every box but the two unknown names,
        assert g["labels"].tolist() == [F.CLASS_NAMES.index(n) for n in info["gt_names"][keep]]   # valid_flag or not
        assert g["num_pts"].tolist() == (info["num_lidar_pts"] + info["num_radar_pts"])[keep].tolist() and "attrs" not in g
        rows = np.concatenate([info["gt_boxes"], info["gt_velocity"]], 1)[keep].astype(np.float32)
        want = to_frame(rows, info["lidar2ego_rotation"], info["lidar2ego_translation"])
        got = g["boxes"].numpy().astype(np.float64)
        assert g["boxes"].dtype == torch.float32
        nan = np.isnan(want[:, 7])
        assert nan.any() and np.array_equal(np.isnan(got[:, 7:]), np.stack([nan, nan], 1))       # a NaN velocity stays NaN
        cols = [0, 1, 2, 7, 8]
        assert (np.nan_to_num(np.abs(got[:, cols] - want[:, cols])) <= np.nan_to_num(ulp32(want[:, cols])) + 1e-12).all()
        assert (yaw_gap(got[:, 6], want[:, 6]) <= ulp32(3 * np.pi / 2)).all()
        np.testing.assert_array_equal(got[:, 3:6], rows[:, 3:6])
    assert ground_truth_from_infos([], F.CLASS_NAMES, device="cpu") == []
    lidar_only = {k: v for k, v in infos[0].items() if k != "num_radar_pts"}              # as ann_info: lidar counts alone
    keep = np.array([n in F.CLASS_NAMES for n in infos[0]["gt_names"]])
    assert ground_truth_from_infos([lidar_only], F.CLASS_NAMES, "cpu")[0]["num_pts"].tolist() == infos[0]["num_lidar_pts"][keep].tolist()
    k = 1                                                  # frame 2 has no VALID box, but its annotations are all scored
    assert len(gt[F.EMPTY_FRAME]["labels"]) > 0 and int((gt[k]["num_pts"] == 0).sum()) >= 1


def test_summary_says_when_the_ground_truth_has_no_attributes():
    from vidar_amd.det_evaluate import format_summary, summarize
    aps = {n: {0.5: 0.1, 1.0: 0.2, 2.0: 0.3, 4.0: 0.4} for n in F.CLASS_NAMES}
    tps = {n: dict(trans_err=0.5, scale_err=0.5, orient_err=0.5, vel_err=0.5, attr_err=1.0) for n in F.CLASS_NAMES}
    res = summarize(aps, tps)
    plain, noted = format_summary(res), format_summary(res, gt_attrs=False)
    assert noted.startswith(plain) and len(noted.splitlines()) == len(plain.splitlines()) + 1
    assert "mAAE is 1" in noted.splitlines()[-1] and "attributes" in noted.splitlines()[-1] and "mAAE is 1" not in plain


def test_mismatched_tokens_and_missing_frames_raise(infos, preds, written, tmp_path):
    from vidar_amd.det_evaluate import read_results_json, write_results_json
    with pytest.raises(ValueError, match="tok1"):
        write_results_json(tmp_path / "x.json", ["tok1"], preds[:1], infos[:1], F.CLASS_NAMES)
    write_results_json(tmp_path / "y.json", ["tok0"], preds[:1], infos[:1], F.CLASS_NAMES)
    with pytest.raises(KeyError, match="tok1"):
        read_results_json(tmp_path / "y.json", infos[:2], F.CLASS_NAMES)
