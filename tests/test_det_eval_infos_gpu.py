"""GPU: detection scoring from an info pkl (det_evaluate.ground_truth_from_infos / boxes_to_ego / the submission file and
tools/test.py --ann-file) on the fixture of tests/det_data_cases.py, against the independent restatement of the devkit in
tests/det_eval_cases.py, to the tolerance tests/test_det_eval_gpu.py uses for that restatement."""
import contextlib
import copy
import importlib.util
import io
import json
import math
from pathlib import Path

import numpy as np
import pytest
import torch

import det_data_cases as F
import det_eval_cases as D
from det_data_cases import to_frame
from test_det_eval_gpu import compare_metrics

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
MARGIN = 1e-3


@pytest.fixture(scope="module", autouse=True)
def deterministic_library_convolutions():
    """the two launcher runs below are compared bit for bit; the library's FPN convolutions repeat their bits only under this
    switch (tests/test_det_finetune_data_gpu.py)"""
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = before


@pytest.fixture(scope="module")
def ann(tmp_path_factory):
    return F.det_mini_nuscenes(tmp_path_factory.mktemp("det_mini"))


@pytest.fixture(scope="module")
def infos(ann):
    return F.sorted_infos(ann)


def lidar_predictions(info, k):
    """gravity-centred LiDAR-frame rows (float32) scattered around the frame's annotations at chosen distances, plus a few
    far from everything"""
    rng = np.random.default_rng(700 + k)
    rows, labels, dist = [], [], []
    gt = np.concatenate([info["gt_boxes"], np.nan_to_num(info["gt_velocity"])], 1)
    for row, name in zip(gt, info["gt_names"]):
        if name not in F.CLASS_NAMES or rng.random() < 0.25:
            continue
        d, a = rng.choice([0.2, 0.7, 1.4, 3.0, 5.5]), rng.uniform(0, 2 * np.pi)
        new = row.copy()
        new[:2] += [d * np.cos(a), d * np.sin(a)]
        new[3:6] *= rng.uniform(0.85, 1.15, 3)
        new[6] += rng.normal(0, 0.3)
        new[7:] += rng.normal(0, 0.4, 2)
        rows.append(new); dist.append(d)
        labels.append(F.CLASS_NAMES.index(name) if rng.random() < 0.9 else int(rng.integers(0, 10)))
    for _ in range(5):
        label = int(rng.integers(0, 10))
        rows.append(np.concatenate([rng.uniform(-45, 45, 2), rng.uniform(-2, 0.5, 1), F.SIZES[F.CLASS_NAMES[label]],
                                    rng.uniform(-3, 3, 1), rng.normal(0, 1, 2)]))
        labels.append(label); dist.append(8.0)
    scores = np.clip(0.9 - 0.1 * np.array(dist) + rng.uniform(-0.08, 0.08, len(dist)), 0.01, 0.99).astype(np.float32)
    assert len(set(scores.tolist())) == len(scores)        # closer boxes score higher, no ties
    return dict(boxes=np.array(rows, np.float32), labels=np.array(labels, np.int64), scores=scores)


def ego_case(infos, lidar2ego=None):
    """the case as the restatement takes it: every box moved into the ego frame HERE, numpy fp64, stored as float32"""
    pred, gt = [], []
    for k, info in enumerate(infos):
        q, t = lidar2ego(info) if lidar2ego else (info["lidar2ego_rotation"], info["lidar2ego_translation"])
        p = lidar_predictions(info, k)
        pred.append(dict(boxes=to_frame(p["boxes"], q, t).astype(np.float32), labels=p["labels"], scores=p["scores"]))
        keep = np.array([n in F.CLASS_NAMES for n in info["gt_names"]])
        rows = np.concatenate([info["gt_boxes"], info["gt_velocity"]], 1)[keep].astype(np.float32)
        gt.append(dict(boxes=to_frame(rows, q, t).astype(np.float32),
                       labels=np.array([F.CLASS_NAMES.index(n) for n in info["gt_names"][keep]], np.int64),
                       num_pts=(info["num_lidar_pts"] + info["num_radar_pts"])[keep].astype(np.int64)))
    return dict(pred=pred, gt=gt)


def assert_decisions_have_margin(case):
    """no centre distance within MARGIN of a matching threshold, no box within MARGIN of its class range, no two candidates of
    a prediction within MARGIN of each other: fp32 and fp64 arithmetic, and the reference itself, decide the case alike"""
    pairs = 0
    for p, g in zip(case["pred"], case["gt"]):
        for boxes, labels in ((p["boxes"], p["labels"]), (g["boxes"], g["labels"])):
            radius = np.hypot(boxes[:, 0].astype(np.float64), boxes[:, 1].astype(np.float64))
            limit = np.array([D.CLASS_RANGE[F.CLASS_NAMES[l]] for l in labels], np.float64)
            assert (np.abs(radius - limit) > MARGIN).all()
        for i in range(len(p["labels"])):
            same = g["labels"] == p["labels"][i]
            d = np.sort(np.hypot(*(g["boxes"][same, :2].astype(np.float64) - p["boxes"][i, :2].astype(np.float64)).T))
            assert all((np.abs(d - th) > MARGIN).all() for th in D.DIST_THS)
            near = d[d < max(D.DIST_THS) + 1.0]
            assert (np.diff(near) > MARGIN).all()
            pairs += int((d < D.DIST_TH_TP).sum())
    assert pairs > 50                                      # and the case is not empty of matches


def on_device(case):
    dev = torch.device("cuda", 0)
    return [{k: torch.from_numpy(v).to(dev) for k, v in p.items()} for p in case["pred"]]


def device_predictions(infos, lidar2ego=None):
    from vidar_amd.det_evaluate import boxes_to_ego
    dev = torch.device("cuda", 0)
    out = []
    for k, info in enumerate(infos):
        q, t = lidar2ego(info) if lidar2ego else (info["lidar2ego_rotation"], info["lidar2ego_translation"])
        p = {key: torch.from_numpy(v).to(dev) for key, v in lidar_predictions(info, k).items()}
        out.append(dict(p, boxes=boxes_to_ego(p["boxes"], q, t)))
    return out


@pytest.fixture(scope="module")
def base(infos):
    """-> (metrics of DetectionEval on the info-file route, the restatement's metrics), computed once"""
    from vidar_amd.det_evaluate import DetectionEval, ground_truth_from_infos
    case = ego_case(infos)
    assert_decisions_have_margin(case)
    gt = ground_truth_from_infos(infos, F.CLASS_NAMES, torch.device("cuda", 0))
    assert all(g["boxes"].is_cuda and g["boxes"].dtype == torch.float32 for g in gt)
    return DetectionEval(F.CLASS_NAMES).evaluate(device_predictions(infos), gt), D.evaluate(case)


def test_info_file_ground_truth_scores_like_the_restatement(base):
    got, want = base
    compare_metrics(got, want)
    print("mAP", got["mean_ap"], "NDS", got["nd_score"], got["tp_errors"])
    assert 0.1 < got["mean_ap"] < 0.95                     # a case with matches at every threshold, and misses
    assert got["tp_errors"]["attr_err"] == 1.0             # no attributes in the info files
    assert not math.isnan(got["tp_errors"]["vel_err"])     # NaN ground-truth velocities drop out of the mean, not into it


def test_metrics_do_not_depend_on_the_ego_frame_chosen(infos, base):
    """lidar2ego replaced by Rz(phi) o lidar2ego -- another rigid transform whose translation has the same norm in the
    xy-plane -- and predictions and ground truth moved with it: every ego-frame box turns about the ego origin, so radii,
    centre distances, yaw and velocity differences keep their values up to fp32 rounding and, with the margins asserted for
    the base case, every decision stays."""
    from vidar_amd.det_evaluate import DetectionEval, ground_truth_from_infos
    phi = 0.9
    turn = np.array([math.cos(phi / 2), 0.0, 0.0, math.sin(phi / 2)])

    def turned(info):
        t = np.asarray(info["lidar2ego_translation"], np.float64)
        c, s = math.cos(phi), math.sin(phi)
        return F.qmul(turn, info["lidar2ego_rotation"]), [c * t[0] - s * t[1], s * t[0] + c * t[1], t[2]]
    moved = []
    for info in infos:
        q, t = turned(info)
        assert abs(np.hypot(t[0], t[1]) - np.hypot(*info["lidar2ego_translation"][:2])) < 1e-12
        moved.append(dict(info, lidar2ego_rotation=list(q), lidar2ego_translation=t))
    assert_decisions_have_margin(ego_case(infos, turned))
    gt = ground_truth_from_infos(moved, F.CLASS_NAMES, torch.device("cuda", 0))
    assert not torch.allclose(gt[0]["boxes"][:, :2], ground_truth_from_infos(infos[:1], F.CLASS_NAMES, "cuda")[0]["boxes"][:, :2],
                              atol=0.5)
    got = DetectionEval(F.CLASS_NAMES).evaluate(device_predictions(infos, turned), gt)
    compare_metrics(got, base[0])
    # and scoring LiDAR-frame boxes against ego-frame ground truth is NOT the same thing on this calibration
    mixed = DetectionEval(F.CLASS_NAMES).evaluate(on_device(dict(pred=[lidar_predictions(i, k) for k, i in enumerate(infos)])),
                                                 ground_truth_from_infos(infos, F.CLASS_NAMES, "cuda"))
    assert abs(mixed["mean_ap"] - base[0]["mean_ap"]) > 0.05


def without_velocity(metrics):
    """-> (the metrics with every velocity-derived entry zeroed, those entries)"""
    m = copy.deepcopy(metrics)
    vel = dict(cls={n: m["label_tp_errors"][n]["vel_err"] for n in F.CLASS_NAMES}, mean=m["tp_errors"]["vel_err"],
               score=m["tp_scores"]["vel_err"], nds=m["nd_score"])
    for n in F.CLASS_NAMES:
        m["label_tp_errors"][n]["vel_err"] = 0.0
        m["detail"][f"pts_bbox_NuScenes/{n}_vel_err"] = 0.0
    m["tp_errors"]["vel_err"] = m["tp_scores"]["vel_err"] = m["nd_score"] = 0.0
    m["detail"]["pts_bbox_NuScenes/mAVE"] = m["detail"]["pts_bbox_NuScenes/NDS"] = 0.0
    return m, vel


def launcher():
    spec = importlib.util.spec_from_file_location("vidar_tools_test", ROOT / "tools" / "test.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def run_launcher(ann, folder, *flags):
    """tools/test.py main on the fixture -> (its module, --out path, --results-json path, what it printed)"""
    tool = launcher()
    out, sub = folder / "det.json", folder / "sub" / "results_nusc.json"
    printed = io.StringIO()
    with contextlib.redirect_stdout(printed):
        tool.main(["finetune/vidar_1_8_nusc_1future", "--bev", "24", "24", "--cams", "2", "--ann-file", str(ann),
                   "--samples", "0", "--results-json", str(sub), "--out", str(out), *flags])
    return tool, out, sub, printed.getvalue()


@pytest.fixture(scope="module")
def host_run(ann, tmp_path_factory):
    """the run on the host image path, once for the tests below"""
    return run_launcher(ann, tmp_path_factory.mktemp("host_run"))


def test_test_launcher_scores_the_info_file_and_writes_the_submission(infos, host_run):
    from vidar_amd.det_evaluate import DetectionEval, ground_truth_from_infos, read_results_json
    tool, out, sub, printed = host_run
    doc = json.loads(out.read_text())
    assert set(doc) == {"frames", "metrics"}
    assert [f["sample"] for f in doc["frames"]] == [i["token"] for i in infos]                   # every frame, dataset order
    assert [f["scene"] for f in doc["frames"]] == [i["scene_token"] for i in infos] and all(f["boxes"] > 0 for f in doc["frames"])
    got = doc["metrics"]
    got["label_aps"] = {n: {float(k): v for k, v in d.items()} for n, d in got["label_aps"].items()}   # JSON keys are strings
    tokens, pred = read_results_json(sub, infos, F.CLASS_NAMES, device="cuda")
    assert tokens == [i["token"] for i in infos] and sum(len(p["labels"]) for p in pred) > 0
    again = DetectionEval(F.CLASS_NAMES).evaluate([{k: p[k] for k in ("boxes", "scores", "labels")} for p in pred],
                                                  ground_truth_from_infos(infos, F.CLASS_NAMES, "cuda"))
    # Everything but the velocity agrees to the restatement's tolerance.  The velocity is the one field the submission layout
    # truncates: it holds two components of the GLOBAL-frame velocity, and with the fixture's tilted ego2global the dropped
    # vertical component v_z does not come back.  Read back, a box's ego-frame velocity is off by at most |R[2, :2]| |v_z|
    # with R = ego2global; |v_z| <= |R[2, :2]| |v_xy| + |v_ego_z| and |v_ego_z| <= a |v| with a = |lidar2ego[2, :2]|,
    # |v| <= |v_xy| / sqrt(1 - a^2).  Every vel_err is an average of per-pair errors, so it moves by at most the largest
    # such bound over the boxes of the file, and NDS by a tenth of what mAVE moves.
    a = np.linalg.norm(F.rot(F.LIDAR2EGO["rotation"])[2, :2])
    slack = 0.0
    for info, p in zip(infos, pred):
        e = np.linalg.norm(F.rot(info["ego2global_rotation"])[2, :2])
        speed = float(p["boxes"][:, 7:].double().norm(dim=1).max()) if len(p["labels"]) else 0.0
        slack = max(slack, 1.01 * e * (e + a / math.sqrt(1 - a * a)) * speed)
    print("velocity slack of the layout", slack, "mAVE", got["tp_errors"]["vel_err"])
    assert slack < 0.05 * got["tp_errors"]["vel_err"]      # the allowance stays small next to what it is an allowance on
    (got_rest, got_vel), (again_rest, again_vel) = without_velocity(got), without_velocity(again)
    compare_metrics(got_rest, again_rest)
    for n in F.CLASS_NAMES:
        x, y = got_vel["cls"][n], again_vel["cls"][n]
        assert math.isnan(x) == math.isnan(y) and (math.isnan(x) or abs(x - y) <= 1e-5 + slack), (n, x, y)
    assert abs(got_vel["mean"] - again_vel["mean"]) <= 1e-5 + slack and abs(got_vel["score"] - again_vel["score"]) <= 1e-5 + slack
    assert abs(got_vel["nds"] - again_vel["nds"]) <= 1e-5 + slack / 10
    assert "Per-class results:" in printed and "NDS: %.4f" % got["nd_score"] in printed and "mAAE is 1" in printed
    assert f"results: {sub}" in printed
    # --eval-stride keeps whole scenes
    assert tool.whole_scene_subset(infos, 2) == list(range(6)) and tool.whole_scene_subset(infos, None) == list(range(F.N_FRAMES))


def test_test_mode_item_is_one_tensor_on_both_image_paths(ann):
    """a test-mode item has no time axis: the device image path must still give the host path's tensor"""
    from vidar_amd.configs import dataset_kwargs, get_config
    from vidar_amd.data import DetectionSequenceDataset
    from vidar_amd.data.loader import collate, finish_batch
    kw = dataset_kwargs(get_config("finetune/vidar_1_8_nusc_1future"), test_mode=True)
    host = DetectionSequenceDataset(ann, **kw)[7]
    item = DetectionSequenceDataset(ann, device_images=True, **kw)[7]
    assert item["img_raw"].shape == (2, 40, 64, 3) and item["img_raw"].dtype == torch.uint8 and "img" not in item
    img = finish_batch(collate([item]), torch.device("cuda", 0))["img"]
    assert img.shape == (1, 2, 3, 64, 64) and torch.equal(img[0].cpu(), host["img"])
    assert item["img_metas"]["img_shape"] == host["img_metas"]["img_shape"]


def test_test_launcher_with_device_images_gives_the_same_document(ann, host_run, tmp_path):
    """--device-images on the info-file route: the same tensor goes into the model, so the frames, the metrics and the
    submission file are those of the host image path, bit for bit"""
    _, host_out, host_sub, _ = host_run
    _, out, sub, printed = run_launcher(ann, tmp_path, "--device-images")
    assert "NDS: " in printed
    doc, host = json.loads(out.read_text()), json.loads(host_out.read_text())
    assert doc["frames"] == host["frames"] and len(doc["frames"]) == F.N_FRAMES
    floats = lambda m: dict(m, label_aps={n: {float(k): v for k, v in d.items()} for n, d in m["label_aps"].items()})
    compare_metrics(floats(doc["metrics"]), floats(host["metrics"]), ap_tol=0.0, tp_tol=0.0)
    assert json.loads(sub.read_text()) == json.loads(host_sub.read_text())
