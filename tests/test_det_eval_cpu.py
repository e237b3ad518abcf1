"""CPU: the detection metric's yardstick on a hand-worked case, the case generator's grid property, the pair-error header
(csrc/det_eval_math.h) through a stand-alone host program, and the no-GPU behaviour of the evaluator and its entry point."""
import math
import os
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import det_eval_cases as D

ROOT = Path(__file__).resolve().parents[1]


def test_yardstick_on_a_hand_worked_case():
    """One car annotation, one car prediction 0.25 m away, score 0.9.
    accumulate(car, any threshold >= 0.5): the prediction matches (0.25 < th) -> tp = [1], fp = [0], npos = 1, so
    prec = [1], rec = [1].  np.interp onto the 101 recall points: every point below rec[0] = 1 takes the left edge
    prec[0] = 1, the point 1.0 itself is prec[0] -> precision == 1 everywhere, confidence == 0.9 everywhere.
    calc_ap: mean(max(1 - 0.1, 0) over points 11..100) / (1 - 0.1) = 0.9 / 0.9 = 1 at all four thresholds.
    The nine other classes have no ground truth -> no_predictions() -> AP 0: mAP = (1 + 9 * 0) / 10 = 0.1.
    calc_tp(car, trans_err): cummean([0.25]) = [0.25], interpolated over confidence -> 0.25 at every point,
    max_recall_ind = 100 >= 11 -> mean = 0.25.  Every other class gives 1.0 (max_recall_ind = 0 < 11), trans_err is never
    NaN by definition: mATE = (0.25 + 9 * 1) / 10 = 0.925."""
    r = D.evaluate(D.hand_case())
    assert [r["label_aps"]["car"][th] for th in D.DIST_THS] == pytest.approx([1.0] * 4, abs=1e-12)
    assert r["mean_ap"] == pytest.approx(0.1, abs=1e-12)
    assert r["label_tp_errors"]["car"]["trans_err"] == pytest.approx(0.25, abs=1e-12)
    assert r["tp_errors"]["trans_err"] == pytest.approx(0.925, abs=1e-12)
    # no attribute ground truth: attr_err of every match is NaN -> cummean gives ones -> 1
    assert r["label_tp_errors"]["car"]["attr_err"] == 1.0
    assert math.isnan(r["label_tp_errors"]["traffic_cone"]["orient_err"])
    assert math.isnan(r["label_tp_errors"]["barrier"]["vel_err"])
    assert not math.isnan(r["label_tp_errors"]["barrier"]["orient_err"])
    assert r["nd_score"] == pytest.approx((5 * r["mean_ap"] + sum(max(1 - v, 0) for v in r["tp_errors"].values())) / 10)
    assert len(r["detail"]) == 10 * 9 + 5 + 2
    assert r["detail"]["pts_bbox_NuScenes/car_AP_dist_0.5"] == 1.0
    assert r["detail"]["pts_bbox_NuScenes/mATE"] == 0.925


def test_yardstick_special_cases():
    by_name = {c["name"]: c for c in D.cases()}
    th = {t: i for i, t in enumerate(D.DIST_THS)}
    # a pair at exactly the threshold does not match there, and does at the next one
    match, _, _, P, G = D.match_lists(by_name["exact_thresholds"])
    for i, t in enumerate(D.DIST_THS):
        assert match[i][i] == -1 and all(match[j][i] == i for j in range(i + 1, 4))
    # equidistant: the lower row wins (rows 1 and 2 of the first sample)
    match, _, _, _, _ = D.match_lists(by_name["equidistant"])
    assert match[th[2.0]][0] == 1 and match[th[4.0]][2] == 3
    # equal scores: the later index (row 1, 0.75 m) goes first and takes the annotation; row 0 (0.25 m) is left out
    match, _, _, _, _ = D.match_lists(by_name["equal_scores"])
    assert match[th[1.0]][1] == 0 and match[th[1.0]][0] == -1 and match[th[0.5]][0] == 0
    # nearest taken, next one at 2.5 m: false positive at 2 m although the taken one is 0.5 m away
    match, _, _, _, _ = D.match_lists(by_name["nearest_taken"])
    assert match[th[2.0]][1] == -1 and match[th[4.0]][1] == 1


def test_generator_keeps_the_grid_property():
    cs = D.cases()
    assert len(cs) >= 15 and all(D.check_grid(c) for c in cs)
    assert max(len(p["labels"]) for c in cs for p in c["pred"]) == 500
    bad = D.hand_case()
    bad["pred"][0]["boxes"][0, 0] += 1.0 / 128
    with pytest.raises(AssertionError):
        D.check_grid(bad)


def _matched_pairs():
    """(gt, pred, class name) of every pair any case matches at 2 m or 4 m, plus attribute variations"""
    pairs = []
    for case in D.cases():
        gts, preds = D.flatten(case)
        for name in D.CLASS_NAMES:
            for th in (2.0, 4.0):
                for pk, gk, _ in D.accumulate(gts, preds, name, th)[1]:
                    if gk >= 0:
                        pairs.append((gts[gk], preds[pk], name))
    assert len(pairs) > 200
    return pairs


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("det_eval_host") / "det_eval_host"
    base = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", f"-I{ROOT / 'vidar_amd' / 'csrc'}",
            str(ROOT / "tests" / "det_eval_host.cpp"), "-o", str(exe)]
    # a stand-alone program with its own main: the host sanitizers apply when the toolchain ships their runtimes
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.run(base, check=True)
    return exe


def test_pair_error_header_against_the_yardstick(host_program, tmp_path):
    pairs = _matched_pairs()
    blob = struct.pack("<i", len(pairs))
    for gt, pr, name in pairs:
        blob += np.asarray(gt["box"], np.float32).tobytes() + np.asarray(pr["box"], np.float32).tobytes()
        blob += struct.pack("<3i", gt["attr"], pr["attr"], int(name == "barrier"))
    (tmp_path / "in.bin").write_bytes(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(host_program), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True,
                         text=True, env=env)
    assert run.returncode == 0, run.stderr[-2000:]
    got = np.fromfile(tmp_path / "out.bin", dtype=np.float32).reshape(len(pairs), 5).astype(np.float64)
    want = np.asarray([D.pair_errors(gt, pr, name) for gt, pr, name in pairs], np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.isnan(want[:, 1]).any() and np.isnan(want[:, 4]).any() and not np.isnan(want[:, 4]).all()
    diff = np.nan_to_num(np.abs(got - want), nan=0.0)
    print("largest difference per error:", diff.max(0))
    assert diff.max() <= 1e-5
    # the barrier period halves what a car would be charged
    b = [i for i, p in enumerate(pairs) if p[2] == "barrier"]
    assert b and want[b, 3].max() <= math.pi / 2 + 1e-12 and want[:, 3].max() > math.pi / 2


def test_evaluator_refuses_cpu_tensors():
    from vidar_amd.det_evaluate import DetectionEval
    case = D.hand_case()
    pred = [{k: torch.from_numpy(v) for k, v in s.items()} for s in case["pred"]]
    gt = [{k: torch.from_numpy(v) for k, v in s.items()} for s in case["gt"]]
    with pytest.raises(RuntimeError):
        DetectionEval().evaluate(pred, gt)


def test_default_attributes_follow_the_speed_rule():
    """host-side table check of the heuristic against the yardstick's restatement (CPU tensors are fine here: it is
    plumbing, no kernel behind it)"""
    from vidar_amd.det_evaluate import default_attributes
    labels = torch.arange(10).repeat(2)
    boxes = torch.zeros(20, 9)
    boxes[10:, 7] = 0.3
    got = default_attributes(labels, boxes, D.CLASS_NAMES).tolist()
    want = [D.default_attribute(D.CLASS_NAMES[int(l)], [float(v) for v in b]) for l, b in zip(labels, boxes)]
    assert got == want
    assert D.ATTRIBUTES[got[D.CLASS_NAMES.index("pedestrian")]] == "pedestrian.standing"
    assert D.ATTRIBUTES[got[10 + D.CLASS_NAMES.index("bicycle")]] == "cycle.with_rider"


def test_entry_point_argument_checks_without_a_gpu():
    """empty extents return 0 and bad ones VIDAR_ERR_BAD_ARG before any HIP call: both answers come back on a machine
    without a GPU"""
    from vidar_amd._lib import BAD_ARG, lib
    import ctypes
    f = lib().vidar_det_eval_match_f32
    ths = (ctypes.c_float * 4)(0.5, 1.0, 2.0, 4.0)
    fake = 4096                                                   # a non-NULL address that is never dereferenced
    # (pred_box, pred_attr, pred_start, gt_box, gt_attr, gt_start, dist_ths, match, gt_match, err, P, G, NS, NT, tp, C, barrier)
    assert f(None, None, None, None, None, None, None, None, None, None, 0, 0, 0, 4, 2, 10, 5, None) == 0      # no segments
    assert f(None, None, fake, None, None, fake, ths, None, None, None, 0, 0, 30, 4, 2, 10, 5, None) == 0      # no boxes
    assert f(None, None, fake, None, None, fake, ths, None, None, None, 0, 0, 30, 0, -1, 10, 5, None) == 0     # no thresholds
    for P, G, NS, NT, tp, C in ((-1, 0, 1, 4, 2, 10), (0, -1, 1, 4, 2, 10), (0, 0, -1, 4, 2, 10), (0, 0, 1, -1, 2, 10),
                                (0, 0, 1, 9, 2, 10), (0, 0, 1, 4, 4, 10), (0, 0, 1, 4, -2, 10), (0, 0, 1, 4, 2, 0)):
        assert f(None, None, fake, None, None, fake, ths, None, None, None, P, G, NS, NT, tp, C, 5, None) == BAD_ARG
    # missing pointers with something to do
    assert f(None, None, fake, fake, None, fake, ths, fake, fake, fake, 3, 2, 1, 4, 2, 10, 5, None) == BAD_ARG   # pred_box
    assert f(fake, None, fake, fake, None, fake, None, fake, fake, fake, 3, 2, 1, 4, 2, 10, 5, None) == BAD_ARG  # dist_ths
    assert f(fake, None, fake, fake, None, fake, ths, fake, fake, None, 3, 2, 1, 4, 2, 10, 5, None) == BAD_ARG   # err
    assert f(fake, None, None, fake, None, fake, ths, fake, fake, fake, 3, 2, 1, 4, 2, 10, 5, None) == BAD_ARG   # pred_start
