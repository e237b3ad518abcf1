"""GPU: the detection-metric matcher (csrc/det_eval.hip through its C entry point), DetectionEval.evaluate and the
tools/test.py wiring against the fp64 restatement of the devkit in tests/det_eval_cases.py -- a RECALLED restatement, not
the devkit.  The cases live on a 1/64 m grid, so the fp32 kernel and the fp64 loops take identical decisions."""
import ctypes
import functools
import importlib.util
import json
import math
from pathlib import Path

import numpy as np
import pytest
import torch

import det_eval_cases as D

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
CASES = {c["name"]: c for c in D.cases()}
C, NT, TP = len(D.CLASS_NAMES), len(D.DIST_THS), D.DIST_THS.index(D.DIST_TH_TP)


@functools.lru_cache(maxsize=None)
def want_matches(name):
    return D.match_lists(CASES[name])


@functools.lru_cache(maxsize=None)
def want_metrics(name):
    return D.evaluate(CASES[name])


def on_device(case, order=None, pred_perm=None):
    """the case as DetectionEval takes it; `order`: a permutation of the samples, `pred_perm`: seed of a permutation of
    the predictions inside every sample"""
    dev = torch.device("cuda", 0)
    idx = list(range(len(case["pred"]))) if order is None else list(order)
    pred, gt = [], []
    for i in idx:
        p = {k: torch.from_numpy(v).to(dev) for k, v in case["pred"][i].items()}
        if pred_perm is not None:
            perm = torch.from_numpy(np.random.default_rng(pred_perm + i).permutation(len(p["labels"]))).to(dev)
            p = {k: v[perm] for k, v in p.items()}
        pred.append(p)
        gt.append({k: torch.from_numpy(v).to(dev) for k, v in case["gt"][i].items()})
    return pred, gt


def kernel_operands(case):
    """the flat arrays of vidar_det_eval_match_f32, laid out with plain Python from the header's description: grouped by
    segment = sample * C + class, predictions by score descending with the later input row first on equal scores, ground
    truth in input order"""
    gts, preds = D.flatten(case)
    seg = lambda b: b["sample"] * C + D.CLASS_NAMES.index(b["name"])
    po = sorted(range(len(preds)), key=lambda k: (seg(preds[k]), -preds[k]["score"], -k))
    go = sorted(range(len(gts)), key=lambda k: (seg(gts[k]), k))
    NS = len(case["pred"]) * C

    def starts(boxes, order):
        s = np.zeros(NS + 1, np.int32)
        for k in order:
            s[seg(boxes[k]) + 1] += 1
        return np.cumsum(s).astype(np.int32)
    arr = lambda rows, dt, width: np.asarray(rows, dt).reshape(len(rows), *width)
    return dict(po=po, go=go, NS=NS,
                pred_box=arr([preds[k]["box"] for k in po], np.float32, (9,)), pred_attr=arr([preds[k]["attr"] for k in po], np.int32, ()),
                pred_start=starts(preds, po), gt_box=arr([gts[k]["box"] for k in go], np.float32, (9,)),
                gt_attr=arr([gts[k]["attr"] for k in go], np.int32, ()), gt_start=starts(gts, go))


@pytest.mark.parametrize("name", list(CASES))
def test_matcher_equals_the_restatement(name):
    from vidar_amd._lib import lib, ptr
    dev = torch.device("cuda", 0)
    k = kernel_operands(CASES[name])
    want_match, want_err, want_gt_match, P, G = want_matches(name)
    t = {n: torch.from_numpy(k[n]).to(dev) for n in ("pred_box", "pred_attr", "pred_start", "gt_box", "gt_attr", "gt_start")}
    match = torch.full((NT, P), -7, dtype=torch.int32, device=dev)
    gt_match = torch.full((NT, G), -7, dtype=torch.int32, device=dev)
    err = torch.full((P, 5), -7.0, dtype=torch.float32, device=dev)
    ths = (ctypes.c_float * NT)(*D.DIST_THS)
    rc = lib().vidar_det_eval_match_f32(ptr(t["pred_box"]), ptr(t["pred_attr"]), ptr(t["pred_start"]), ptr(t["gt_box"]),
                                        ptr(t["gt_attr"]), ptr(t["gt_start"]), ths, ptr(match), ptr(gt_match), ptr(err), P, G,
                                        k["NS"], NT, TP, C, D.CLASS_NAMES.index("barrier"),
                                        torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    match, gt_match, err = match.cpu().numpy(), gt_match.cpu().numpy(), err.cpu().numpy().astype(np.float64)
    po, go = k["po"], k["go"]
    # kernel rows -> the restatement's numbering on both sides
    got_match = np.full((NT, P), -9)
    got_gt_match = np.full((NT, G), -9)
    for th in range(NT):
        for row, pk in enumerate(po):
            got_match[th, pk] = go[match[th, row]] if match[th, row] >= 0 else match[th, row]
        for row, gk in enumerate(go):
            got_gt_match[th, gk] = po[gt_match[th, row]] if gt_match[th, row] >= 0 else gt_match[th, row]
    assert np.array_equal(got_match, np.asarray(want_match).reshape(NT, P))
    assert np.array_equal(got_gt_match, np.asarray(want_gt_match).reshape(NT, G))
    want = np.full((P, 5), np.nan)
    for pk, e in enumerate(want_err):
        if e is not None:
            want[pk] = e
    got = np.empty((P, 5))
    got[po] = err
    assert np.array_equal(np.isnan(got), np.isnan(want))
    diff = np.nan_to_num(np.abs(got - want), nan=0.0)
    print(name, "P", P, "G", G, "matches at 2 m", int((np.asarray(want_match[TP]) >= 0).sum()) if P else 0,
          "largest err difference", diff.max() if P else 0.0)
    assert not P or diff.max() <= 1e-5


def compare_metrics(got, want, ap_tol=1e-9, tp_tol=1e-5):
    def same(a, b, tol):
        assert math.isnan(a) == math.isnan(b), (a, b)
        assert math.isnan(a) or abs(a - b) <= tol, (a, b)
    for n in D.CLASS_NAMES:
        for th in D.DIST_THS:
            same(got["label_aps"][n][th], want["label_aps"][n][th], ap_tol)
        same(got["mean_dist_aps"][n], want["mean_dist_aps"][n], ap_tol)
        for e in D.TP_METRICS:
            same(got["label_tp_errors"][n][e], want["label_tp_errors"][n][e], tp_tol)
    same(got["mean_ap"], want["mean_ap"], ap_tol)
    for e in D.TP_METRICS:
        same(got["tp_errors"][e], want["tp_errors"][e], tp_tol)
        same(got["tp_scores"][e], want["tp_scores"][e], tp_tol)
    same(got["nd_score"], want["nd_score"], tp_tol)
    assert set(got["detail"]) == set(want["detail"])
    for k, v in want["detail"].items():
        same(got["detail"][k], v, 1.01e-4)                       # both sides are rounded to four decimals


@pytest.mark.parametrize("name", list(CASES) + ["hand"])
def test_evaluate_equals_the_restatement(name):
    from vidar_amd.det_evaluate import DetectionEval, format_summary
    case = D.hand_case() if name == "hand" else CASES[name]
    want = D.evaluate(case) if name == "hand" else want_metrics(name)
    got = DetectionEval(D.CLASS_NAMES).evaluate(*on_device(case))
    assert list(got) == ["label_aps", "label_tp_errors", "mean_dist_aps", "mean_ap", "tp_errors", "tp_scores", "nd_score",
                         "detail"]
    compare_metrics(got, want)
    assert len(got["detail"]) == 97
    table = format_summary(got)
    assert table.splitlines()[0] == "mAP: %.4f" % want["mean_ap"] and "NDS: %.4f" % want["nd_score"] in table


def test_more_than_500_predictions_in_a_sample_raise():
    from vidar_amd.det_evaluate import DetectionEval
    pred, gt = on_device(CASES["500_predictions"])
    pred[0] = {k: torch.cat([v, v[:1]]) for k, v in pred[0].items()}
    with pytest.raises(ValueError, match="500"):
        DetectionEval(D.CLASS_NAMES).evaluate(pred, gt)


@pytest.mark.parametrize("name", ["mixed_3x10", "exact_thresholds", "pred_only_gt_only", "equidistant"])
def test_sample_order_does_not_matter(name):
    from vidar_amd.det_evaluate import DetectionEval
    case = CASES[name]
    n = len(case["pred"])
    order = list(np.random.default_rng(5).permutation(n))
    if order == list(range(n)):
        order = order[::-1]
    got = DetectionEval(D.CLASS_NAMES).evaluate(*on_device(case, order=order))
    compare_metrics(got, want_metrics(name))
    base = DetectionEval(D.CLASS_NAMES).evaluate(*on_device(case))
    compare_metrics(got, base, ap_tol=1e-12, tp_tol=1e-12)       # same matches, same fp64 passes: the same numbers


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if not c["score_ties"]])
def test_prediction_order_does_not_matter(name):
    from vidar_amd.det_evaluate import DetectionEval
    got = DetectionEval(D.CLASS_NAMES).evaluate(*on_device(CASES[name], pred_perm=11))
    compare_metrics(got, want_metrics(name))
    base = DetectionEval(D.CLASS_NAMES).evaluate(*on_device(CASES[name]))
    compare_metrics(got, base, ap_tol=1e-12, tp_tol=1e-12)


def test_tools_test_reports_the_metrics(tmp_path, monkeypatch, capsys):
    """tools/test.py on a detection recipe: "metrics" sits next to the per-frame records, holds every key, and equals the
    restatement run on the very boxes the call decoded (captured at the evaluator's door)."""
    from vidar_amd import det_evaluate
    seen = {}
    real = det_evaluate.DetectionEval.evaluate

    def spy(self, pred, gt):
        seen["pred"], seen["gt"] = pred, gt
        return real(self, pred, gt)
    monkeypatch.setattr(det_evaluate.DetectionEval, "evaluate", spy)
    spec = importlib.util.spec_from_file_location("vidar_tools_test", ROOT / "tools" / "test.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out = tmp_path / "det.json"
    tool.main(["finetune/vidar_1_8_nusc_1future", "--no-backbone", "--bev", "50", "50", "--samples", "2", "--out", str(out)])
    printed = capsys.readouterr().out
    doc = json.loads(out.read_text())
    assert set(doc) == {"frames", "metrics"} and len(doc["frames"]) > 0 and "boxes" in doc["frames"][0]
    got = doc["metrics"]
    assert list(got) == ["label_aps", "label_tp_errors", "mean_dist_aps", "mean_ap", "tp_errors", "tp_scores", "nd_score",
                         "detail"]
    got["label_aps"] = {n: {float(k): v for k, v in d.items()} for n, d in got["label_aps"].items()}   # JSON keys are strings
    assert len(seen["pred"]) == 2 and all(p["boxes"].is_cuda for p in seen["pred"])
    case = dict(pred=[{k: v.cpu().numpy() for k, v in p.items()} for p in seen["pred"]],
                gt=[{k: v.cpu().numpy() for k, v in g.items()} for g in seen["gt"]])
    assert all(np.array_equal(g["num_pts"], np.ones_like(g["num_pts"])) and "attrs" not in g for g in case["gt"])
    want = D.evaluate(case)
    compare_metrics(got, want)
    assert "Per-class results:" in printed and "NDS: %.4f" % want["nd_score"] in printed
    # no ground-truth attributes: every match's attr_err is NaN -> 1 wherever it is defined
    assert all(got["label_tp_errors"][n]["attr_err"] == 1.0 for n in D.CLASS_NAMES if n not in ("barrier", "traffic_cone"))
    # an untrained detector: its boxes are noise, precision stays under the 0.1 floor that calc_ap subtracts
    print("untrained: mAP", got["mean_ap"], "NDS", got["nd_score"])
    assert got["mean_ap"] <= 0.05 and got["nd_score"] <= 0.25
