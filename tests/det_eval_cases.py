"""TEST INFRASTRUCTURE: the yardstick of the detection metric (tests/test_det_eval_{cpu,gpu}.py) and its case generator.

A plain-Python, fp64, loop-for-loop restatement of the nuScenes devkit's detection evaluation -- `accumulate`, `calc_ap`,
`calc_tp`, `DetectionMetrics` and the five true-positive error functions -- RECALLED from the devkit
(python-sdk/nuscenes/eval/detection/{algo,data_classes,evaluate}.py, eval/common/utils.py), NOT compiled from it and not
checked against it: the devkit is neither part of the reference tree nor installable here.  Parity with this file is
parity with a restatement.  It shares no code with vidar_amd (the class list, the attribute list and the
detection_cvpr_2019 constants are restated below on purpose) and is never used by the product.

Boxes are [N, 9] rows (x, y, z, three sizes, yaw, vx, vy) in the ego-centred frame of their sample; attribute ids index
ATTRIBUTES, -1 = none (the devkit's '').

Case generator: every x, y is a multiple of 1/64 m with |x|, |y| <= 64, so coordinates are exact in fp32 and dx*dx + dy*dy
is exact in fp32 for every pair closer than 64 m; farther pairs round monotonically and stay above every threshold.  The
fp32 matcher and this fp64 restatement therefore take identical decisions, ties and exact-threshold distances included.
`check_grid` asserts the property for every generated case."""
import math

import numpy as np

CLASS_NAMES = ("car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian",
               "traffic_cone")
ATTRIBUTES = ("cycle.with_rider", "cycle.without_rider", "pedestrian.moving", "pedestrian.standing",
              "pedestrian.sitting_lying_down", "vehicle.moving", "vehicle.parked", "vehicle.stopped")
CLASS_RANGE = {"car": 50, "truck": 50, "bus": 50, "trailer": 50, "construction_vehicle": 50, "pedestrian": 40,
               "motorcycle": 40, "bicycle": 40, "traffic_cone": 30, "barrier": 30}
DIST_THS = (0.5, 1.0, 2.0, 4.0)
DIST_TH_TP = 2.0
MIN_RECALL = 0.1
MIN_PRECISION = 0.1
MEAN_AP_WEIGHT = 5
MAX_BOXES_PER_SAMPLE = 500
TP_METRICS = ("trans_err", "scale_err", "orient_err", "vel_err", "attr_err")          # the devkit's order
ERR_COLUMNS = ("trans_err", "vel_err", "scale_err", "orient_err", "attr_err")         # column order of the kernel's err[P, 5]
ERR_NAME_MAPPING = {"trans_err": "mATE", "scale_err": "mASE", "orient_err": "mAOE", "vel_err": "mAVE", "attr_err": "mAAE"}
GRID = 64


# ------------------------------------------------------------------------------------------------------------------
# eval/common/utils.py
# ------------------------------------------------------------------------------------------------------------------
def center_distance(gt, pr):
    return math.sqrt((pr["box"][0] - gt["box"][0]) ** 2 + (pr["box"][1] - gt["box"][1]) ** 2)


def velocity_l2(gt, pr):
    return math.sqrt((pr["box"][7] - gt["box"][7]) ** 2 + (pr["box"][8] - gt["box"][8]) ** 2)


def scale_iou(gt, pr):
    sa, sr = gt["box"][3:6], pr["box"][3:6]
    va, vr = sa[0] * sa[1] * sa[2], sr[0] * sr[1] * sr[2]
    inter = min(sa[0], sr[0]) * min(sa[1], sr[1]) * min(sa[2], sr[2])
    return inter / (va + vr - inter)


def angle_diff(x, y, period):
    diff = (x - y + period / 2) % period - period / 2
    if diff > math.pi:
        diff = diff - 2 * math.pi
    return diff


def yaw_diff(gt, pr, period):
    return abs(angle_diff(gt["box"][6], pr["box"][6], period))


def attr_acc(gt, pr):
    if gt["attr"] < 0:
        return float("nan")
    return float(gt["attr"] == pr["attr"])


def pair_errors(gt, pr, class_name):
    """the five errors of a matched pair in ERR_COLUMNS order"""
    period = math.pi if class_name == "barrier" else 2 * math.pi
    return [center_distance(gt, pr), velocity_l2(gt, pr), 1 - scale_iou(gt, pr), yaw_diff(gt, pr, period),
            1 - attr_acc(gt, pr)]


def cummean(x):
    x = np.asarray(x, dtype=float)
    if sum(np.isnan(x)) == len(x):
        return np.ones(len(x))
    sum_vals = np.nancumsum(x)
    count_vals = np.cumsum(~np.isnan(x))
    return np.divide(sum_vals, count_vals, out=np.zeros_like(sum_vals), where=count_vals != 0)


# ------------------------------------------------------------------------------------------------------------------
# loading + filtering (eval/common/loaders.py: add_center_dist, filter_eval_boxes without the bike-rack step)
# ------------------------------------------------------------------------------------------------------------------
def flatten(case):
    """case -> (gts, preds): lists of dict(sample, name, box [9 floats], score, attr, num_pts) in input order, filtered by
    class range (hypot(x, y) < class_range) and, for the ground truth, num_pts > 0; `k` numbers the survivors"""
    gts, preds = [], []
    for s, (p, g) in enumerate(zip(case["pred"], case["gt"])):
        n = len(p["labels"])
        assert n <= MAX_BOXES_PER_SAMPLE, "Error: Only <= %d boxes per sample allowed!" % MAX_BOXES_PER_SAMPLE
        for i in range(n):
            box = [float(v) for v in p["boxes"][i]]
            name = CLASS_NAMES[int(p["labels"][i])]
            if math.sqrt(box[0] ** 2 + box[1] ** 2) < CLASS_RANGE[name]:
                preds.append(dict(sample=s, name=name, box=box, score=float(p["scores"][i]),
                                  attr=int(p["attrs"][i]) if p.get("attrs") is not None else None, k=len(preds)))
        for i in range(len(g["labels"])):
            box = [float(v) for v in g["boxes"][i]]
            name = CLASS_NAMES[int(g["labels"][i])]
            if math.sqrt(box[0] ** 2 + box[1] ** 2) < CLASS_RANGE[name] and int(g["num_pts"][i]) > 0:
                gts.append(dict(sample=s, name=name, box=box,
                                attr=int(g["attrs"][i]) if g.get("attrs") is not None else -1, k=len(gts)))
    for p in preds:
        if p["attr"] is None:
            p["attr"] = default_attribute(p["name"], p["box"])
    return gts, preds


DEFAULT_ATTRIBUTE = {"car": "vehicle.parked", "pedestrian": "pedestrian.moving", "trailer": "vehicle.parked",
                     "truck": "vehicle.parked", "bus": "vehicle.moving", "motorcycle": "cycle.without_rider",
                     "construction_vehicle": "vehicle.parked", "bicycle": "cycle.without_rider", "barrier": "",
                     "traffic_cone": ""}


def default_attribute(name, box):
    """the speed heuristic of mmdet3d's NuScenesDataset._format_bbox -> attribute id (-1 = '')"""
    if math.sqrt(box[7] ** 2 + box[8] ** 2) > 0.2:
        if name in ("car", "construction_vehicle", "bus", "truck", "trailer"):
            attr = "vehicle.moving"
        elif name in ("bicycle", "motorcycle"):
            attr = "cycle.with_rider"
        else:
            attr = DEFAULT_ATTRIBUTE[name]
    else:
        if name == "pedestrian":
            attr = "pedestrian.standing"
        elif name == "bus":
            attr = "vehicle.stopped"
        else:
            attr = DEFAULT_ATTRIBUTE[name]
    return ATTRIBUTES.index(attr) if attr else -1


# ------------------------------------------------------------------------------------------------------------------
# eval/detection/algo.py
# ------------------------------------------------------------------------------------------------------------------
def no_predictions():
    return dict(recall=np.linspace(0, 1, 101), precision=np.zeros(101), confidence=np.zeros(101),
                **{m: np.ones(101) for m in TP_METRICS})


def accumulate(gts, preds, class_name, dist_th):
    """-> (metric data, matches): matches = [(pred k, gt k or -1, the five errors or None)] in processing order"""
    by_sample = {}
    for g in gts:
        by_sample.setdefault(g["sample"], []).append(g)
    npos = len([1 for g in gts if g["name"] == class_name])
    matches = []
    if npos == 0:
        return no_predictions(), [(p["k"], -1, None) for p in preds if p["name"] == class_name]
    pred_boxes_list = [p for p in preds if p["name"] == class_name]
    pred_confs = [p["score"] for p in pred_boxes_list]
    sortind = [i for (v, i) in sorted((v, i) for (i, v) in enumerate(pred_confs))][::-1]
    tp, fp, conf = [], [], []
    match_data = {m: [] for m in ERR_COLUMNS}
    match_data["conf"] = []
    taken = set()
    for ind in sortind:
        pred_box = pred_boxes_list[ind]
        min_dist = np.inf
        match_gt_idx = None
        for gt_idx, gt_box in enumerate(by_sample.get(pred_box["sample"], [])):
            if gt_box["name"] == class_name and not (pred_box["sample"], gt_idx) in taken:
                this_distance = center_distance(gt_box, pred_box)
                if this_distance < min_dist:
                    min_dist = this_distance
                    match_gt_idx = gt_idx
        is_match = min_dist < dist_th
        if is_match:
            taken.add((pred_box["sample"], match_gt_idx))
            tp.append(1)
            fp.append(0)
            conf.append(pred_box["score"])
            gt_box_match = by_sample[pred_box["sample"]][match_gt_idx]
            errs = pair_errors(gt_box_match, pred_box, class_name)
            for m, e in zip(ERR_COLUMNS, errs):
                match_data[m].append(e)
            match_data["conf"].append(pred_box["score"])
            matches.append((pred_box["k"], gt_box_match["k"], errs))
        else:
            tp.append(0)
            fp.append(1)
            conf.append(pred_box["score"])
            matches.append((pred_box["k"], -1, None))
    if len(match_data["trans_err"]) == 0:
        return no_predictions(), matches
    tp = np.cumsum(tp).astype(float)
    fp = np.cumsum(fp).astype(float)
    conf = np.array(conf)
    prec = tp / (fp + tp)
    rec = tp / float(npos)
    rec_interp = np.linspace(0, 1, 101)
    prec = np.interp(rec_interp, rec, prec, right=0)
    conf = np.interp(rec_interp, rec, conf, right=0)
    md = dict(recall=rec_interp, precision=prec, confidence=conf)
    for key in ERR_COLUMNS:
        tmp = cummean(np.array(match_data[key]))
        md[key] = np.interp(conf[::-1], match_data["conf"][::-1], tmp[::-1])[::-1]
    return md, matches


def max_recall_ind(md):
    non_zero = np.nonzero(md["confidence"])[0]
    return 0 if len(non_zero) == 0 else non_zero[-1]


def calc_ap(md, min_recall, min_precision):
    prec = np.copy(md["precision"])
    prec = prec[round(100 * min_recall) + 1:]
    prec -= min_precision
    prec[prec < 0] = 0
    return float(np.mean(prec)) / (1.0 - min_precision)


def calc_tp(md, min_recall, metric_name):
    first_ind = round(100 * min_recall) + 1
    last_ind = max_recall_ind(md)
    if last_ind < first_ind:
        return 1.0
    return float(np.mean(md[metric_name][first_ind: last_ind + 1]))


# ------------------------------------------------------------------------------------------------------------------
# eval/detection/evaluate.py + data_classes.DetectionMetrics + the reference's flat keys (nuscenes_dataset.py:287-302)
# ------------------------------------------------------------------------------------------------------------------
def match_lists(case):
    """-> (match [NT][P] gt k or -1 per surviving prediction k, err [P][5] at the TP threshold (None = unmatched),
    gt_match [NT][G] prediction k or -1, P, G)"""
    gts, preds = flatten(case)
    match = [[-1] * len(preds) for _ in DIST_THS]
    gt_match = [[-1] * len(gts) for _ in DIST_THS]
    err = [None] * len(preds)
    for name in CLASS_NAMES:
        for t, th in enumerate(DIST_THS):
            _, matches = accumulate(gts, preds, name, th)
            for pk, gk, errs in matches:
                match[t][pk] = gk
                if gk >= 0:
                    gt_match[t][gk] = pk
                if th == DIST_TH_TP:
                    err[pk] = errs
    return match, err, gt_match, len(preds), len(gts)


def evaluate(case):
    gts, preds = flatten(case)
    label_aps = {n: {} for n in CLASS_NAMES}
    label_tp_errors = {n: {} for n in CLASS_NAMES}
    for name in CLASS_NAMES:
        mds = {th: accumulate(gts, preds, name, th)[0] for th in DIST_THS}
        for th in DIST_THS:
            label_aps[name][th] = calc_ap(mds[th], MIN_RECALL, MIN_PRECISION)
        for metric in TP_METRICS:
            if name in ["traffic_cone"] and metric in ["attr_err", "vel_err", "orient_err"]:
                tp = np.nan
            elif name in ["barrier"] and metric in ["attr_err", "vel_err"]:
                tp = np.nan
            else:
                tp = calc_tp(mds[DIST_TH_TP], MIN_RECALL, metric)
            label_tp_errors[name][metric] = tp
    mean_dist_aps = {n: float(np.mean(list(d.values()))) for n, d in label_aps.items()}
    mean_ap = float(np.mean(list(mean_dist_aps.values())))
    tp_errors = {m: float(np.nanmean([label_tp_errors[n][m] for n in CLASS_NAMES])) for m in TP_METRICS}
    tp_scores = {m: max(0.0, 1 - tp_errors[m]) for m in TP_METRICS}
    total = float(MEAN_AP_WEIGHT * mean_ap + np.sum(list(tp_scores.values())))
    nd_score = total / float(MEAN_AP_WEIGHT + len(tp_scores))
    out = dict(label_aps=label_aps, label_tp_errors=label_tp_errors, mean_dist_aps=mean_dist_aps, mean_ap=mean_ap,
               tp_errors=tp_errors, tp_scores=tp_scores, nd_score=nd_score)
    detail = {}
    prefix = "pts_bbox_NuScenes"
    for name in CLASS_NAMES:
        for k, v in label_aps[name].items():
            detail["{}/{}_AP_dist_{}".format(prefix, name, k)] = float("{:.4f}".format(v))
        for k, v in label_tp_errors[name].items():
            detail["{}/{}_{}".format(prefix, name, k)] = float("{:.4f}".format(v))
        for k, v in tp_errors.items():
            detail["{}/{}".format(prefix, ERR_NAME_MAPPING[k])] = float("{:.4f}".format(v))
    detail["{}/NDS".format(prefix)] = nd_score
    detail["{}/mAP".format(prefix)] = mean_ap
    out["detail"] = detail
    return out


# ------------------------------------------------------------------------------------------------------------------
# the case generator
# ------------------------------------------------------------------------------------------------------------------
SIZES = ((1.95, 4.6, 1.7), (2.5, 6.9, 2.8), (2.8, 6.4, 3.2), (2.9, 11.0, 3.5), (2.9, 12.3, 3.9), (2.5, 0.5, 1.0),
         (0.8, 2.1, 1.5), (0.6, 1.7, 1.3), (0.7, 0.7, 1.8), (0.4, 0.4, 1.1))
C = {n: i for i, n in enumerate(CLASS_NAMES)}


def _box(rng, label, x, y, yaw=None, vel=None, scale=None):
    size = np.asarray(SIZES[label]) * (rng.uniform(0.8, 1.25, 3) if scale is None else scale)
    yaw = rng.uniform(-math.pi, math.pi) if yaw is None else yaw
    vel = rng.normal(0.0, 1.5, 2) if vel is None else vel
    return [x, y, rng.uniform(-2.0, 0.0), *size, yaw, *vel]


def _sample(rng, preds=(), gts=(), with_attrs=False):
    """preds: (label, x, y, score[, box keywords]); gts: (label, x, y[, num_pts[, box keywords]])"""
    pb = [_box(rng, p[0], p[1], p[2], **(p[4] if len(p) > 4 else {})) for p in preds]
    gb = [_box(rng, g[0], g[1], g[2], **(g[4] if len(g) > 4 else {})) for g in gts]
    pred = dict(boxes=np.asarray(pb, np.float32).reshape(-1, 9), scores=np.asarray([p[3] for p in preds], np.float32),
                labels=np.asarray([p[0] for p in preds], np.int64))
    gt = dict(boxes=np.asarray(gb, np.float32).reshape(-1, 9), labels=np.asarray([g[0] for g in gts], np.int64),
              num_pts=np.asarray([g[3] if len(g) > 3 else 1 + i % 7 for i, g in enumerate(gts)], np.int64))
    if with_attrs:
        pred["attrs"] = rng.integers(-1, len(ATTRIBUTES), len(preds)).astype(np.int32)
        gt["attrs"] = rng.integers(-1, len(ATTRIBUTES), len(gts)).astype(np.int32)
    return pred, gt


def _case(name, samples, score_ties=False):
    return dict(name=name, pred=[s[0] for s in samples], gt=[s[1] for s in samples], score_ties=score_ties)


def _g(rng, lo, hi, size=None):
    """grid coordinates in [lo, hi) metres"""
    return rng.integers(int(lo * GRID), int(hi * GRID), size) / GRID


def _scores(rng, n):
    """n distinct fp32 scores in (0.02, 0.98)"""
    return rng.permutation(np.linspace(0.02, 0.98, n)).astype(np.float32)


def _around(rng, label, gts, n_near, n_far, spread=3.0, area=25.0):
    """predictions of `label`: n_near within `spread` of a random annotation of that label, n_far anywhere"""
    own = [g for g in gts if g[0] == label]
    out = []
    for _ in range(n_near if own else 0):
        g = own[rng.integers(len(own))]
        out.append([label, g[1] + _g(rng, -spread, spread), g[2] + _g(rng, -spread, spread)])
    for _ in range(n_far):
        out.append([label, _g(rng, -area, area), _g(rng, -area, area)])
    return out


def _grid_segment(rng, n, label, cols):
    """n annotations of one class on a 2 m lattice, with predictions that land in the last row, between two rows 16 apart
    (a tie across the 64-lane chunk boundary when n allows: the lower row must win), twice near one row (the second finds
    it taken) and nowhere"""
    gts = [(label, (i % cols) * 2.0, (i // cols) * 2.0) for i in range(n)]
    last = gts[-1]
    preds = [(label, last[1] + 0.25, last[2] + 0.25, 0.9), (label, -20.0, -20.0, 0.5)]
    if n > 2 * cols:
        k = min(50, n - cols - 2)
        if n > 64 + cols:
            k = 64 - cols + 2                                 # rows k (first chunk) and k + cols (second chunk)
        preds.append((label, gts[k][1], gts[k][2] + 1.0, 0.8))
        preds.append((label, gts[k][1] + 0.25, gts[k][2] + 0.75, 0.7))   # row k is taken: goes to k + cols
        preds.append((label, gts[k][1] - 0.25, gts[k][2] + 1.0, 0.6))    # both taken: next ones are 2 m away and more
    else:
        preds.append((label, gts[0][1] - 0.5, gts[0][2], 0.8))
    return _sample(rng, preds, gts)


def cases():
    rng = np.random.default_rng(20191)
    car, truck, bus, barrier, ped, cone, bic = C["car"], C["truck"], C["bus"], C["barrier"], C["pedestrian"], \
        C["traffic_cone"], C["bicycle"]
    out = []
    # a segment with predictions and no ground truth, and the reverse; bicycles are predicted and never annotated
    out.append(_case("pred_only_gt_only", [
        _sample(rng, [(car, 5.0, 5.0, 0.9), (car, 6.0, 5.0, 0.8), (car, 7.0, 5.0, 0.7), (ped, 1.0, 1.25, 0.6),
                      (bic, 3.0, 3.0, 0.5)],
                [(truck, 5.0, 5.5), (truck, 9.0, 9.0), (ped, 1.0, 1.0)]),
        _sample(rng, [(truck, 2.0, 2.0, 0.4)], [(car, 2.0, 2.5)])]))
    # one pair at exactly 0.5 / 1 / 2 / 4 m: no match at that threshold, a match at the next
    out.append(_case("exact_thresholds", [_sample(rng, [(car, 10.0 + th, -7.0, 0.9 - 0.1 * i)], [(car, 10.0, -7.0)])
                                          for i, th in enumerate(DIST_THS)]
                     + [_sample(rng, [(ped, 3.0 + 1.875, 4.0, 0.3)], [(ped, 3.0, 4.0 + 0.6875)])]))     # 1.99707 m: inside
    # equidistant to two annotations: the lower row wins (listed far-near-near so that the order is not the answer)
    out.append(_case("equidistant", [
        _sample(rng, [(car, 0.0, 5.0, 0.9), (car, 0.0, 5.5, 0.8)], [(car, 20.0, 5.0), (car, 1.0, 5.0), (car, -1.0, 5.0)]),
        _sample(rng, [(bus, 4.0, 4.0, 0.9)], [(bus, 4.0, 5.0), (bus, 5.0, 4.0), (bus, 3.0, 4.0), (bus, 4.0, 3.0)])]))
    # two equal scores competing for one annotation: the LATER index goes first (here the farther one, which wins)
    out.append(_case("equal_scores", [
        _sample(rng, [(car, 0.25, 0.0, 0.7), (car, 0.0, 0.75, 0.7), (car, 8.0, 8.0, 0.7), (car, 8.25, 8.0, 0.9)],
                [(car, 0.0, 0.0), (car, 8.0, 8.5)])], score_ties=True))
    # nearest annotation taken, the next one beyond the threshold (2.5 m): false positive up to 2 m, a match at 4 m
    out.append(_case("nearest_taken", [
        _sample(rng, [(car, 0.25, 0.0, 0.9), (car, 0.5, 0.0, 0.8)], [(car, 0.0, 0.0), (car, 3.0, 0.0)])]))
    # greedy but not optimal: the first prediction takes the middle annotation, the others are pushed outwards
    out.append(_case("greedy_chain", [
        _sample(rng, [(ped, 1.0, 0.0, 0.9), (ped, 1.75, 0.0, 0.8), (ped, 3.5, 0.0, 0.7), (ped, 1.5, 0.25, 0.6)],
                [(ped, 0.0, 0.0), (ped, 1.5, 0.0), (ped, 3.0, 0.0)])]))
    # annotation counts across the wave width and across the register / streamed forms of the matcher
    for n in (1, 64, 65, 130):
        out.append(_case(f"segment_{n}_annotations", [_grid_segment(rng, n, ped, 16)]))
    for n in (256, 257, 300):
        out.append(_case(f"segment_{n}_annotations", [_grid_segment(rng, n, car, 20)]))
    # 500 predictions in one segment (the per-sample limit), 40 annotations
    gts = [(car, _g(rng, -30, 30), _g(rng, -30, 30)) for _ in range(40)]
    preds = _around(rng, car, gts, 380, 120, area=30.0)
    out.append(_case("500_predictions", [_sample(rng, [(*p, s) for p, s in zip(preds, _scores(rng, 500))], gts,
                                                 with_attrs=True)]))
    # 3 samples x 10 classes, attributes on both sides, some NaN ground-truth velocities, some num_pts == 0
    samples = []
    all_scores = _scores(rng, 3 * 60)
    for s in range(3):
        labels = rng.integers(0, 10, 24)
        gts = [(int(l), _g(rng, -24, 24), _g(rng, -24, 24), int(rng.integers(0, 5)),
                dict(vel=[math.nan, math.nan]) if rng.uniform() < 0.15 else {}) for l in labels]
        preds = sum((_around(rng, l, gts, 4, 2) for l in range(10)), [])
        samples.append(_sample(rng, [(*p, sc) for p, sc in zip(preds, all_scores[s * 60:])], gts, with_attrs=True))
    out.append(_case("mixed_3x10", samples))
    # at and beyond class_range (car 50 m, pedestrian 40 m, barrier 30 m): 30-40-50 triangles sit exactly on the range
    out.append(_case("class_range", [
        _sample(rng, [(car, 30.0, 40.0, 0.9), (car, 30.0, 39.75, 0.8), (car, 49.0, 11.0, 0.7), (ped, 24.0, 32.0, 0.6),
                      (ped, 24.0, 31.75, 0.5), (barrier, 18.0, 24.0, 0.4), (barrier, 17.75, 24.0, 0.3)],
                [(car, 30.0, 40.0), (car, 30.25, 39.5), (car, 49.0, 10.0), (ped, 24.0, 32.0), (ped, 23.75, 31.75),
                 (barrier, 18.0, 24.0), (barrier, 17.5, 24.0), (car, 60.0, 0.0)])]))
    # annotations without lidar points are dropped before matching
    out.append(_case("num_pts_zero", [
        _sample(rng, [(car, 1.0, 1.0, 0.9), (car, 5.0, 5.0, 0.8)], [(car, 1.0, 1.25, 0), (car, 5.0, 5.5, 3),
                                                                  (car, 1.0, 2.5, 2)])]))
    # NaN ground-truth velocity: every truck match (all-NaN sequence -> ones), one of the car matches (NaN-aware mean)
    nan = dict(vel=[math.nan, math.nan])
    out.append(_case("nan_velocity", [
        _sample(rng, [(truck, 1.0, 1.0, 0.9), (truck, 9.0, 1.0, 0.8), (car, -5.0, 0.25, 0.7), (car, -9.0, 0.5, 0.6),
                      (car, -13.0, 0.25, 0.5)],
                [(truck, 1.0, 1.5, 1, nan), (truck, 9.0, 1.5, 1, nan), (car, -5.0, 0.0, 1, nan), (car, -9.0, 0.0),
                 (car, -13.0, 0.0)])]))
    # yaw differences near pi/2 and pi: period pi for barriers, 2 pi for cars
    diffs = (math.pi / 2 - 0.01, math.pi / 2 + 0.01, math.pi - 0.01, math.pi + 0.01, -math.pi / 2 + 0.01, 0.02,
             2 * math.pi - 0.01)
    preds, gts = [], []
    for i, d in enumerate(diffs):
        for label, y in ((barrier, 2.0), (car, -2.0)):
            yaw = rng.uniform(-1.0, 1.0)
            gts.append((label, -9.0 + 3.0 * i, y, 1, dict(yaw=yaw)))
            preds.append((label, -9.0 + 3.0 * i, y + 0.25, 0.9 - 0.05 * i - (0.02 if label == car else 0.0),
                          dict(yaw=yaw - d)))
    out.append(_case("barrier_yaw", [_sample(rng, preds, gts)]))
    # a class with no ground truth at all next to ordinary ones (counts as 0 in mAP)
    gts = [(car, _g(rng, -20, 20), _g(rng, -20, 20)) for _ in range(6)] + \
          [(ped, _g(rng, -20, 20), _g(rng, -20, 20)) for _ in range(6)]
    preds = _around(rng, car, gts, 8, 3) + _around(rng, ped, gts, 8, 3) + _around(rng, cone, gts, 0, 5)
    out.append(_case("class_without_gt", [_sample(rng, [(*p, s) for p, s in zip(preds, _scores(rng, len(preds)))], gts)]))
    for c in out:
        check_grid(c)
    return out


def hand_case():
    """one car annotation, one car prediction 0.25 m away with score 0.9"""
    rng = np.random.default_rng(1)
    return _case("hand", [_sample(rng, [(C["car"], 10.25, 5.0, 0.9)], [(C["car"], 10.0, 5.0)])])


def check_grid(case):
    """the property the exact fp32 / fp64 agreement of the matcher rests on"""
    for side in ("pred", "gt"):
        for s in case[side]:
            xy = np.asarray(s["boxes"], np.float64)[:, :2]
            assert np.array_equal(xy * GRID, np.round(xy * GRID)), (case["name"], "x, y off the 1/64 m grid")
            assert (np.abs(xy) <= 64).all(), (case["name"], "x, y beyond 64 m")
            assert s["boxes"].dtype == np.float32
    return True
