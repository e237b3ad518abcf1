"""nuScenes detection metrics (mAP, the five true-positive errors, NDS) on the device, without the devkit.

    ev = DetectionEval()                                   # class_names=CLASS_NAMES, config="detection_cvpr_2019"
    result = ev.evaluate(pred, gt)                         # -> the devkit's metrics_summary keys + result["detail"]
    print(format_summary(result))

`pred` / `gt`: one dict per sample, in the same order, of tensors ON THE DEVICE.  Boxes are [N, 9] rows (x, y, z, three
sizes, yaw, vx, vy) in the EGO frame of their sample: the class ranges are distances to the ego origin.  NMSFreeCoder
decodes into the LiDAR frame and the info files annotate in it, so both sides go through `boxes_to_ego` with the sample's
lidar2ego calibration first (`ground_truth_from_infos` does it for the annotations of an info pkl).
    pred[i]: boxes [N, 9], scores [N], labels [N] (index into class_names), optional attrs [N] (index into ATTRIBUTES,
             -1 = none; absent: `default_attributes`, the reference's speed heuristic)
    gt[i]:   boxes [G, 9], labels [G], num_pts [G] (lidar + radar points inside the box), optional attrs [G] (absent: none)

The reference hands all of this to the nuScenes devkit (projects/mmdet3d_plugin/datasets/nuscnes_eval.py:628-676 calls
its accumulate / calc_ap / calc_tp; nuscenes_dataset.py:280-302 flattens the summary into `pts_bbox_NuScenes/...` keys).
The devkit is not part of the reference tree, so its semantics -- the matching rule, the 101-point resampling, calc_ap,
calc_tp, the NaN rules, DetectionMetrics, the constants of detection_cvpr_2019.json below, the attribute names and the
speed heuristic of mmdet3d's `_format_bbox` -- are RECALLED here and NOT PINNED to it; the `detail` key names are the
reference's own.  tests/det_eval_cases.py restates them independently and the two are compared.

Pipeline: class-range and num_pts filtering and the sorts with torch (plumbing), the greedy matching of every (sample,
class, threshold) in one launch of csrc/det_eval.hip (vidar_det_eval_match_f32: one wave per segment and threshold, no
atomics, deterministic), then one fp64 torch pass per class over small arrays.  There is no CPU path.

NOT applied: the devkit's bike-rack filter (bicycles / motorcycles inside a bike-rack annotation are dropped); it needs
annotations the info files do not carry.

`write_results_json` / `read_results_json`: the decoded boxes in the nuScenes detection submission layout, so that a run
can be cross-checked with the devkit elsewhere."""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib
from .configs import CLASS_NAMES

# --- recalled from the devkit (detection_cvpr_2019.json, detection/constants.py); not pinned -------------------------
CONFIGS = {
    "detection_cvpr_2019": dict(
        class_range={"car": 50, "truck": 50, "bus": 50, "trailer": 50, "construction_vehicle": 50, "pedestrian": 40,
                     "motorcycle": 40, "bicycle": 40, "traffic_cone": 30, "barrier": 30},
        dist_ths=(0.5, 1.0, 2.0, 4.0), dist_th_tp=2.0, min_recall=0.1, min_precision=0.1, max_boxes_per_sample=500,
        mean_ap_weight=5),
}
ATTRIBUTES = ("cycle.with_rider", "cycle.without_rider", "pedestrian.moving", "pedestrian.standing",
              "pedestrian.sitting_lying_down", "vehicle.moving", "vehicle.parked", "vehicle.stopped")
TP_METRICS = ("trans_err", "scale_err", "orient_err", "vel_err", "attr_err")
ERR_COLUMNS = ("trans_err", "vel_err", "scale_err", "orient_err", "attr_err")     # columns of the kernel's err[P, 5]
ERR_NAME_MAPPING = {"trans_err": "mATE", "scale_err": "mASE", "orient_err": "mAOE", "vel_err": "mAVE", "attr_err": "mAAE"}
NAN_BY_DEFINITION = {"traffic_cone": ("attr_err", "vel_err", "orient_err"), "barrier": ("attr_err", "vel_err")}
# --- recalled from mmdet3d's NuScenesDataset (DefaultAttribute and the speed rule of _format_bbox); not pinned --------
DEFAULT_ATTRIBUTE = {"car": "vehicle.parked", "pedestrian": "pedestrian.moving", "trailer": "vehicle.parked",
                     "truck": "vehicle.parked", "bus": "vehicle.moving", "motorcycle": "cycle.without_rider",
                     "construction_vehicle": "vehicle.parked", "bicycle": "cycle.without_rider", "barrier": "",
                     "traffic_cone": ""}
_MOVING = {"car": "vehicle.moving", "construction_vehicle": "vehicle.moving", "bus": "vehicle.moving",
           "truck": "vehicle.moving", "trailer": "vehicle.moving", "bicycle": "cycle.with_rider",
           "motorcycle": "cycle.with_rider"}
_STILL = {"pedestrian": "pedestrian.standing", "bus": "vehicle.stopped"}
DETAIL_PREFIX = "pts_bbox_NuScenes"


def _attr_id(name):
    return ATTRIBUTES.index(name) if name else -1


def default_attributes(labels, boxes, class_names=CLASS_NAMES):
    """Attribute ids for predictions that come without: speed > 0.2 m/s -> vehicle.moving for the five vehicle classes,
    cycle.with_rider for bicycle / motorcycle; otherwise pedestrian.standing, vehicle.stopped for a bus; everything else
    the class's DefaultAttribute.  -> int32 [N] on the boxes' device."""
    moving = torch.tensor([_attr_id(_MOVING.get(n, DEFAULT_ATTRIBUTE[n])) for n in class_names], dtype=torch.int32,
                          device=boxes.device)
    still = torch.tensor([_attr_id(_STILL.get(n, DEFAULT_ATTRIBUTE[n])) for n in class_names], dtype=torch.int32,
                         device=boxes.device)
    v = boxes[:, 7:9].double()
    fast = torch.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) > 0.2
    labels = labels.long()
    return torch.where(fast, moving[labels], still[labels])


def _interp(x, xp, fp, right=None):
    """np.interp(x, xp, fp, right=right) for a non-decreasing xp, in numpy's operation order: the last j with
    xp[j] <= x, fp[j] where x == xp[j] or j is the last point, the left edge holds, `right` beyond the last point"""
    n = xp.numel()
    j = torch.searchsorted(xp, x, right=True) - 1
    j0 = j.clamp(0, n - 1)
    j1 = (j0 + 1).clamp(max=n - 1)
    x0, y0 = xp[j0], fp[j0]
    slope = (fp[j1] - y0) / (xp[j1] - x0)
    val = slope * (x - x0) + y0
    val = torch.where((j0 == n - 1) | (x0 == x), y0, val)
    val = torch.where(j < 0, fp[0], val)
    return torch.where(x > xp[-1], fp[-1] if right is None else torch.full_like(val, right), val)


def _order(score, group):
    """rows ordered by group ascending, then score descending, equal scores with the LATER row first -- the devkit's
    sorted((v, i))[::-1] inside every group.  Two sorts on keys that are unique by construction (fp32 score bits mapped
    to a monotone integer | row, then group | rank), so that nothing rests on a sort being stable."""
    n = score.numel()
    row = torch.arange(n, device=score.device)
    bits = (score.float() + 0.0).contiguous().view(torch.int32)         # + 0.0: -0.0 and 0.0 are one score
    mono = torch.where(bits >= 0, bits, bits ^ 0x7FFFFFFF).long()      # increasing with the score
    by_score = torch.sort(mono * (1 << 32) + row, descending=True).indices
    rank = torch.empty_like(row)
    rank[by_score] = row
    return torch.sort(group.long() * (1 << 32) + rank).indices


def _starts(group, n_groups):
    s = torch.zeros(n_groups + 1, dtype=torch.int64, device=group.device)
    s[1:] = torch.cumsum(torch.bincount(group, minlength=n_groups), 0)
    return s.to(torch.int32)


class Matched:
    """Filtered, flattened boxes and the matcher's verdicts, all in the filtered input order.
    match [NT, P]: matched row of the filtered ground truth or -1; gt_match [NT, G]: matched prediction row or -1;
    err [P, 5] (ERR_COLUMNS) at dist_th_tp, NaN rows where unmatched."""
    __slots__ = ("scores", "labels", "gt_labels", "match", "gt_match", "err", "pred_keep", "gt_keep")


class DetectionEval:
    def __init__(self, class_names=CLASS_NAMES, config="detection_cvpr_2019"):
        cfg = CONFIGS[config] if isinstance(config, str) else dict(config)
        self.class_names = tuple(class_names)
        unknown = [n for n in self.class_names if n not in cfg["class_range"]]
        if unknown:
            raise ValueError(f"no class_range for {unknown}")
        self.cfg = cfg
        self.dist_ths = tuple(float(t) for t in cfg["dist_ths"])
        self.tp_index = self.dist_ths.index(float(cfg["dist_th_tp"]))

    # ------------------------------------------------------------------------------------------------------------
    def _flatten(self, samples, keys, what):
        if not all(all(isinstance(s[k], torch.Tensor) and s[k].is_cuda for k in keys) and
                   (s.get("attrs") is None or s["attrs"].is_cuda) for s in samples):
            raise RuntimeError(f"DetectionEval: the {what} tensors must be on the GPU (vidar_amd has no CPU path)")
        dev = samples[0]["boxes"].device
        counts = [int(s["boxes"].shape[0]) for s in samples]
        for s, n in zip(samples, counts):
            if s["boxes"].dim() != 2 or s["boxes"].shape[1] != 9 or any(s[k].shape[0] != n for k in keys):
                raise ValueError(f"DetectionEval: {what} boxes must be [N, 9] with N entries in {keys[1:]}")
        sample = torch.repeat_interleave(torch.arange(len(samples), device=dev),
                                         torch.tensor(counts, device=dev), output_size=sum(counts))
        cat = {k: torch.cat([s[k] for s in samples]) for k in keys}
        has = [s.get("attrs") is not None for s in samples]
        if any(has) and not all(has):
            raise ValueError(f"DetectionEval: attrs given for some {what} samples only")
        cat["attrs"] = torch.cat([s["attrs"] for s in samples]).to(torch.int32) if all(has) else None
        return sample, cat, counts

    def prepare(self, pred, gt) -> dict:
        """Filter by class range and num_pts, flatten, and put both sides into the matcher's layout: grouped by segment
        (sample * C + class), the predictions of a segment in processing order."""
        if len(pred) != len(gt):
            raise ValueError("DetectionEval: pred and gt must list the same samples")
        if len(pred) == 0:
            raise ValueError("DetectionEval: no samples")
        C = len(self.class_names)
        ps, p, counts = self._flatten(pred, ("boxes", "scores", "labels"), "prediction")
        gs, g, _ = self._flatten(gt, ("boxes", "labels", "num_pts"), "ground-truth")
        if max(counts) > self.cfg["max_boxes_per_sample"]:
            raise ValueError(f"DetectionEval: only <= {self.cfg['max_boxes_per_sample']} boxes per sample allowed, "
                             f"got {max(counts)}")
        dev = p["boxes"].device
        plab, glab = p["labels"].long(), g["labels"].long()
        if bool(((plab < 0) | (plab >= C)).any()) or bool(((glab < 0) | (glab >= C)).any()):
            raise ValueError(f"DetectionEval: labels outside 0 .. {C - 1}")
        rng = torch.tensor([float(self.cfg["class_range"][n]) for n in self.class_names], dtype=torch.float64, device=dev)

        def radius(b):
            xy = b[:, :2].double()
            return torch.sqrt(xy[:, 0] * xy[:, 0] + xy[:, 1] * xy[:, 1])
        pkeep = radius(p["boxes"]) < rng[plab]
        gkeep = (radius(g["boxes"]) < rng[glab]) & (g["num_pts"] > 0)
        pbox, gbox = p["boxes"][pkeep].float(), g["boxes"][gkeep].float()
        plab, glab, score = plab[pkeep], glab[gkeep], p["scores"][pkeep].float()     # scores are compared in fp32
        pattr = p["attrs"][pkeep] if p["attrs"] is not None else default_attributes(plab, pbox, self.class_names)
        gattr = g["attrs"][gkeep] if g["attrs"] is not None else None
        NS = len(pred) * C
        pseg, gseg = ps[pkeep] * C + plab, gs[gkeep] * C + glab
        po = _order(score, pseg)                                   # the kernel's processing order
        go = torch.sort(gseg * (1 << 32) + torch.arange(gseg.numel(), device=dev)).indices     # by segment, input order inside
        return dict(scores=score, labels=plab, gt_labels=glab, pred_keep=pkeep, gt_keep=gkeep, po=po, go=go, NS=NS,
                    pred_box=pbox[po].contiguous(), pred_attr=pattr[po].contiguous(), pred_start=_starts(pseg, NS),
                    gt_box=gbox[go].contiguous(), gt_attr=gattr[go].contiguous() if gattr is not None else None,
                    gt_start=_starts(gseg, NS))

    def run_matcher(self, k):
        """One launch of vidar_det_eval_match_f32 on prepared operands -> (match [NT, P], gt_match [NT, G], err [P, 5]) in
        the kernel's row order."""
        P, G, NT = k["pred_box"].shape[0], k["gt_box"].shape[0], len(self.dist_ths)
        dev = k["pred_box"].device
        match = torch.empty(NT, P, dtype=torch.int32, device=dev)
        gt_match = torch.empty(NT, G, dtype=torch.int32, device=dev)
        err = torch.empty(P, 5, dtype=torch.float32, device=dev)
        ths = (ctypes.c_float * NT)(*self.dist_ths)                # host array
        barrier = self.class_names.index("barrier") if "barrier" in self.class_names else -1
        ptr = _lib.ptr
        with _lib.TIMER.span("det_eval_match", 36 * (P + G)):
            _lib.check(_lib.lib().vidar_det_eval_match_f32(
                ptr(k["pred_box"]), ptr(k["pred_attr"]), ptr(k["pred_start"]), ptr(k["gt_box"]), ptr(k["gt_attr"]),
                ptr(k["gt_start"]), ths, ptr(match), ptr(gt_match), ptr(err), P, G, k["NS"], NT, self.tp_index,
                len(self.class_names), barrier, _lib.stream_of(k["pred_box"])), "det_eval_match")
        return match, gt_match, err

    def match(self, pred, gt) -> Matched:
        """prepare + run_matcher, with the verdicts brought back to the filtered input order on both sides."""
        k = self.prepare(pred, gt)
        k_match, k_gmatch, k_err = self.run_matcher(k)
        po, go = k["po"], k["go"]
        m = Matched()
        m.scores, m.labels, m.gt_labels, m.pred_keep, m.gt_keep = (k[n] for n in ("scores", "labels", "gt_labels",
                                                                                  "pred_keep", "gt_keep"))
        km, kg = k_match.long(), k_gmatch.long()
        m.match = torch.empty_like(km)
        m.match[:, po] = torch.where(km >= 0, go[km.clamp(min=0)], km) if go.numel() else km
        m.gt_match = torch.empty_like(kg)
        m.gt_match[:, go] = torch.where(kg >= 0, po[kg.clamp(min=0)], kg) if po.numel() else kg
        m.err = torch.empty_like(k_err)
        m.err[po] = k_err
        return m

    # ------------------------------------------------------------------------------------------------------------
    def evaluate(self, pred, gt) -> dict:
        return self.metrics(self.match(pred, gt))

    def metrics(self, m: Matched) -> dict:
        """The passes after the matching, in fp64 with torch on the verdicts' device: per class and threshold the
        precision / recall curve and AP, per class the five true-positive errors, then the summary."""
        cfg, names, NT = self.cfg, self.class_names, len(self.dist_ths)
        C = len(names)
        dev = m.scores.device
        f64 = dict(dtype=torch.float64, device=dev)
        first = round(100 * cfg["min_recall"]) + 1
        conf_all = m.scores.double()
        order = _order(m.scores, m.labels)                          # per class: the devkit's global processing order
        hit = m.match >= 0
        tp_count = torch.zeros(NT, C, **f64).index_add_(1, m.labels, hit.double())
        host = torch.cat([torch.bincount(m.labels, minlength=C).double(), torch.bincount(m.gt_labels, minlength=C).double(),
                          tp_count.reshape(-1)]).tolist()          # the one host read ahead of the per-class passes
        npred, npos, tp_count = host[:C], host[C:2 * C], [host[2 * C + t * C: 2 * C + (t + 1) * C] for t in range(NT)]
        rec_i = torch.arange(101, **f64) * 0.01                    # np.linspace(0, 1, 101): i * step
        rec_i[-1] = 1.0
        ar = torch.arange(101, device=dev)
        one, zero = torch.ones((), **f64), torch.zeros((), **f64)
        aps, tps = [], []
        start = 0
        for c in range(C):
            idx = order[start: start + int(npred[c])]
            start += int(npred[c])
            conf = conf_all[idx]
            # a tensor divisor: torch turns `tensor / python_number` into a multiplication by the reciprocal on the
            # device, which is one ulp off a / b for some values and moves the `rec == recall point` decisions
            npos_c = torch.tensor(npos[c], **f64)
            for t in range(NT):
                if npos[c] == 0 or tp_count[t][c] == 0:            # the devkit's no_predictions()
                    aps.append(zero)
                    if t == self.tp_index:
                        tps += [one] * 5
                    continue
                tpf = hit[t, idx]
                tp, fp = torch.cumsum(tpf.double(), 0), torch.cumsum((~tpf).double(), 0)
                prec, rec = tp / (fp + tp), tp / npos_c
                prec_i = _interp(rec_i, rec, prec, right=0.0)
                aps.append((prec_i[first:] - cfg["min_precision"]).clamp(min=0).mean() / (1.0 - cfg["min_precision"]))
                if t != self.tp_index:
                    continue
                conf_i = _interp(rec_i, rec, conf, right=0.0)
                last = torch.where(conf_i != 0, ar, torch.zeros_like(ar)).max()        # max_recall_ind
                window = (ar >= first) & (ar <= last)
                mconf = conf[tpf].flip(0)                           # ascending, as np.interp wants it
                errs = m.err[idx][tpf].double()
                for e in range(5):
                    x = errs[:, e]
                    nan = torch.isnan(x)
                    cnt = torch.cumsum((~nan).double(), 0)
                    cm = torch.where(cnt > 0, torch.cumsum(torch.where(nan, zero, x), 0) / cnt.clamp(min=1), zero)
                    cm = torch.where(nan.all(), torch.ones_like(cm), cm)               # cummean: all NaN -> ones
                    curve = _interp(conf_i.flip(0), mconf, cm.flip(0)).flip(0)
                    mean = torch.where(window, curve, zero).sum() / window.sum().clamp(min=1)
                    tps.append(torch.where(last < first, one, mean))                   # calc_tp
        aps = torch.stack(aps).reshape(C, NT).tolist()
        tps = torch.stack(tps).reshape(C, 5).tolist()
        label_aps = {n: {th: aps[c][t] for t, th in enumerate(self.dist_ths)} for c, n in enumerate(names)}
        label_tp = {n: {e: (float("nan") if e in NAN_BY_DEFINITION.get(n, ()) else tps[c][ERR_COLUMNS.index(e)])
                        for e in TP_METRICS} for c, n in enumerate(names)}
        return summarize(label_aps, label_tp, cfg["mean_ap_weight"])


def summarize(label_aps, label_tp_errors, mean_ap_weight=5):
    """DetectionMetrics.serialize() without the run time, plus the reference's flat `detail` keys"""
    mean_dist_aps = {n: sum(d.values()) / len(d) for n, d in label_aps.items()}
    mean_ap = sum(mean_dist_aps.values()) / len(mean_dist_aps)
    tp_errors = {}
    for e in TP_METRICS:
        vals = [v[e] for v in label_tp_errors.values() if not math.isnan(v[e])]
        tp_errors[e] = sum(vals) / len(vals) if vals else float("nan")
    tp_scores = {e: max(0.0, 1.0 - v) for e, v in tp_errors.items()}
    nd_score = (mean_ap_weight * mean_ap + sum(tp_scores.values())) / (mean_ap_weight + len(tp_scores))
    detail = {}
    for n in label_aps:
        for th, v in label_aps[n].items():
            detail[f"{DETAIL_PREFIX}/{n}_AP_dist_{th}"] = float(f"{v:.4f}")
        for e, v in label_tp_errors[n].items():
            detail[f"{DETAIL_PREFIX}/{n}_{e}"] = float(f"{v:.4f}")
    for e, v in tp_errors.items():
        detail[f"{DETAIL_PREFIX}/{ERR_NAME_MAPPING[e]}"] = float(f"{v:.4f}")
    detail[f"{DETAIL_PREFIX}/NDS"] = nd_score
    detail[f"{DETAIL_PREFIX}/mAP"] = mean_ap
    return dict(label_aps=label_aps, label_tp_errors=label_tp_errors, mean_dist_aps=mean_dist_aps, mean_ap=mean_ap,
                tp_errors=tp_errors, tp_scores=tp_scores, nd_score=nd_score, detail=detail)


def format_summary(result, gt_attrs=True) -> str:
    """the devkit's closing table (without its run time); `gt_attrs=False`: the ground truth came without attributes
    (`ground_truth_from_infos`), which the table then says"""
    lines = ["mAP: %.4f" % result["mean_ap"]]
    lines += ["%s: %.4f" % (ERR_NAME_MAPPING[e], v) for e, v in result["tp_errors"].items()]
    lines += ["NDS: %.4f" % result["nd_score"], "Per-class results:", "Object Class\tAP\tATE\tASE\tAOE\tAVE\tAAE"]
    for n, ap in result["mean_dist_aps"].items():
        tp = result["label_tp_errors"][n]
        lines.append("%s\t%.3f\t%.3f\t%.3f\t%.3f\t%.3f\t%.3f" % (n, ap, tp["trans_err"], tp["scale_err"], tp["orient_err"],
                                                                 tp["vel_err"], tp["attr_err"]))
    if not gt_attrs:
        lines.append("(the info files carry no attributes: mAAE is 1 by construction and NDS is lower than the devkit's by "
                     "that term)")
    return "\n".join(lines)


# --- from LiDAR-frame boxes and info files to what `evaluate` takes, and the submission file ---------------------------
MODALITY = dict(use_lidar=False, use_camera=True, use_radar=False, use_map=False, use_external=True)


def _rotation_matrices(q):
    """unit quaternions (w, x, y, z) [..., 4] fp64 -> rotation matrices [..., 3, 3] ([3P] pyquaternion's formula)"""
    q = q / q.norm(dim=-1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    rows = [1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
            2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
            2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]
    return torch.stack(rows, -1).reshape(*q.shape[:-1], 3, 3)


def _quat_mul(a, b):
    aw, ax, ay, az = a.unbind(-1)
    bw, bx, by, bz = b.unbind(-1)
    return torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def _f64(a, device):
    return torch.as_tensor(a, dtype=torch.float64, device=device)


def _rigid(boxes, rotation, translation):
    """fp64: centres R c + t, the heading vector (cos h, sin h, 0) and the velocity (vx, vy, 0) rotated.  The heading
    angle h = -yaw - pi/2 is formed in fp32, as output_to_nusc_box_det forms it on the fp32 yaw column, then widened."""
    b = boxes.double()
    R = _rotation_matrices(_f64(rotation, b.device))
    t = _f64(translation, b.device)
    rot = lambda v: (R @ v.unsqueeze(-1)).squeeze(-1)
    zero = torch.zeros_like(b[:, 0])
    h = (-boxes[:, 6].float() - math.pi / 2).double()
    return b, rot(b[:, :3]) + t, rot(torch.stack([torch.cos(h), torch.sin(h), zero], -1)), \
        rot(torch.stack([b[:, 7], b[:, 8], zero], -1)), h


def boxes_to_ego(boxes, rotation, translation):
    """Rigid transform of box rows [N, 9] (centre, sizes, yaw, vx, vy): the centre is rotated and moved, the velocity
    (vx, vy, 0) rotated, the sizes untouched; the heading (the x axis of the box, at -yaw - pi/2 in the devkit's
    convention for these LiDAR-style rows) is rotated and its yaw read off again as the devkit's quaternion_yaw does --
    for a rotation about z that ADDS the rotation's yaw to the heading, i.e. subtracts it from the row's yaw.
    `rotation`: unit quaternion(s) (w, x, y, z), [4] or one per box [N, 4]; `translation`: [3] or [N, 3]; both may be lists,
    arrays or tensors.  Computed in fp64 on the boxes' device, stored as fp32.  With lidar2ego_rotation / _translation of
    a sample this takes LiDAR-frame boxes to the ego frame (lidar_nusc_box_to_global,
    UniAD/projects/mmdet3d_plugin/datasets/data_utils/data_utils.py:118-126); feed it gravity-centred rows."""
    b, c, head, vel, _ = _rigid(boxes, rotation, translation)
    yaw = -torch.atan2(head[:, 1], head[:, 0]) - math.pi / 2
    return torch.cat([c, b[:, 3:6], yaw[:, None], vel[:, :2]], 1).float()


def ground_truth_from_infos(infos, class_names=CLASS_NAMES, device="cuda"):
    """the `gt` list of `DetectionEval.evaluate` from the frames of an info pkl (vidar_amd.data.load_infos), one entry per
    frame in their order: EVERY annotation of the frame whose name is in `class_names` (not the `valid_flag` subset: the
    evaluator's own num_pts > 0 filter removes the same boxes the devkit removes), `num_pts` = lidar + radar points (lidar
    alone where the file has no `num_radar_pts`),
    gravity-centred boxes moved from the LiDAR frame to the ego frame of the sample with `boxes_to_ego`; a NaN velocity
    stays NaN, as in the devkit (such a match does not count in mAVE).
    No attributes: the info files carry none.  Every attr_err is then NaN, mAAE is 1 and NDS is lower than the devkit's by
    that term (1/10 of the devkit's 1 - mAAE)."""
    import numpy as np
    if len(infos) == 0:
        return []
    class_names = list(class_names)
    rows, labels, num_pts, quat, trans, counts = [], [], [], [], [], []
    for info in infos:
        names = np.asarray(info["gt_names"])
        keep = np.array([n in class_names for n in names], bool).reshape(-1)
        box = np.concatenate([np.asarray(info["gt_boxes"], np.float64).reshape(-1, 7),
                              np.asarray(info["gt_velocity"], np.float64).reshape(-1, 2)], 1)[keep]
        rows.append(box)
        labels.append(np.array([class_names.index(n) for n in names[keep]], np.int64))
        pts = np.asarray(info["num_lidar_pts"], np.int64)
        if "num_radar_pts" in info:                      # as annotations.ann_info: older info files carry lidar counts only
            pts = pts + np.asarray(info["num_radar_pts"], np.int64)
        num_pts.append(pts[keep])
        quat.append(np.broadcast_to(np.asarray(info["lidar2ego_rotation"], np.float64), (len(box), 4)))
        trans.append(np.broadcast_to(np.asarray(info["lidar2ego_translation"], np.float64), (len(box), 3)))
        counts.append(len(box))
    dev = torch.device(device)
    boxes = boxes_to_ego(torch.from_numpy(np.concatenate(rows)).float().to(dev), np.concatenate(quat), np.concatenate(trans))
    labels = torch.from_numpy(np.concatenate(labels)).to(dev)
    num_pts = torch.from_numpy(np.concatenate(num_pts)).to(dev)
    return [dict(boxes=b, labels=l, num_pts=n)
            for b, l, n in zip(boxes.split(counts), labels.split(counts), num_pts.split(counts))]


def _attribute_name(name, speed):
    """the speed rule of _format_bbox_det (nuscenes_e2e_dataset.py:903-922)"""
    if speed > 0.2:
        return _MOVING.get(name, DEFAULT_ATTRIBUTE[name])
    return _STILL.get(name, DEFAULT_ATTRIBUTE[name])


def write_results_json(path, tokens, pred, infos, class_names=CLASS_NAMES, config="detection_cvpr_2019", meta=None):
    """the decoded boxes in the nuScenes detection submission layout: {"meta": ..., "results": {token: [entry, ...]}}, an
    entry holding sample_token, translation, size, rotation (w, x, y, z), velocity, detection_name, detection_score and
    attribute_name, boxes in the GLOBAL frame.
    `pred[i]`: dict(boxes [N, 9] LiDAR-frame rows with the z of the BOTTOM face -- `boxes_3d.tensor` of the detector's
    result --, scores [N], labels [N]) of the frame `tokens[i]` / `infos[i]`, tensors anywhere.
    Semantics of output_to_nusc_box_det + lidar_nusc_box_to_global (UniAD/projects/mmdet3d_plugin/datasets/data_utils/
    data_utils.py:53-132) + _format_bbox_det (nuscenes_e2e_dataset.py:873-945): gravity centre, the yaw -yaw - pi/2 as a
    quaternion about z, boxes farther from the ego origin than their class range dropped (in the ego frame), then
    ego2global; the attribute name from the speed in the global frame.  ([3P] the devkit's Box and pyquaternion are
    restated in fp64.)  -> kept[i]: the rows of pred[i] that were written, in order."""
    import json
    import numpy as np
    from pathlib import Path
    class_names = list(class_names)
    ranges = CONFIGS[config]["class_range"] if isinstance(config, str) else config["class_range"]
    results, kept = {}, []
    for token, p, info in zip(tokens, pred, infos):
        if token != info["token"]:
            raise ValueError(f"write_results_json: prediction of {token!r} paired with the info of {info['token']!r}")
        box = p["boxes"].detach().cpu().float()
        box = torch.cat([box[:, :2], (box[:, 2] + box[:, 5] * 0.5)[:, None], box[:, 3:]], 1)      # gravity_center, fp32
        labels = p["labels"].detach().cpu().long()
        scores = p["scores"].detach().cpu().float()
        n = len(box)
        l2e, e2g = (_f64(info[k], "cpu") for k in ("lidar2ego_rotation", "ego2global_rotation"))
        b, ego_c, _, ego_v, h = _rigid(box, l2e, info["lidar2ego_translation"])
        q = torch.stack([torch.cos(h / 2), torch.zeros_like(h), torch.zeros_like(h), torch.sin(h / 2)], -1)
        q = _quat_mul(e2g.expand(n, 4), _quat_mul(l2e.expand(n, 4), q))
        radius = torch.sqrt(ego_c[:, 0] * ego_c[:, 0] + ego_c[:, 1] * ego_c[:, 1])
        keep = ~(radius > _f64([ranges[class_names[int(l)]] for l in labels], "cpu"))
        R = _rotation_matrices(e2g)
        glob_c = ego_c @ R.T + _f64(info["ego2global_translation"], "cpu")
        glob_v = ego_v @ R.T
        entries = []
        for i in torch.nonzero(keep).flatten().tolist():
            name = class_names[int(labels[i])]
            v = glob_v[i, :2].tolist()
            entries.append(dict(sample_token=token, translation=glob_c[i].tolist(), size=b[i, 3:6].tolist(),
                                rotation=q[i].tolist(), velocity=v, detection_name=name, detection_score=float(scores[i]),
                                attribute_name=_attribute_name(name, float(np.sqrt(v[0] ** 2 + v[1] ** 2)))))
        results[token] = entries
        kept.append(torch.nonzero(keep).flatten())
    Path(path).parent.mkdir(parents=True, exist_ok=True)
    Path(path).write_text(json.dumps(dict(meta=dict(meta or MODALITY), results=results)))
    return kept


def read_results_json(path, infos=None, class_names=CLASS_NAMES, device="cpu"):
    """a submission file -> (tokens, pred): pred[i] = dict(boxes [N, 9] fp32 rows with the gravity centre, scores,
    labels, attrs (index into ATTRIBUTES, -1 for "")) of tokens[i], plus `rotation` [N, 4] fp64 (the file's quaternion;
    the row's yaw is the devkit's quaternion_yaw of it, brought back to the rows' convention).
    Without `infos` the frames come in the file's order and the boxes stay in the GLOBAL frame.  With `infos` the result
    lists THEIR frames in THEIR order (a frame the file lacks is an error) and the boxes are moved into each sample's EGO
    frame with the inverse of ego2global (on quaternions, so that the file's orientation loses nothing on the way): what
    `DetectionEval.evaluate` takes next to `ground_truth_from_infos(infos)`.  The layout keeps two components of the
    global-frame velocity: with a tilted ego2global the vertical one is gone, and the ego-frame velocity read back is off
    by up to |R[2, :2]| |v_z| from the one `boxes_to_ego` gives the same box."""
    import json
    from pathlib import Path
    class_names = list(class_names)
    results = json.loads(Path(path).read_text())["results"]
    tokens = list(results) if infos is None else [info["token"] for info in infos]
    dev = torch.device(device)
    pred = []
    for k, token in enumerate(tokens):
        if token not in results:
            raise KeyError(f"{path}: no results for sample {token!r}")
        ent = results[token]
        col = lambda key, width: _f64([e[key] for e in ent], "cpu").reshape(len(ent), width)
        c, size, q, v = col("translation", 3), col("size", 3), col("rotation", 4), col("velocity", 2)
        if infos is not None:
            inv = _f64(infos[k]["ego2global_rotation"], "cpu") * _f64([1.0, -1.0, -1.0, -1.0], "cpu")
            R = _rotation_matrices(inv)
            c = (c - _f64(infos[k]["ego2global_translation"], "cpu")) @ R.T
            v = (torch.cat([v, torch.zeros(len(ent), 1, dtype=torch.float64)], 1) @ R.T)[:, :2]
            q = _quat_mul(inv.expand(len(ent), 4), q)
        head = _rotation_matrices(q)[:, :, 0] if len(ent) else torch.zeros(0, 3, dtype=torch.float64)
        yaw = -torch.atan2(head[:, 1], head[:, 0]) - math.pi / 2
        pred.append(dict(boxes=torch.cat([c, size, yaw[:, None], v], 1).float().to(dev), rotation=q,
                         scores=torch.tensor([e["detection_score"] for e in ent], dtype=torch.float32, device=dev),
                         labels=torch.tensor([class_names.index(e["detection_name"]) for e in ent], dtype=torch.int64,
                                             device=dev),
                         attrs=torch.tensor([_attr_id(e["attribute_name"]) for e in ent], dtype=torch.int32, device=dev)))
    return tokens, pred
