"""Shared inputs and the torch restatement of tests/test_occ_score_{cpu,gpu}.py: the occupancy score
(vidar_occ_score_f32, include/vidar_hip.h).  torch + numpy only, no GPU, no kernel of the product.

table(): per voxel, in the dtype of its input (fp32: every torch operation rounds on its own, as the kernel's do),
    ev_p = hit_p + free_p   ev_m = hit_m + free_m   o_p = hit_p / ev_p
    both = ev_p >= min_pred && ev_m >= min_meas     y = hit_m >= min_hits
voxels with a non-finite plane left out, then the columns n_pred, n_meas, n_both, n_occ, brier (fp64), tp / fp / fn per
threshold, cnt / pos per bin of o_p, as fp64 sums of 0 / 1 masks.

lattice(): seeded grids on the lattice of eighths in [0, 4], about half of them zeros and a quarter in [0, 1], so that
values sit exactly on every floor and threshold (ev == 0.5, o_p == 0.25, hit_m == 0.125): both sides must put them on
the same side.

wall_scene(): a scene where right and wrong are known -- the `plane` volume of ray_stats_cases (logits -2, the layer
x = 40 at 14), one origin for both frames, 300 rays per frame whose measured returns lie on the forecast's wall in
frame 0 (x = 40.5 +- 0.3) and six voxels nearer in frame 1 (x = 34.5 +- 0.3).  pipeline64() is the fp64 restatement of
ray_occupancy -> sweep_evidence -> occupancy_score on it.  Measured on the CPU at the marches (64, 1.0), (128, 0.5),
(200, 0.25), thresholds (0.125, 0.25, 0.5):

                          agreeing wall (frame 0)     displaced wall (frame 1)
    IoU at 0.25           0.617 / 0.621 / 0.576       tp == 0, fn = 97 / 97 / 97
    Brier                 0.046 / 0.053 / 0.062       0.145 / 0.140 / 0.136
    n_both                779 / 808 / 823             667 / 694 / 713
    borderline voxels     0 / 2 / 0                   0 / 0 / 1
"""
import math

import numpy as np
import torch

import ray_occupancy_cases as RO
import ray_stats_cases as RS
import sweep_evidence_cases as SE

FLOORS = dict(min_pred=0.5, min_meas=0.5, min_hits=0.125)


def columns(T, B):
    return 5 + 3 * T + 2 * B


def classify(pred, meas, min_pred, min_meas, min_hits):
    """pred, meas [S, 2, V] in one dtype -> dict of [S, V] tensors: pred_ok, meas_ok, both, y (bool), o_p, ev_p, ev_m"""
    dt = pred.dtype
    c = lambda v: torch.tensor(v, dtype=dt)
    hp, fp, hm, fm = pred[:, 0], pred[:, 1], meas[:, 0], meas[:, 1]
    finite = torch.isfinite(hp) & torch.isfinite(fp) & torch.isfinite(hm) & torch.isfinite(fm)
    ev_p, ev_m = hp + fp, hm + fm
    pred_ok = finite & (ev_p >= c(min_pred))
    meas_ok = finite & (ev_m >= c(min_meas))
    return dict(pred_ok=pred_ok, meas_ok=meas_ok, both=pred_ok & meas_ok, y=hm >= c(min_hits), o_p=hp / ev_p, ev_p=ev_p,
                ev_m=ev_m, hit_m=hm)


def table(pred, meas, thresholds, bins, min_pred=0.5, min_meas=0.5, min_hits=0.125):
    """-> [S, 5 + 3T + 2B] float64"""
    dt = pred.dtype
    v = classify(pred, meas, min_pred, min_meas, min_hits)
    both, y, o_p = v["both"], v["y"], v["o_p"]
    n = lambda m: m.double().sum(1)
    term = (o_p.double() - y.double()) ** 2
    cols = [n(v["pred_ok"]), n(v["meas_ok"]), n(both), n(both & y),
            torch.where(both, term, torch.zeros_like(term)).sum(1)]
    for t in thresholds:
        yhat = o_p >= torch.tensor(float(t), dtype=dt)
        cols += [n(both & yhat & y), n(both & yhat & ~y), n(both & ~yhat & y)]
    if bins:
        b = (torch.where(both, o_p, torch.zeros_like(o_p)) * bins).long().clamp(max=bins - 1)
        for k in range(bins):
            cols += [n(both & (b == k)), n(both & (b == k) & y)]
    return torch.stack(cols, 1)


def lattice(S, V, seed):
    """-> (pred, meas) [S, 2, V] fp32 on the lattice of eighths in [0, 4], about half zeros"""
    g = torch.Generator().manual_seed(seed)

    def draw():
        # half of the non-zero values from [0, 1]: evidence sums and ratios of small eighths hit the boundaries often
        wide = torch.randint(0, 33, (S, 2, V), generator=g)
        small = torch.randint(0, 9, (S, 2, V), generator=g)
        x = torch.where(torch.rand(S, 2, V, generator=g) < 0.5, small, wide).float() / 8
        return torch.where(torch.rand(S, 2, V, generator=g) < 0.5, torch.zeros_like(x), x)
    return draw(), draw()


def on_a_boundary(pred, meas, thresholds, min_pred=0.5, min_meas=0.5, min_hits=0.125):
    """how many voxels sit EXACTLY on (a floor of the evidence, min_hits, a threshold); the lattice must have all three"""
    v = classify(pred, meas, min_pred, min_meas, min_hits)
    floor = int(((v["ev_p"] == min_pred) | (v["ev_m"] == min_meas)).sum())
    hits = int((v["hit_m"] == min_hits).sum())
    th = int(sum(((v["o_p"] == float(t)) & v["both"]).sum() for t in thresholds))
    return floor, hits, th


def borderline(pred, meas, thresholds, eps=1e-3, min_pred=0.5, min_meas=0.5, min_hits=0.125):
    """[S] int: voxels of the restatement whose decision could flip under an error of eps -- an evidence within eps of
    its floor, hit_m within eps of min_hits, or o_p within eps of a threshold (where both grids speak or nearly do)"""
    v = classify(pred, meas, min_pred, min_meas, min_hits)
    near = ((v["ev_p"] - min_pred).abs() <= eps) | ((v["ev_m"] - min_meas).abs() <= eps)
    near |= (v["hit_m"] - min_hits).abs() <= eps
    close = (v["ev_p"] >= min_pred - eps) & (v["ev_m"] >= min_meas - eps)
    for t in thresholds:
        near |= close & ((v["o_p"] - float(t)).abs() <= eps)
    return near.sum(1)


# ---- the scene with a wall ---------------------------------------------------------------------------------------------
WALL_MARCHES = [(64, 1.0), (128, 0.5), (200, 0.25)]
WALL_IDS = [f"K{K}-step{step}" for K, step in WALL_MARCHES]
WALL_THRESHOLDS = (0.125, 0.25, 0.5)
WALL_RAYS = 300
WALL_X = (RS.PLANE_X + 0.5, RS.PLANE_X + 0.5 - 6.0)       # frame 0: on the forecast's wall; frame 1: six voxels nearer


def wall_scene():
    """-> sigma [2,4,10,96], origin [2,3], pts [600,3], tindex [600] (fp32)"""
    rng = np.random.default_rng(3)
    pts, tindex = [], []
    for f, x in enumerate(WALL_X):
        y = rng.uniform(0.7, 9.3, WALL_RAYS)
        z = rng.uniform(0.6, 3.4, WALL_RAYS)
        pts.append(np.stack([x + rng.uniform(-0.3, 0.3, WALL_RAYS), y, z], 1))
        tindex.append(np.full(WALL_RAYS, float(f)))
    origin = torch.tensor([RS.ORIGINS[0], RS.ORIGINS[0]], dtype=torch.float32)
    return (RS.volume("plane"), origin, torch.from_numpy(np.concatenate(pts)).float(),
            torch.from_numpy(np.concatenate(tindex)).float())


_WALL = {}


def pipeline64(K, step):
    """fp64 restatement of the whole pipeline on the wall scene -> dict(pred, meas [2, 2, V] fp64, table [2, cols],
    borderline [2]); once per march"""
    key = (K, step)
    if key not in _WALL:
        sigma, origin, pts, tindex = wall_scene()
        pred = torch.stack(RO.occupancy(sigma.double(), origin, pts, tindex, K, step), 1).reshape(2, 2, -1)
        meas = torch.stack(SE.evidence(tuple(sigma.shape), origin, pts, tindex, K, step, torch.float64), 1).reshape(2, 2, -1)
        _WALL[key] = dict(pred=pred, meas=meas, table=table(pred, meas, WALL_THRESHOLDS, 10),
                          borderline=borderline(pred, meas, WALL_THRESHOLDS))
    return _WALL[key]


def iou(row, j):
    tp, fp, fn = (float(row[5 + 3 * j + i]) for i in range(3))
    return tp / (tp + fp + fn) if tp + fp + fn else math.nan
