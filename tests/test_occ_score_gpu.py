"""GPU: the occupancy score (vidar_occ_score_f32, csrc/occ_score.hip) and what is built on it.

1. the table against the torch fp32 restatement (tests/occ_score_cases.py) on lattice grids whose values sit exactly on
   every floor and threshold: S = 3 with V = 7 * 9 * 33, V = 1 and V = 100 003 (several tiles), T = 1, 3, 8 (with
   duplicates), B = 0, 10, 16; every count equal, brier within 1e-12 relative, equal bits over two runs; voxels with a
   NaN / inf in any plane are left out of every column;
2. end to end on a scene where right and wrong are known (occ_score_cases.wall_scene): ray_occupancy -> sweep_evidence ->
   occupancy_score on the device against the fp64 restatement of the pipeline.  A count may differ by at most the number
   of borderline voxels of the restatement (a decision within 1e-3 of flipping), which must stay <= 1 % of n_both; the
   restatement itself must call the agreeing wall right (IoU at 0.25 >= 0.5) and the displaced wall wrong (tp == 0,
   fn > 0, a larger Brier score);
3. the head and the detector: measured_occupancy is sweep_evidence on the decode's own rays; forward_test carries the
   `occ.*` entries with the option on and is unchanged with it off, on the host and on the device tail.

Measured on an MI355X: every count of part 2 EQUAL to the restatement's at all three marches and in both frames (the 0 - 2
borderline voxels fell on the restatement's side); |brier sum - restatement's| <= 9.2e-6 on sums of 36 .. 97."""
import math

import numpy as np
import pytest
import torch

import occ_score_cases as OC
from test_ray_occupancy_gpu import small_model  # noqa: F401  (the reduced detector, built once per module)

pytestmark = pytest.mark.gpu

SHAPES = {"V2079": (3, 2, 7, 9, 33), "V1": (3, 2, 1), "V100003": (3, 2, 100003)}
SEEDS = {"V2079": 21, "V1": 22, "V100003": 23}
THRESHOLDS = {1: (0.25,), 3: (0.25, 0.5, 0.25), 8: (0.0, 0.125, 0.25, 0.3, 0.5, 0.5, 0.75, 1.0)}
TABLE_CASES = [(s, T, B) for s in SHAPES for T, B in ((1, 0), (3, 10), (8, 16))] + [("V2079", 1, 16), ("V2079", 8, 0)]
_LATTICE = {}


def lattice(shape_id):
    """(pred, meas) of a shape on the CPU, flat [S, 2, V]; once"""
    if shape_id not in _LATTICE:
        shape = SHAPES[shape_id]
        _LATTICE[shape_id] = OC.lattice(shape[0], math.prod(shape[2:]), seed=SEEDS[shape_id])
    return _LATTICE[shape_id]


@pytest.mark.parametrize("shape_id,T,B", TABLE_CASES, ids=[f"{s}-T{T}-B{B}" for s, T, B in TABLE_CASES])
def test_table_against_the_torch_restatement(shape_id, T, B):
    from vidar_amd import forecast as FC
    pred, meas = lattice(shape_id)
    th = THRESHOLDS[T]
    if shape_id != "V1":
        assert all(n > 0 for n in OC.on_a_boundary(pred, meas, th))   # floors, min_hits and thresholds are all met exactly
    want = OC.table(pred, meas, th, B)
    shape = SHAPES[shape_id]
    dev = lambda t: t.view(shape).cuda()
    got = FC.occupancy_score(dev(pred), dev(meas), thresholds=th, bins=B)
    again = FC.occupancy_score(dev(pred), dev(meas), thresholds=th, bins=B)
    assert got.shape == (3, OC.columns(T, B)) and got.dtype == torch.float64 and got.is_cuda
    assert torch.equal(got, again)                                    # equal inputs, equal bits
    got = got.cpu()
    counts = [c for c in range(got.shape[1]) if c != 4]
    assert torch.equal(got[:, counts], want[:, counts]), (got - want).abs().max(0)
    print("n_pred, n_meas, n_both, n_occ, brier:", got[:, :5].tolist())
    assert bool(((got[:, 4] - want[:, 4]).abs() <= 1e-12 * want[:, 4]).all())
    if B:
        assert torch.equal(got[:, 5 + 3 * T::2].sum(1), got[:, 2])    # every scored voxel falls in one bin


def test_non_finite_voxels_are_left_out():
    from vidar_amd import forecast as FC
    pred, meas = (t.clone() for t in lattice("V2079"))
    clean = (pred.clone(), meas.clone())
    th, B = THRESHOLDS[3], 10
    spots = []
    for plane in range(4):                                            # hit_p, free_p, hit_m, free_m
        for k, bad in enumerate((math.nan, math.inf, -math.inf)):
            s, v = k, 50 + 300 * plane + 17 * k
            (pred if plane < 2 else meas)[s, plane % 2, v] = bad
            spots.append((s, v))
    for s, v in spots:                                                # the same grids with those voxels emptied: ev == 0
        clean[0][s, :, v] = 0.0
        clean[1][s, :, v] = 0.0
    shape = SHAPES["V2079"]
    got = FC.occupancy_score(pred.view(shape).cuda(), meas.view(shape).cuda(), thresholds=th, bins=B).cpu()
    emptied = FC.occupancy_score(clean[0].view(shape).cuda(), clean[1].view(shape).cuda(), thresholds=th, bins=B).cpu()
    assert bool(torch.isfinite(got).all()) and torch.equal(got, emptied)
    want = OC.table(pred, meas, th, B)
    counts = [c for c in range(got.shape[1]) if c != 4]
    assert torch.equal(got[:, counts], want[:, counts])


def test_bad_arguments_are_errors():
    from vidar_amd import forecast as FC
    g = torch.zeros(2, 2, 4, 5, 6, device="cuda")
    with pytest.raises(ValueError):
        FC.occupancy_score(g, g[:1])
    with pytest.raises(ValueError):
        FC.occupancy_score(g[:, :1], g[:, :1])
    with pytest.raises(TypeError):
        FC.occupancy_score(g.double(), g.double())
    for th in ((), (0.1,) * 9, (0.25, math.nan)):
        with pytest.raises(ValueError):
            FC.occupancy_score(g, g, thresholds=th)
    for bins in (-1, 17):
        with pytest.raises(ValueError):
            FC.occupancy_score(g, g, bins=bins)
    with pytest.raises(ValueError):
        FC.occupancy_score(g, g, min_evidence=math.nan)
    empty = FC.occupancy_score(g[:0], g[:0])
    assert empty.shape == (0, 31) and float(FC.occupancy_score(g, g).abs().sum()) == 0.0
    assert FC.occupancy_score(g[0], g[0]).shape == (31,)


# ---- 2. end to end -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,step", OC.WALL_MARCHES, ids=OC.WALL_IDS)
def test_wall_scene_end_to_end(K, step):
    from vidar_amd import forecast as FC
    from vidar_amd.plugin.dense_heads import ray_ops
    ref = OC.pipeline64(K, step)
    want, border = ref["table"], ref["borderline"]
    # what the metric is for, on the restatement alone
    j = OC.WALL_THRESHOLDS.index(0.25)
    agree, displaced = want[0], want[1]
    brier = [float(r[4] / r[2]) for r in want]
    print(f"restatement: IoU at 0.25 {OC.iou(agree, j):.3f} / {OC.iou(displaced, j):.3f}, brier {brier[0]:.3f} / {brier[1]:.3f}, "
          f"n_both {int(agree[2])} / {int(displaced[2])}, borderline {border.tolist()}")
    assert OC.iou(agree, j) >= 0.5
    assert float(displaced[5 + 3 * j]) == 0.0 and float(displaced[7 + 3 * j]) > 0.0
    assert brier[0] < brier[1]
    assert bool((border.double() <= 0.01 * want[:, 2]).all())

    sigma, origin, pts, tindex = (t.cuda() for t in OC.wall_scene())
    pred = torch.stack(ray_ops.ray_occupancy(sigma, origin, pts, tindex, step, K), 1)
    meas = torch.stack(ray_ops.sweep_evidence(origin, pts, tindex, sigma.shape, step, K), 1)
    got = FC.occupancy_score(pred, meas, thresholds=OC.WALL_THRESHOLDS, bins=10).cpu()
    counts = [c for c in range(got.shape[1]) if c != 4]
    gap = (got - want).abs()
    print(f"device: largest count gap per frame {gap[:, counts].max(1)[0].tolist()}, brier gap {gap[:, 4].tolist()} on "
          f"{want[:, 4].tolist()}")
    assert bool((gap[:, counts] <= border.double().view(2, 1)).all())
    m = FC.occupancy_metrics(got[0], OC.WALL_THRESHOLDS, 10)
    assert m["iou"][j] == pytest.approx(OC.iou(got[0], j)) and m["brier"] == pytest.approx(float(got[0, 4] / got[0, 2]))


# ---- 3. the head and the detector --------------------------------------------------------------------------------------
def _gt_points():
    from vidar_amd.synthetic import make_sample
    _, gt = make_sample(0, rays_per_frame=200, future_frames=6)       # the fixture's sample: its clouds
    return [torch.from_numpy(np.asarray(gt)).float().cuda()]


def test_head_measured_occupancy(small_model, monkeypatch):
    from vidar_amd import deterministic
    from vidar_amd.plugin.dense_heads import ray_ops
    model, metas, feats, pred_dict, cur_metas = small_model
    head = model.future_pred_head
    geom = dict(tgt_bev_h=model.bev_h, tgt_bev_w=model.bev_w, tgt_pc_range=model.point_cloud_range, img_metas=cur_metas)
    gt = _gt_points()
    marched = []                                                      # the arguments the decode hands to ray_argmax
    real = ray_ops.ray_argmax

    def recorded(*a):
        marched.append(a)
        return real(*a)
    monkeypatch.setattr(ray_ops, "ray_argmax", recorded)
    head.get_point_cloud_prediction(pred_dict, gt, 0, **geom)
    monkeypatch.setattr(ray_ops, "ray_argmax", real)
    assert len(marched) == 1
    sigma, origin, pts, tindex, step, K = marched[0]
    with deterministic.use(True):                                     # equal bits need the order-independent sums
        got = head.measured_occupancy(pred_dict, gt, **geom)
        want = torch.stack(ray_ops.sweep_evidence(origin, pts, tindex, sigma.shape, step, K), 1)
    assert got.shape == (1, sigma.shape[0], 2, *sigma.shape[1:]) and torch.equal(got[0], want)
    assert float(got[:, :, 0].sum()) > 0 and float(got[:, :, 1].sum()) > 0


def test_forward_test_carries_the_occupancy_entries(small_model, monkeypatch):
    from vidar_amd import deterministic
    from vidar_amd import evaluate as E
    from vidar_amd import forecast as FC
    from vidar_amd.plugin.dense_heads import ray_ops
    from vidar_amd.plugin.utils import eval_utils
    model, metas, feats, pred_dict, cur_metas = small_model
    head = model.future_pred_head
    geom = dict(tgt_bev_h=model.bev_h, tgt_bev_w=model.bev_w, tgt_pc_range=model.point_cloud_range, img_metas=cur_metas)
    gt = _gt_points()
    th = (0.125, 0.25, 0.5)
    run = lambda: model.forward_test(img_metas=metas, gt_points=gt, img_feats=feats)[0]
    plain_keys = ["absrel_error", "chamfer_distance", "count", "l1_error"]
    results = {}
    monkeypatch.delenv("VIDAR_OCC_METRICS", raising=False)
    try:
        with deterministic.use(True):
            for on_device in (False, True):
                eval_utils.set_device_metrics(on_device)
                eval_utils.set_occupancy_metrics(True, thresholds=th, bins=4)
                results[on_device, True] = run()
                eval_utils.set_occupancy_metrics(False)
                with monkeypatch.context() as mp:                     # off: nothing new is launched
                    for name in ("sweep_evidence", "ray_occupancy"):
                        mp.setattr(ray_ops, name, lambda *a, **k: pytest.fail("launched with the option off"))
                    mp.setattr(FC, "occupancy_score", lambda *a, **k: pytest.fail("launched with the option off"))
                    results[on_device, False] = run()
            table = FC.occupancy_score(head.render_occupancy(pred_dict, end_points=gt, **geom),
                                       head.measured_occupancy(pred_dict, gt, **geom), thresholds=th, bins=4).cpu()
    finally:
        eval_utils.set_device_metrics(None)
        eval_utils.set_occupancy_metrics(None)
    names = FC.occupancy_columns(th, 4)
    assert table.shape == (1, len(results[False, False]), len(names))
    for on_device in (False, True):
        off, on = results[on_device, False], results[on_device, True]
        assert sorted(off) == sorted(on) == [f"frame.{f}" for f in range(table.shape[1])]
        for f, k in enumerate(sorted(off)):
            assert sorted(off[k]) == plain_keys
            assert sorted(on[k]) == sorted(plain_keys + [f"occ.{n}" for n in names])
            assert all(on[k][m] == off[k][m] for m in plain_keys)      # the other entries keep their bits
            assert [on[k][f"occ.{n}"] for n in names] == table[0, f].tolist()
    assert results[True, False].keys() == results[False, False].keys()
    scored = sum(results[False, True][k]["occ.n_both"] for k in results[False, True])
    print(f"voxels scored over the {table.shape[1]} frames: {scored}")
    assert scored > 0
    # the route to the table of tools/test.py
    occ = E.occupancy_summary(E.summarize([results[True, True]]))
    assert sorted(occ) == sorted(results[True, True]) and occ["frame.0"]["thresholds"] == list(th)
    assert occ["frame.0"]["n_both"] == results[True, True]["frame.0"]["occ.n_both"]
