"""GPU: the decode with its confidence (vidar_ray_stats_f32 / vidar_ray_stats_cam_f32, csrc/ray_march.hip ray_stats_body)
and what is built on it (ViDARHeadBase.render_rays / render_cameras(return_stats=True), ViDAR.forecast(stats=...)).

1. the distances are ray_ops.ray_argmax's, bit for bit, skipped and dead rays included;
2. the statistics against the fp64 restatement of tests/ray_stats_cases.py about the DEVICE's own depth, within 4 x the
   error the same restatement makes in fp32 on the CPU (recomputed here, per statistic and per case); dead and skipped rays
   give exactly four zeros;
3. K = 512 through the streamed kernels gives the register form's bits;  4. two runs give equal bits;
5. the camera form equals the listed form on the rays ray_ops.cam_rays writes out;  6. bad arguments are errors;
7. the head and the detector: same sweep and depth with and without the statistics, thresholds, the metre scale.
Shapes: 130 rays in a 2 x 4 x 10 x 96 volume (ray_stats_cases.py), 2 x 3 cameras of 9 x 14 pixels in a 4 x 12 x 14 one."""
import math

import numpy as np
import pytest
import torch

import ray_stats_cases as RC
from forecast_view_cases import camera, volume as cam_volume

pytestmark = pytest.mark.gpu
_DEVICE = {}


def device_run(kind, K, step):
    """(pred, gt, stats) of ray_ops.ray_stats and (pred, gt) of ray_ops.ray_argmax on a case, on the CPU; run once"""
    from vidar_amd.plugin.dense_heads import ray_ops
    key = (kind, K, step)
    if key not in _DEVICE:
        c = RC.case(kind, K, step)
        args = (c.sigma.cuda(), c.origin.cuda(), c.pts.cuda(), c.tindex.cuda(), step, K)
        _DEVICE[key] = tuple(t.cpu() for t in ray_ops.ray_stats(*args) + ray_ops.ray_argmax(*args))
    return _DEVICE[key]


@pytest.mark.parametrize("kind,K,step", RC.CASES, ids=RC.CASE_IDS)
def test_distances_are_the_arg_max_decodes_bits(kind, K, step):
    pred, gt, stats, pred0, gt0 = device_run(kind, K, step)
    assert stats.shape == (RC.R, 4) and stats.dtype == torch.float32
    assert torch.equal(pred, pred0) and torch.equal(gt, gt0)
    assert float(pred[list(RC.SKIPPED)].abs().max()) == 0.0 and float(gt[list(RC.SKIPPED)].abs().max()) == 0.0


@pytest.mark.parametrize("kind,K,step", RC.CASES, ids=RC.CASE_IDS)
def test_statistics_against_fp64_about_the_devices_depth(kind, K, step):
    c = RC.case(kind, K, step)
    pred, _, stats, _, _ = device_run(kind, K, step)
    want, yard = c.yardstick(pred)
    use = c.compared()
    candidates = c.has_live & c.marched
    excluded = int((candidates & ~use).sum())
    err = (stats.double() - want)[use].abs().max(0)[0]
    print(f"rays compared {int(use.sum())}, excluded {excluded}")
    for name, e, y in zip(("p_max", "mean", "rms", "entropy"), err.tolist(), yard.tolist()):
        print(f"  {name:8s} device error {e:.2e}   fp32 restatement error {y:.2e}   ratio {e / y if y else math.inf:.2f}")
    assert excluded <= 0.02 * int(candidates.sum())
    assert bool(torch.isfinite(stats).all())
    dead = ~candidates                                               # skipped, or no live waypoint
    assert int(dead.sum()) >= 2 and float(stats[dead].abs().max()) == 0.0
    assert bool((stats[use][:, 0] > 0).all()) and bool((stats[use][:, 0] <= 1).all()) and bool((stats[use][:, 3] >= 0).all())
    assert bool((err <= 4 * yard).all()), (err.tolist(), yard.tolist())


@pytest.mark.parametrize("kind", RC.VOLUMES)
@pytest.mark.parametrize("step", [1.0, 0.2])
def test_k512_streamed_form_gives_the_register_forms_bits(kind, step):
    from vidar_amd.plugin.dense_heads import ray_ops
    c = RC.case(kind, 512, step)
    args = (c.sigma.cuda(), c.origin.cuda(), c.pts.cuda(), c.tindex.cuda(), step, 512)
    with ray_ops.force_streamed():
        streamed = ray_ops.ray_stats(*args)
    for a, b in zip(streamed, device_run(kind, 512, step)[:3]):
        assert torch.equal(a.cpu(), b)


@pytest.mark.parametrize("K,step", [(512, 0.2), (1026, 0.125)], ids=["K512", "K1026"])
def test_two_runs_give_equal_bits(K, step):
    from vidar_amd.plugin.dense_heads import ray_ops
    c = RC.case("randn", K, step)
    args = (c.sigma.cuda(), c.origin.cuda(), c.pts.cuda(), c.tindex.cuda(), step, K)
    again = ray_ops.ray_stats(*args)
    for a, b in zip(again, device_run("randn", K, step)[:3]):
        assert torch.equal(a.cpu(), b)


# ---- 5. the camera form ------------------------------------------------------------------------------------------------
CAM_GRID = (9, 14, -3.0, -2.5, 2.0, 2.0)                             # Hs, Ws, u0, v0, du, dv: 126 rays per camera


def three_cameras():
    """[2, 3, 4, 4] over the 4 x 12 x 14 volume: looking in from outside, inside it, looking away (every ray misses);
    frame 1: from above a corner, looking away, inside"""
    cams = [[camera((-6.0, 6.3, 2.2), (1.0, 0.05, -0.02)), camera((7.3, 5.6, 1.9), (0.3, 1.0, 0.05)),
             camera((-6.0, 6.3, 2.2), (-1.0, 0.1, 0.0))],
            [camera((-3.0, -4.0, 9.0), (10.0, 10.0, -7.0)), camera((20.0, 6.0, 2.0), (1.0, 0.0, 0.1)),
             camera((5.1, 7.7, 2.4), (-1.0, -0.4, 0.03))]]
    return torch.from_numpy(np.array(cams)).float()


@pytest.mark.parametrize("K,step", [(512, 0.5), (37, 1.0)], ids=["K512-step0.5", "K37-step1.0"])
def test_camera_form_equals_the_listed_form(K, step):
    from vidar_amd.plugin.dense_heads import ray_ops
    Hs, Ws, u0, v0, du, dv = CAM_GRID
    sigma, m = cam_volume(), three_cameras()
    n_f, n_c = m.shape[:2]
    dist, stats = ray_ops.ray_stats_cam(sigma.cuda(), m.cuda(), (Hs, Ws), u0, v0, du, dv, step, K)
    assert dist.shape == (n_f, n_c, Hs, Ws) and stats.shape == (n_f, n_c, Hs, Ws, 4)
    plain = ray_ops.ray_argmax_cam(sigma.cuda(), m.cuda(), (Hs, Ws), u0, v0, du, dv, step, K)
    assert torch.equal(dist, plain)
    origin, pts = ray_ops.cam_rays(m.cuda(), (Hs, Ws), u0, v0, du, dv)
    tindex = torch.arange(n_f, dtype=torch.float32).repeat_interleave(Hs * Ws)
    dist, stats = dist.cpu(), stats.cpu()
    n_live = 0
    for c in range(n_c):
        o, p = origin[:, c].contiguous(), pts[:, c].reshape(-1, 3).contiguous()
        pred, _, listed = ray_ops.ray_stats(sigma.cuda(), o, p, tindex.cuda(), step, K)
        pred0, _ = ray_ops.ray_argmax(sigma.cuda(), o, p, tindex.cuda(), step, K)
        assert torch.equal(pred, pred0)                              # waypoint 0's length on a dead listed ray, as ever
        z, _, _ = RC.logits(sigma, o.cpu(), p.cpu(), tindex, K, step)           # the CPU restatement says which rays live
        live = (z != -math.inf).any(1).view(n_f, Hs, Ws)
        pred, listed = pred.cpu().view(n_f, Hs, Ws), listed.cpu().view(n_f, Hs, Ws, 4)
        assert torch.equal(dist[:, c][live], pred[live]) and torch.equal(stats[:, c][live], listed[live])
        assert bool((dist[:, c][live] > 0).all()) and bool((stats[:, c][live][:, 0] > 0).all())
        for t in (dist[:, c][~live], stats[:, c][~live], listed[~live]):
            assert t.numel() == 0 or float(t.abs().max()) == 0.0
        assert bool((pred[~live] > 0).all())
        n_live += int(live.sum())
        if c == 2:
            assert not bool(live[0].any()) and bool(live[1].all())   # looking away; inside the volume
    assert 0 < n_live < dist.numel()
    print(f"camera rays {dist.numel()}, with a live waypoint {n_live}")


# ---- 6. argument errors ------------------------------------------------------------------------------------------------
def test_bad_arguments_are_errors():
    from vidar_amd.plugin.dense_heads import ray_ops
    c = RC.case("randn", 37, 1.0)
    sigma, origin, pts, tindex = c.sigma.cuda(), c.origin.cuda(), c.pts.cuda(), c.tindex.cuda()
    m = three_cameras().cuda()
    for K in (0, ray_ops.max_k() + 1):
        with pytest.raises(ValueError):
            ray_ops.ray_stats(sigma, origin, pts, tindex, 1.0, K)
        with pytest.raises(ValueError):
            ray_ops.ray_stats_cam(cam_volume().cuda(), m, (9, 14), K=K)
    with pytest.raises(ValueError):
        ray_ops.ray_stats(sigma[:0], origin, pts, tindex, 1.0, 37)                    # F = 0
    with pytest.raises(ValueError):
        ray_ops.ray_stats_cam(cam_volume().cuda()[:0], m[:0], (9, 14))
    for pitch in (dict(du=0.0), dict(dv=0.0)):
        with pytest.raises(ValueError):
            ray_ops.ray_stats_cam(cam_volume().cuda(), m, (9, 14), **pitch)
    with pytest.raises(ValueError):
        ray_ops.ray_stats_cam(cam_volume().cuda(), m[:1], (9, 14))                    # one frame of cameras, two of volume
    none = ray_ops.ray_stats(sigma, origin, pts[:0], tindex[:0], 1.0, 37)             # an empty problem is not an error
    assert [t.shape for t in none] == [(0,), (0,), (0, 4)]
    torch.cuda.synchronize()


# ---- 7. the head and the detector --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_model():
    """the reduced model of tests/test_forecast_view_gpu.py; its no-grad history and future decoder run once"""
    from vidar_amd import train as T
    from vidar_amd.configs import get_config
    from vidar_amd.synthetic import fpn_features, make_sample
    torch.manual_seed(0); np.random.seed(0)
    cfg = get_config("vidar_1_8_nusc_3future", bev_h=24, bev_w=24)
    metas, _ = make_sample(0, rays_per_frame=200, future_frames=6)
    feats = [f.cuda() for f in fpn_features(0, 5, shapes=[(15, 25), (8, 13), (4, 7), (2, 4)])]
    model = T.build_model(cfg).cuda().eval()
    with torch.no_grad():
        pred_dict, cur_metas = model._future_pred_dict([metas], None, feats)
    model._future_pred_dict = lambda img_metas, img=None, img_feats=None: (pred_dict, cur_metas)
    return model, [metas], feats, pred_dict, cur_metas


def test_head_returns_the_statistics_in_metres(small_model, monkeypatch):
    from vidar_amd import forecast as FC
    from vidar_amd.plugin.dense_heads import ray_ops
    model, _, _, pred_dict, cur_metas = small_model
    head = model.future_pred_head
    geom = dict(tgt_bev_h=model.bev_h, tgt_bev_w=model.bev_w, tgt_pc_range=model.point_cloud_range)
    cell = (model.point_cloud_range[3] - model.point_cloud_range[0]) / model.bev_w
    assert abs(cell - 1.0) > 0.5                                      # a scale that shows
    raw = {}                                                          # what the kernels return, in voxel units

    def recorded(name, fn):
        def call(*a, **k):
            raw[name] = fn(*a, **k)
            return raw[name]
        return call
    for name in ("ray_stats", "ray_stats_cam"):
        monkeypatch.setattr(ray_ops, name, recorded(name, getattr(ray_ops, name)))
    rays = FC.lidar_pattern(4, 16).cuda()
    plain = head.render_rays(pred_dict, directions=rays, img_metas=cur_metas, **geom)
    assert not raw                                                    # return_stats=False is the arg-max path
    pts, stats = head.render_rays(pred_dict, directions=rays, img_metas=cur_metas, return_stats=True, **geom)
    assert len(stats) == 1 and len(stats[0]) == len(pts[0]) == 7
    for a, b, s in zip(pts[0], plain[0], stats[0]):
        assert torch.equal(a, b) and s.shape == (a.shape[0], 4)
    got = torch.cat(stats[0])                                         # every ray is kept: frame-major, as they were listed
    want = raw["ray_stats"][2]
    assert got.shape == want.shape == (7 * 64, 4)
    assert torch.equal(got[:, [0, 3]], want[:, [0, 3]])
    torch.testing.assert_close(got[:, 1:3], want[:, 1:3] * cell, rtol=1e-6, atol=0)
    assert float(got[:, 1].max()) > 0

    depth0 = head.render_cameras(pred_dict, cur_metas, cameras=[0, 3], stride=32, **geom)
    depth, dstats = head.render_cameras(pred_dict, cur_metas, cameras=[0, 3], stride=32, return_stats=True, **geom)
    assert torch.equal(depth, depth0) and dstats.shape == (*depth.shape, 4) == (1, 7, 2, 29, 50, 4)
    want = raw["ray_stats_cam"][1]
    assert torch.equal(dstats[0][..., [0, 3]], want[..., [0, 3]])
    torch.testing.assert_close(dstats[0][..., 1:3], want[..., 1:3] * cell, rtol=1e-6, atol=0)
    assert bool(((dstats[..., 0] > 0) == (depth > 0)).all())         # nothing met: zeros in both


def test_forecast_with_statistics_and_thresholds(small_model):
    from vidar_amd import forecast as FC
    model, metas, feats, _, _ = small_model
    rays = FC.lidar_pattern(4, 16)
    call = lambda **kw: model.forecast(img_metas=metas, img_feats=feats, rays=rays, cameras="all", stride=32, **kw)
    plain, full = call(), call(stats=True)
    assert sorted(plain) == ["depth", "sweep", "sweep_index", "valid_frames"]
    assert sorted(full) == ["depth", "depth_stats", "sweep", "sweep_index", "sweep_stats", "valid_frames"]

    def same_sweep(a, b):
        return all(torch.equal(x, y) for k in ("sweep", "sweep_index") for x, y in zip(a[k][0], b[k][0]))
    assert same_sweep(plain, full) and torch.equal(plain["depth"], full["depth"])
    for p, s in zip(full["sweep"][0], full["sweep_stats"][0]):
        assert s.shape == (p.shape[0], 4) and bool(torch.isfinite(s).all())
    assert full["depth_stats"].shape == (*full["depth"].shape, 4)

    nothing = call(min_prob=0.0, max_rms=math.inf)
    assert same_sweep(plain, nothing) and torch.equal(plain["depth"], nothing["depth"])

    p_all = torch.cat([s[:, 0] for s in full["sweep_stats"][0]] + [full["depth_stats"][..., 0].reshape(-1)])
    nobody = call(min_prob=float(p_all.max()) + 1e-3)
    assert all(p.shape == (0, 3) and i.numel() == 0 for p, i in zip(nobody["sweep"][0], nobody["sweep_index"][0]))
    assert float(nobody["depth"].abs().max()) == 0.0 and float(plain["depth"].max()) > 0.0

    p_mid = float(torch.cat([s[:, 0] for s in full["sweep_stats"][0]]).median())
    r_mid = float(torch.cat([s[:, 2] for s in full["sweep_stats"][0]]).median())
    mid = call(min_prob=p_mid, max_rms=r_mid)
    kept = 0
    for f in range(7):
        sel = FC.confidence_mask(full["sweep_stats"][0][f], p_mid, r_mid)
        assert torch.equal(mid["sweep_index"][0][f], full["sweep_index"][0][f][sel])
        assert torch.equal(mid["sweep"][0][f], full["sweep"][0][f][sel])
        assert torch.equal(mid["sweep_stats"][0][f], full["sweep_stats"][0][f][sel])
        kept += int(sel.sum())
    total = sum(p.shape[0] for p in full["sweep"][0])
    assert 0 < kept < total
    sel = FC.confidence_mask(full["depth_stats"], p_mid, r_mid)
    assert torch.equal(mid["depth"], torch.where(sel, full["depth"], torch.zeros_like(full["depth"])))
    assert torch.equal(mid["depth_stats"], full["depth_stats"])       # the statistics themselves are not thinned
    print(f"sweep rays {total}, kept at p_max >= {p_mid:.3f} and rms <= {r_mid:.2f} m: {kept}; "
          f"pixels with a return {int((full['depth'] > 0).sum())}, kept {int((mid['depth'] > 0).sum())}")
