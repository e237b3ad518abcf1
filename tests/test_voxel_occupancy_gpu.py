"""GPU: the occupancy query at listed points and at every voxel's centre (vidar_point_occupancy_f32 /
vidar_voxel_occupancy_f32, csrc/ray_march.hip point_occupancy_body) and what is built on it (ViDARHeadBase.occupancy_at /
render_occupancy_dense, ViDAR.forecast(occupancy="dense"), eval_utils.set_occupancy_metrics(source="dense")).

1. the listed form against the fp64 restatement of tests/voxel_occupancy_cases.py, within 4 x the error the same
   restatement makes in fp32 on the CPU (recomputed here, per output, case and extent); extents 0.3, 1.0, 2.5;
2. the dense form likewise, on all 7 680 voxels of every case;
3. the dense form equals the listed form on the materialised voxel centres, bit for bit, and K = 512 through the streamed
   kernels gives the register form's bits for both;
4. a small, awkward volume: 45 rays, an origin exactly at a voxel's centre, one outside, K = 5;
5. ranges, and exact zeros beyond the marched range;  6. equal bits run after run and under the deterministic mode;
7. the head (both classes) and the detector.
Shapes: a 2 x 4 x 10 x 96 volume with 130 listed rays (ray_stats_cases.py), a 3 x 1 x 3 x 5 one, the 24 x 24 BEV model."""
import math

import numpy as np
import pytest
import torch

import head_route_cases as HR
import ray_stats_cases as RS
import voxel_occupancy_cases as VC

pytestmark = pytest.mark.gpu
_POINT, _DENSE = {}, {}


def ops():
    from vidar_amd.plugin.dense_heads import ray_ops
    return ray_ops


def device_point(kind, K, step, extent):
    key = (kind, K, step, extent)
    if key not in _POINT:
        q = VC.listed(kind, K, step)
        _POINT[key] = ops().point_occupancy(RS.volume(kind).cuda(), q.origin.cuda(), q.pts.cuda(), q.tindex.cuda(), step, K,
                                            extent).cpu()
    return _POINT[key]


def device_dense(kind, K, step):
    """(hit, free) [F, Z, Y, X] of ray_ops.voxel_occupancy at extent 1.0, on the CPU; run once"""
    key = (kind, K, step)
    if key not in _DENSE:
        _DENSE[key] = tuple(t.cpu() for t in ops().voxel_occupancy(RS.volume(kind).cuda(), RS.rays()[0].cuda(), step, K))
    return _DENSE[key]


def held_to_the_yardstick(got, q, extent, what):
    """got [R, 2] against q's fp64 answers on the compared queries: 4 x the fp32 restatement's own error, per output"""
    use, yard = q.compared(), q.yardstick(extent)
    err = (got.double() - q.want64[extent])[use].abs().max(0)[0].tolist()
    for name, e, y in zip(("hit", "free"), err, yard):
        print(f"  {what} extent {extent}: {name:4s} device error {e:.2e}   fp32 restatement error {y:.2e}   "
              f"ratio {e / y if y else math.inf:.2f}")
    dead = ~q.candidates()                                            # skipped, or no live waypoint
    assert got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    assert int(dead.sum()) == 0 or float(got[dead].abs().max()) == 0.0
    assert all(e <= 4 * y for e, y in zip(err, yard)), (what, extent, err, yard)


# ---- 1. / 2. against the fp64 restatement -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,K,step", VC.CASES, ids=VC.CASE_IDS)
def test_point_form_against_fp64(kind, K, step):
    q = VC.listed(kind, K, step)
    print(f"rays compared {int(q.compared().sum())}, excluded {q.excluded()}")
    assert q.excluded() <= VC.MAX_EXCLUDED_RAYS and int((~q.candidates()).sum()) >= 2
    for extent in VC.EXTENTS:
        got = device_point(kind, K, step, extent)
        assert got.shape == (RS.R, 2)
        held_to_the_yardstick(got, q, extent, "listed")
        assert float(got[list(RS.SKIPPED)].abs().max()) == 0.0


@pytest.mark.parametrize("kind,K,step", VC.CASES, ids=VC.CASE_IDS)
def test_dense_form_against_fp64(kind, K, step):
    q = VC.dense(kind, K, step)
    hit, free = device_dense(kind, K, step)
    assert hit.shape == free.shape == (RS.F_, RS.Z, RS.Y, RS.X)
    print(f"voxels compared {int(q.compared().sum())}, excluded {q.excluded()}")
    assert q.excluded() <= VC.MAX_EXCLUDED_VOXELS * hit.numel()
    held_to_the_yardstick(torch.stack([hit.reshape(-1), free.reshape(-1)], 1), q, 1.0, "dense")


# ---- 3. one body, two sources, two K forms -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["randn", "plane"])
@pytest.mark.parametrize("K,step", [(512, 1.0), (37, 1.0), (1026, 0.125)], ids=["K512", "K37", "K1026"])
def test_dense_form_equals_the_point_form_on_the_voxel_centres(kind, K, step):
    sigma, origin = RS.volume(kind).cuda(), RS.rays()[0].cuda()
    pts, tindex = (t.cuda() for t in VC.voxel_centres(sigma.shape))
    for extent in (0.3, 1.0):
        hit, free = ops().voxel_occupancy(sigma, origin, step, K, extent)
        listed = ops().point_occupancy(sigma, origin, pts, tindex, step, K, extent)
        assert torch.equal(torch.stack([hit.reshape(-1), free.reshape(-1)], 1), listed) and float(listed.max()) > 0
        if K == 512:
            with ops().force_streamed():
                s_hit, s_free = ops().voxel_occupancy(sigma, origin, step, K, extent)
                s_listed = ops().point_occupancy(sigma, origin, pts, tindex, step, K, extent)
            assert torch.equal(s_hit, hit) and torch.equal(s_free, free) and torch.equal(s_listed, listed)
    assert torch.equal(hit.cpu(), device_dense(kind, K, step)[0])     # the default extent is 1.0


# ---- 4. small and awkward ----------------------------------------------------------------------------------------------
def test_small_volume_awkward_origins():
    """[3, 1, 3, 5]: 45 rays, no multiple of the 4 rays of a workgroup.  Frame 0's origin sits exactly at the centre of
    voxel (z 0, y 1, x 2); frame 1's lies outside, so far that part of its rays has no live waypoint within K = 5 steps of 1;
    frame 2's lies inside.  Most voxels are further than K step from their origin."""
    K, step = 5, 1.0
    sigma = torch.randn(3, 1, 3, 5, generator=torch.Generator().manual_seed(5)) * 2
    origin = torch.tensor([[2.5, 1.5, 0.5], [-4.95, 1.4, 0.5], [0.7, 2.2, 0.4]])
    pts, tindex = VC.voxel_centres(sigma.shape)
    q = VC.Queries(sigma, origin, pts, tindex, K, step, (1.0,))
    dead = ~q.has_live
    print(f"dead per frame {[int(dead[f * 15:(f + 1) * 15].sum()) for f in range(3)]}, excluded {q.excluded()}, "
          f"beyond K step {int((q.L64 - 0.5 >= K * step).sum())}")
    assert bool(dead[7]) and int(dead[:15].sum()) == 1                # the voxel at the origin, and only that one
    assert 0 < int(dead[15:30].sum()) < 15 and int(dead[30:].sum()) == 0
    assert q.excluded() == 0
    hit, free = ops().voxel_occupancy(sigma.cuda(), origin.cuda(), step, K)
    got = torch.stack([hit.reshape(-1), free.reshape(-1)], 1).cpu()
    held_to_the_yardstick(got, q, 1.0, "small")
    assert float(got[7].abs().max()) == 0.0 and float(got[dead].abs().max()) == 0.0
    assert float(got[q.L64 - 0.5 >= K * step].abs().max()) == 0.0 and float(got.max()) > 0.1
    # the listed form on the same end points, with two rows skipped
    t2 = tindex.clone()
    t2[3], t2[20] = -1.0, 3.0
    listed = ops().point_occupancy(sigma.cuda(), origin.cuda(), pts.cuda(), t2.cuda(), step, K).cpu()
    keep = torch.ones(45, dtype=torch.bool)
    keep[[3, 20]] = False
    assert torch.equal(listed[keep], got[keep]) and float(listed[[3, 20]].abs().max()) == 0.0
    assert float(got[3].max()) > 0 or float(got[20].max()) > 0        # they were not zero rows anyway
    # empty problems
    assert ops().point_occupancy(sigma.cuda(), origin.cuda(), pts[:0].cuda(), tindex[:0].cuda(), step, K).shape == (0, 2)


def test_bad_arguments_are_errors():
    sigma, origin = RS.volume("randn").cuda(), RS.rays()[0].cuda()
    _, pts, tindex = (t.cuda() for t in RS.rays())
    for kw in (dict(K=0), dict(K=ops().max_k() + 1), dict(extent=0.0), dict(extent=-1.0), dict(extent=float("nan")),
               dict(extent=float("inf"))):
        with pytest.raises(ValueError):
            ops().point_occupancy(sigma, origin, pts, tindex, **dict(dict(step=1.0, K=37), **kw))
        with pytest.raises(ValueError):
            ops().voxel_occupancy(sigma, origin, **dict(dict(step=1.0, K=37), **kw))
    with pytest.raises(ValueError):
        ops().voxel_occupancy(sigma, origin[:1], 1.0, 37)             # one origin, two frames
    torch.cuda.synchronize()


# ---- 5. ranges ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", RS.VOLUMES)
def test_ranges_and_exact_zeros_beyond_the_marched_range(kind):
    K, step = 37, 1.0
    q = VC.dense(kind, K, step)
    assert float(((q.L64 - 0.5) - K * step).abs().min()) > 1e-4       # no voxel sits on the boundary: fp32 and fp64 agree
    beyond = (q.L64 - 0.5 >= K * step).view(RS.F_, RS.Z, RS.Y, RS.X)
    assert 0.55 < float(beyond.float().mean()) < 0.61                 # 58 % of the voxels
    hit, free = device_dense(kind, K, step)
    assert float(hit[beyond].abs().max()) == 0.0 and float(free[beyond].abs().max()) == 0.0
    for k, s in RS.MARCHES:
        hit, free = device_dense(kind, k, s)
        assert float(hit.min()) >= 0.0 and float(free.min()) >= 0.0 and float((hit + free).max()) <= 1 + 1e-5
        assert float((hit + free).max()) > 0.5


# ---- 6. no atomics -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,step", [(512, 0.2), (1026, 0.125)], ids=["K512", "K1026"])
def test_equal_bits_run_after_run_and_in_the_deterministic_mode(K, step):
    from vidar_amd import deterministic
    sigma, origin = RS.volume("randn").cuda(), RS.rays()[0].cuda()
    _, pts, tindex = (t.cuda() for t in RS.rays())
    dense0, point0 = device_dense("randn", K, step), device_point("randn", K, step, 1.0)
    for _ in range(2):                                                # the cached run was the first of three
        again = ops().voxel_occupancy(sigma, origin, step, K)
        assert torch.equal(again[0].cpu(), dense0[0]) and torch.equal(again[1].cpu(), dense0[1])
        assert torch.equal(ops().point_occupancy(sigma, origin, pts, tindex, step, K).cpu(), point0)
    with deterministic.use(True):
        det = ops().voxel_occupancy(sigma, origin, step, K)
        assert torch.equal(det[0].cpu(), dense0[0]) and torch.equal(det[1].cpu(), dense0[1])
        assert torch.equal(ops().point_occupancy(sigma, origin, pts, tindex, step, K).cpu(), point0)


# ---- 7. the head and the detector --------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", HR.CLASSES)
def test_head_routes_are_the_ops_on_the_decodes_rays(cls, monkeypatch):
    """the tiny heads of tests/head_route_cases.py: render_occupancy_dense is ray_ops.voxel_occupancy on the volumes and
    origins the decode marches, occupancy_at(points=gt_points) ray_ops.point_occupancy on the decode's own rays"""
    K = 37
    head = HR.build_head(cls, K).cuda()
    pred_dict, gt = HR.to("cuda", HR.pred_dict(head)), HR.to("cuda", HR.clouds(head))
    kw = dict(HR.geom(head), img_metas=HR.metas())
    if cls == "ViDARHeadBase":
        kw["batched_origin_points"] = HR.origin_points().cuda()
    marched = []                                                      # the arguments the decode hands to ray_argmax
    real = ops().ray_argmax

    def recorded(*a):
        marched.append(a)
        return real(*a)
    monkeypatch.setattr(ops(), "ray_argmax", recorded)
    head.get_point_cloud_prediction(pred_dict, gt, 0, *HR.geom(head).values(),
                                    **{k: v for k, v in kw.items() if not k.startswith("tgt_")})
    monkeypatch.setattr(ops(), "ray_argmax", real)
    assert len(marched) == HR.BS
    dense = head.render_occupancy_dense(pred_dict, **kw)
    wide = head.render_occupancy_dense(pred_dict, extent=2.5, **kw)
    at = head.occupancy_at(pred_dict, gt, **kw)
    at_wide = head.occupancy_at(pred_dict, gt, extent=2.5, **kw)
    assert dense.shape == (HR.BS, HR.F_, 2, HR.Z, HR.H, HR.W) and len(at) == HR.BS
    for b, (sigma, origin, pts, tindex, step, k) in enumerate(marched):
        assert k == K
        assert torch.equal(dense[b], torch.stack(ops().voxel_occupancy(sigma, origin, step, k), 1))
        assert torch.equal(wide[b], torch.stack(ops().voxel_occupancy(sigma, origin, step, k, 2.5), 1))
        n = gt[b].shape[0]
        assert at[b].shape == (n, 2)
        assert torch.equal(at[b], ops().point_occupancy(sigma, origin, pts, tindex, step, k)[:n])
        assert torch.equal(at_wide[b], ops().point_occupancy(sigma, origin, pts, tindex, step, k, 2.5)[:n])
        undecoded = torch.arange(n, device="cuda") % 5 == 0          # every fifth point belongs to no decoded frame
        assert float(at[b][undecoded].abs().max()) == 0.0 and float(at[b].max()) > 0
    assert bool(torch.isfinite(dense).all()) and float(dense.sum(2).max()) <= 1 + 1e-5 and not torch.equal(dense, wide)


@pytest.fixture(scope="module")
def small_model():
    """the reduced model of tests/test_forecast_view_gpu.py; its no-grad history and future decoder run once"""
    from vidar_amd import train as T
    from vidar_amd.configs import get_config
    from vidar_amd.synthetic import fpn_features, make_sample
    torch.manual_seed(0); np.random.seed(0)
    cfg = get_config("vidar_1_8_nusc_3future", bev_h=24, bev_w=24)
    metas, gt = make_sample(0, rays_per_frame=200, future_frames=6)
    feats = [f.cuda() for f in fpn_features(0, 5, shapes=[(15, 25), (8, 13), (4, 7), (2, 4)])]
    model = T.build_model(cfg).cuda().eval()
    with torch.no_grad():
        pred_dict, cur_metas = model._future_pred_dict([metas], None, feats)
    model._future_pred_dict = lambda img_metas, img=None, img_feats=None: (pred_dict, cur_metas)
    return model, [metas], feats, pred_dict, cur_metas, [torch.from_numpy(np.asarray(gt)).float().cuda()]


def test_forecast_dense(small_model, monkeypatch):
    from vidar_amd import forecast as FC
    model, metas, feats, pred_dict, cur_metas, _ = small_model
    head = model.future_pred_head
    geom = dict(tgt_bev_h=model.bev_h, tgt_bev_w=model.bev_w, tgt_pc_range=model.point_cloud_range)
    want = head.render_occupancy_dense(pred_dict, img_metas=cur_metas, **geom)
    out = model.forecast(img_metas=metas, img_feats=feats, occupancy="dense")        # neither rays nor cameras
    assert sorted(out) == ["evidence", "occupancy", "valid_frames"]
    Z = want.shape[3]
    assert want.shape == (1, 7, 2, Z, model.bev_h, model.bev_w) and torch.equal(out["evidence"], want)
    ev, occ = want.sum(2), out["occupancy"]
    assert occ.shape == (1, 7, Z, model.bev_h, model.bev_w)
    unseen = ev < 0.5
    assert torch.equal(torch.isnan(occ), unseen) and 0 < int(unseen.sum()) < unseen.numel()
    assert torch.equal(occ[~unseen], (want[:, :, 0] / ev)[~unseen])
    assert float(want.min()) >= 0.0 and float(ev.max()) <= 1 + 1e-5
    low = model.forecast(img_metas=metas, img_feats=feats, occupancy="dense", min_evidence=0.05)
    assert torch.equal(torch.isnan(low["occupancy"]), ev < 0.05) and int((ev < 0.05).sum()) < int(unseen.sum())
    # next to a sweep: the sweep keeps its bits, and the sweep's own grid sees fewer voxels
    rays = FC.lidar_pattern(4, 16)
    plain = model.forecast(img_metas=metas, img_feats=feats, rays=rays)
    both = model.forecast(img_metas=metas, img_feats=feats, rays=rays, occupancy="dense")
    assert all(torch.equal(a, b) for a, b in zip(both["sweep"][0], plain["sweep"][0]))
    assert torch.equal(both["evidence"], want)
    sweep = model.forecast(img_metas=metas, img_feats=feats, rays=rays, occupancy="sweep")
    seen_sweep, seen_dense = int((~torch.isnan(sweep["occupancy"])).sum()), int((~unseen).sum())
    print(f"voxels with an answer: 64-ray sweep {seen_sweep}, dense {seen_dense} of {unseen.numel()}")
    assert seen_dense > seen_sweep
    # without the option nothing new is launched
    with monkeypatch.context() as mp:
        for name in ("voxel_occupancy", "point_occupancy"):
            mp.setattr(ops(), name, lambda *a, **k: pytest.fail("launched without the option"))
        model.forecast(img_metas=metas, img_feats=feats, rays=rays, occupancy="sweep")
    with pytest.raises(ValueError):
        model.forecast(img_metas=metas, img_feats=feats, occupancy="voxels")


def test_forward_test_scores_the_dense_grid(small_model, monkeypatch):
    from vidar_amd import deterministic
    from vidar_amd.plugin.utils import eval_utils
    model, metas, feats, pred_dict, cur_metas, gt = small_model
    run = lambda: model.forward_test(img_metas=metas, gt_points=gt, img_feats=feats)[0]
    monkeypatch.delenv("VIDAR_OCC_METRICS", raising=False)
    try:
        with deterministic.use(True):                                 # the rays source sums with atomics otherwise
            eval_utils.set_occupancy_metrics(True, thresholds=(0.25,), bins=4)
            with monkeypatch.context() as mp:                         # the default source launches nothing new
                mp.setattr(ops(), "voxel_occupancy", lambda *a, **k: pytest.fail("launched under source='rays'"))
                rays = run()
            eval_utils.set_occupancy_metrics(True, source="dense", thresholds=(0.25,), bins=4)
            dense = run()
            eval_utils.set_occupancy_metrics(False)
            off = run()
    finally:
        eval_utils.set_occupancy_metrics(None)
    assert sorted(rays) == sorted(dense) == sorted(off) == [f"frame.{f}" for f in range(7)]
    for f in range(7):
        r, d, o = rays[f"frame.{f}"], dense[f"frame.{f}"], off[f"frame.{f}"]
        assert sorted(r) == sorted(d) and "occ.n_pred" in d and not any(k.startswith("occ.") for k in o)
        same = lambda a, b: a == b or (math.isnan(a) and math.isnan(b))
        assert all(same(d[k], o[k]) and same(r[k], o[k]) for k in o)  # the other metrics keep their values
        assert d["occ.n_meas"] == r["occ.n_meas"]                     # the measured side is untouched
        print(f"frame {f}: n_pred rays {r['occ.n_pred']:.0f} dense {d['occ.n_pred']:.0f}, n_both rays {r['occ.n_both']:.0f} "
              f"dense {d['occ.n_both']:.0f} of n_meas {d['occ.n_meas']:.0f}")
        assert d["occ.n_pred"] >= r["occ.n_pred"] and d["occ.n_pred"] > 0
