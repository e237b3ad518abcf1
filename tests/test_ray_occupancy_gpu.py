"""GPU: occupancy evidence of the decode's softmax (vidar_ray_occupancy_f32 / vidar_ray_occupancy_cam_f32,
csrc/ray_march.hip ray_occupancy_body) and what is built on it (ViDARHeadBase.render_occupancy,
ViDAR.forecast(occupancy=...)).

1. parity: all 18 cases of tests/ray_occupancy_cases.py, both outputs, both modes, against the fp64 restatement; per case
   and output the max abs error over the voxels is held to 4 x the fp32 restatement's own error (recomputed here; the
   deterministic mode adds its own bound); finite, >= 0; all rays skipped and R = 0 give exact zeros;
2. the deterministic mode: equal bits over runs, over a permutation of the rays and over the two K forms;
3. the camera form against the listed form on the rays ray_ops.cam_rays writes out;
4. bad arguments are errors;  5. the head and the detector.
Shapes: 130 rays in a 2 x 4 x 10 x 96 volume (ray_stats_cases.py), 2 x 3 cameras of 9 x 14 pixels in a 4 x 12 x 14 one."""
import math

import numpy as np
import pytest
import torch

import ray_occupancy_cases as RO
import ray_stats_cases as RC
from forecast_view_cases import volume as cam_volume
from test_ray_stats_gpu import CAM_GRID, three_cameras

pytestmark = pytest.mark.gpu
NAMES = ("hit", "free")
_DEVICE = {}


def device_run(kind, K, step, det):
    """(hit, free) of ray_ops.ray_occupancy on a case in the default (det False) or deterministic mode, on the CPU; once"""
    from vidar_amd import deterministic
    from vidar_amd.plugin.dense_heads import ray_ops
    key = (kind, K, step, det)
    if key not in _DEVICE:
        c = RO.case(kind, K, step)
        with deterministic.use(det):
            out = ray_ops.ray_occupancy(c.sigma.cuda(), c.origin.cuda(), c.pts.cuda(), c.tindex.cuda(), step, K)
        _DEVICE[key] = tuple(t.cpu() for t in out)
    return _DEVICE[key]


def det_bound(c, want, M):
    """the deterministic mode's own error per voxel (det_acc.h): M 2^(2h - 62) + 2^-23 |want|, h from the call's
    contribution bound R K 8, M >= the largest contribution"""
    h = math.ceil(math.log2(RC.R * c.K * 8))
    return M * 2.0 ** (2 * h - 62) + 2.0 ** -23 * want.abs()


@pytest.mark.parametrize("kind,K,step", RO.CASES, ids=RO.CASE_IDS)
def test_parity_with_the_fp64_restatement(kind, K, step):
    c = RO.case(kind, K, step)
    yard = c.yardstick()
    touched = int(((c.want64[0] + c.want64[1]) > 0).sum())
    print(f"voxels touched {touched} of {c.want64[0].numel()}")
    failures = []
    for det in (False, True):
        got = device_run(kind, K, step, det)
        for name, g, want, y, w in zip(NAMES, got, c.want64, yard, (c.p64, c.b64)):
            assert g.shape == c.sigma.shape and g.dtype == torch.float32
            assert bool(torch.isfinite(g).all()) and float(g.min()) >= 0.0
            err = (g.double() - want).abs()
            print(f"  {'deterministic' if det else 'default':13s} {name:4s} device error {float(err.max()):.2e}   "
                  f"fp32 restatement error {y:.2e}   ratio {float(err.max()) / y if y else math.inf:.2f}   "
                  f"largest value {float(want.max()):.1f}")
            allowed = 4 * y + (det_bound(c, want, float(w.max())) if det else 0.0)
            if not bool((err <= allowed).all()):
                failures.append((det, name, float(err.max()), y))
    assert not failures, failures


def test_skipped_rays_and_no_rays_give_exact_zeros():
    from vidar_amd import deterministic
    from vidar_amd.plugin.dense_heads import ray_ops
    c = RO.case("randn", 65, 0.25)
    sigma, origin, pts = c.sigma.cuda(), c.origin.cuda(), c.pts.cuda()
    skipped = torch.where(torch.arange(RC.R) % 2 == 0, torch.tensor(-1.0), torch.tensor(float(RC.F_))).cuda()
    skipped[3] = float("nan")
    for det in (False, True):
        with deterministic.use(det):
            for K, step in ((65, 0.25), (512, 1.0)):
                for out in (ray_ops.ray_occupancy(sigma, origin, pts, skipped, step, K),
                            ray_ops.ray_occupancy(sigma, origin, pts[:0], skipped[:0], step, K)):
                    for g in out:
                        assert g.shape == sigma.shape and float(g.abs().max()) == 0.0


# ---- 2. the deterministic mode -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,step", [(512, 0.2), (1026, 0.125)], ids=["K512", "K1026"])
def test_deterministic_mode_gives_equal_bits(K, step):
    from vidar_amd import deterministic
    from vidar_amd.plugin.dense_heads import ray_ops
    c = RO.case("randn", K, step)
    first = device_run("randn", K, step, True)
    sigma, origin, pts, tindex = c.sigma.cuda(), c.origin.cuda(), c.pts.cuda(), c.tindex.cuda()
    perm = torch.randperm(RC.R, generator=torch.Generator().manual_seed(5)).cuda()
    with deterministic.use(True):
        again = ray_ops.ray_occupancy(sigma, origin, pts, tindex, step, K)
        shuffled = ray_ops.ray_occupancy(sigma, origin, pts[perm].contiguous(), tindex[perm].contiguous(), step, K)
        with ray_ops.force_streamed():
            streamed = ray_ops.ray_occupancy(sigma, origin, pts, tindex, step, K)
    for a, b, s, f in zip(again, shuffled, streamed, first):
        assert torch.equal(a.cpu(), f) and torch.equal(b.cpu(), f)
        assert torch.equal(s.cpu(), f)                                # K = 512: the streamed form's bits
    # the default mode stays within the parity test's bound (4 x yardstick + the mode's own) of the deterministic one
    yard = c.yardstick()
    for name, d, f, want, y, w in zip(NAMES, device_run("randn", K, step, False), first, c.want64, yard, (c.p64, c.b64)):
        gap = (d.double() - f.double()).abs()
        allowed = 4 * y + det_bound(c, want, float(w.max()))
        print(f"  {name:4s} default against deterministic: max gap {float(gap.max()):.2e}, allowed at least {4 * y:.2e}")
        assert bool((gap <= allowed).all())


# ---- 3. the camera form ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,step", [(512, 0.5), (37, 1.0)], ids=["K512-step0.5", "K37-step1.0"])
def test_camera_form_against_the_listed_form(K, step):
    from vidar_amd import deterministic
    from vidar_amd.plugin.dense_heads import ray_ops
    Hs, Ws, u0, v0, du, dv = CAM_GRID
    sigma, m = cam_volume(), three_cameras()
    n_f, n_c = m.shape[:2]
    grid = ((Hs, Ws), u0, v0, du, dv, step, K)
    origin, pts = ray_ops.cam_rays(m.cuda(), (Hs, Ws), u0, v0, du, dv)
    tindex = torch.arange(n_f, dtype=torch.float32).repeat_interleave(Hs * Ws)
    with deterministic.use(True):
        fused = [t.cpu().double() for t in ray_ops.ray_occupancy_cam(sigma.cuda(), m.cuda(), *grid)]
        listed = [[t.cpu().double() for t in ray_ops.ray_occupancy(
            sigma.cuda(), origin[:, c].contiguous(), pts[:, c].reshape(-1, 3).contiguous(), tindex.cuda(), step, K)]
            for c in range(n_c)]
        away = ray_ops.ray_occupancy_cam(sigma.cuda(), m[:, 2:3].cuda(), *grid)
    default = [t.cpu().double() for t in ray_ops.ray_occupancy_cam(sigma.cuda(), m.cuda(), *grid)]
    for g in away:
        assert float(g[0].abs().max()) == 0.0 and float(g[1].abs().max()) > 0.0   # frame 0: looking away; frame 1: inside
    # the CPU restatement on the rays written out, camera by camera; the number of terms of every voxel's sum
    want64, want32, n_v = [0.0, 0.0], [0.0, 0.0], 0
    for c in range(n_c):
        rays = (origin[:, c].cpu(), pts[:, c].reshape(-1, 3).cpu(), tindex, K, step)
        for v, (a, b) in enumerate(zip(RO.occupancy(sigma.double(), *rays), RO.occupancy(sigma, *rays))):
            want64[v] = want64[v] + a
            want32[v] = want32[v] + b.double()
        z, _, _ = RC.logits(sigma.double(), *rays)
        n_v = n_v + RO.counts(sigma.shape, *rays[:3], K, step, z != -math.inf)
    # one fixed-point call against three: each result is its exact sum within N_v delta / 2 (delta <= 2^(h - 61) as no
    # contribution exceeds 1; 16 more terms for waypoints whose fp32 cell differs from the fp64 one) and one fp32 rounding
    h_fused = math.ceil(math.log2(n_f * n_c * Hs * Ws * K * 8))
    h_listed = math.ceil(math.log2(n_f * Hs * Ws * K * 8))
    for v, name in enumerate(NAMES):
        total = sum(per[v] for per in listed)
        size = fused[v].abs() + sum(per[v].abs() for per in listed)
        tol = 2.0 ** -24 * size + (n_v + 16).double() * (2.0 ** (h_fused - 62) + n_c * 2.0 ** (h_listed - 62))
        gap = (fused[v] - total).abs()
        print(f"  {name:4s} fused against the listed form: max gap {float(gap.max()):.2e}, exact on "
              f"{int((gap == 0).sum())} of {gap.numel()} voxels; largest value {float(total.max()):.2f}")
        assert bool((gap <= tol).all())
        assert bool(((total == 0) == (fused[v] == 0)).all()) and float(total.max()) > 0
        yard = float((want32[v] - want64[v]).abs().max())
        err = float((default[v] - want64[v]).abs().max())
        print(f"  {name:4s} default mode: device error {err:.2e}   fp32 restatement error {yard:.2e}   "
              f"ratio {err / yard if yard else math.inf:.2f}")
        assert err <= 4 * yard and float(default[v].min()) >= 0.0


# ---- 4. argument errors ------------------------------------------------------------------------------------------------
def test_bad_arguments_are_errors():
    from vidar_amd import deterministic
    from vidar_amd._lib import BAD_ARG, lib, ptr, stream_of
    from vidar_amd.plugin.dense_heads import ray_ops
    c = RO.case("randn", 37, 1.0)
    sigma, origin, pts, tindex = c.sigma.cuda(), c.origin.cuda(), c.pts.cuda(), c.tindex.cuda()
    m = three_cameras().cuda()
    for K in (0, ray_ops.max_k() + 1):
        with pytest.raises(ValueError):
            ray_ops.ray_occupancy(sigma, origin, pts, tindex, 1.0, K)
        with pytest.raises(ValueError):
            ray_ops.ray_occupancy_cam(cam_volume().cuda(), m, (9, 14), K=K)
    with pytest.raises(ValueError):
        ray_ops.ray_occupancy_cam(cam_volume().cuda(), m[:1], (9, 14))                # one frame of cameras, two of volume
    for pitch in (dict(du=0.0), dict(dv=0.0)):
        with pytest.raises(ValueError):
            ray_ops.ray_occupancy_cam(cam_volume().cuda(), m, (9, 14), **pitch)
    hit, free = torch.full_like(sigma, 7.0), torch.full_like(sigma, 7.0)
    with deterministic.use(True):
        deterministic.sync()
        need = ray_ops.occupancy_workspace_bytes(*sigma.shape)
        assert need == 8 * (2 * sigma.numel() + 2)
        small = torch.empty(need - 8, dtype=torch.uint8, device="cuda")
        for wsp, wsn in ((None, 0), (ptr(small), need - 8)):
            rc = lib().vidar_ray_occupancy_f32(ptr(sigma), ptr(origin), ptr(pts), ptr(tindex), ptr(hit), ptr(free),
                                               *sigma.shape[:1], RC.R, *sigma.shape[1:], 37, 1.0, wsp, wsn,
                                               stream_of(sigma))
            assert rc == BAD_ARG
    torch.cuda.synchronize()
    assert float(hit.min()) == 7.0 and float(free.min()) == 7.0       # nothing was launched, nothing zeroed
    assert ray_ops.occupancy_workspace_bytes(*sigma.shape) == 4 * 8 * 2 * sigma.numel()


# ---- 5. the head and the detector --------------------------------------------------------------------------------------
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


def test_head_and_detector(small_model, monkeypatch):
    from vidar_amd import deterministic
    from vidar_amd import forecast as FC
    from vidar_amd.plugin.dense_heads import ray_ops
    model, metas, feats, pred_dict, cur_metas = small_model
    head = model.future_pred_head
    geom = dict(tgt_bev_h=model.bev_h, tgt_bev_w=model.bev_w, tgt_pc_range=model.point_cloud_range)
    rays = FC.lidar_pattern(4, 16)
    marched = []                                                      # the arguments render_rays hands to ray_argmax

    def recorded(*a):
        marched.append(a)
        return real(*a)
    real = ray_ops.ray_argmax
    monkeypatch.setattr(ray_ops, "ray_argmax", recorded)
    head.render_rays(pred_dict, directions=rays.cuda(), img_metas=cur_metas, **geom)
    monkeypatch.setattr(ray_ops, "ray_argmax", real)
    assert len(marched) == 1
    with deterministic.use(True):                                     # equal bits need the order-independent sums
        sweep = head.render_occupancy(pred_dict, directions=rays.cuda(), img_metas=cur_metas, **geom)
        want = torch.stack(ray_ops.ray_occupancy(*marched[0]), 1)
        cams = head.render_occupancy(pred_dict, cameras="all", stride=32, img_metas=cur_metas, **geom)
        both = head.render_occupancy(pred_dict, directions=rays.cuda(), cameras="all", stride=32, img_metas=cur_metas,
                                     **geom)
    Z = marched[0][0].shape[1]
    assert sweep.shape == (1, 7, 2, Z, model.bev_h, model.bev_w) and torch.equal(sweep[0], want)
    assert torch.equal(both, sweep + cams) and float(cams.sum()) > 0 and float(sweep.sum()) > 0
    with pytest.raises(ValueError):
        head.render_occupancy(pred_dict, img_metas=cur_metas, **geom)

    call = lambda **kw: model.forecast(img_metas=metas, img_feats=feats, rays=rays, cameras="all", stride=32, **kw)
    plain = call()
    with deterministic.use(True):
        occ = call(occupancy=True)
        occ_both = call(occupancy="both", min_evidence=0.25)
    assert sorted(occ) == sorted(list(plain) + ["evidence", "occupancy"])
    for out in (occ, occ_both):
        assert torch.equal(out["depth"], plain["depth"])
        for k in ("sweep", "sweep_index"):
            assert all(torch.equal(a, b) for a, b in zip(out[k][0], plain[k][0]))
    assert torch.equal(occ["evidence"], sweep) and torch.equal(occ_both["evidence"], both)
    for out, floor in ((occ, 0.5), (occ_both, 0.25)):
        ev, o = out["evidence"], out["occupancy"]
        assert o.shape == (1, 7, Z, model.bev_h, model.bev_w)
        unseen = ev.sum(2) < floor
        assert torch.equal(torch.isnan(o), unseen) and 0 < int(unseen.sum()) < unseen.numel()
        seen = o[~unseen]
        assert float(seen.min()) >= 0.0 and float(seen.max()) <= 1.0
        assert torch.equal(seen, (ev[:, :, 0] / ev.sum(2))[~unseen])
    print(f"voxels seen by the sweep {int((~torch.isnan(occ['occupancy'])).sum())}, by sweep and cameras "
          f"{int((~torch.isnan(occ_both['occupancy'])).sum())} of {occ['occupancy'].numel()}")
