"""CPU: the decode's confidence (vidar_ray_stats_f32 / ray_ops.ray_stats, ViDAR.forecast(stats=...)) without a GPU.

1. The inputs of tests/ray_stats_cases.py have the properties the GPU test leans on, so a changed seed cannot hollow it out.
2. The restatement against plain Python loops, and against two volumes whose statistics are known in closed form.
3. vidar_amd.forecast.confidence_mask / confidence_overlay, the header's two prototypes, the argument checks of the two
   entries (no GPU call is reached) and ViDAR.forecast's argument handling through a stub head on CPU tensors."""
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import ray_stats_cases as RC
from vidar_amd import forecast as FC

ROOT = Path(__file__).resolve().parents[1]


# ---- 1. the inputs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,K,step", RC.CASES, ids=RC.CASE_IDS)
def test_inputs_keep_their_properties(kind, K, step):
    c = RC.case(kind, K, step)
    assert c.pts.shape == (RC.R, 3) and RC.R % 4 != 0
    assert c.marched.tolist() == [r not in RC.SKIPPED for r in range(RC.R)]
    dead = int((~c.has_live).sum())                                  # rays without a live waypoint, the skipped ones included
    print(f"dead {dead}, live-set mismatches {int((~c.same_live).sum())}, live waypoints: max {int(c.n_live.max())}, "
          f"median {int(c.n_live[c.marched].median())}")
    assert 1 <= dead <= 4
    assert int((~c.same_live).sum()) == 0
    assert bool(c.has_live[list(RC.REVERSED)].all()) and int(c.n_live[list(RC.REVERSED)].max()) * step <= 4.0
    if (K, step) == (512, 0.2):
        assert int(c.n_live.max()) > 448                             # all eight registers of a lane hold a live waypoint
    if (K, step) == (1026, 0.125):
        assert int(c.n_live.max()) > 512


def test_arg_max_ties_are_why_the_depth_is_handed_in():
    c = RC.case("const", 512, 1.0)
    k32, k64 = c.z32.max(1)[1], c.z64.max(1)[1]
    differ = int((k32 != k64)[c.has_live].sum())
    print(f"constant volume: fp32 and fp64 pick another first arg-max on {differ} of {int(c.has_live.sum())} rays")
    assert differ > 0


# ---- 2. the restatement ------------------------------------------------------------------------------------------------
def loop_stats(z, length, d):
    live = [(zk, lk) for zk, lk in zip(z, length) if zk != -math.inf]
    if not live:
        return [0.0] * 4
    m = max(zk for zk, _ in live)
    S = sum(math.exp(zk - m) for zk, _ in live)
    mean = d + sum(math.exp(zk - m) * (lk - d) for zk, lk in live) / S
    rms = math.sqrt(sum(math.exp(zk - m) * (lk - d) ** 2 for zk, lk in live) / S)
    ent = math.log(S) - sum(math.exp(zk - m) * (zk - m) for zk, lk in live) / S
    return [1.0 / S, mean, rms, ent]


@pytest.mark.parametrize("kind,K,step", [("randn", 65, 0.25), ("plane", 512, 1.0)], ids=["randn-K65", "plane-K512"])
def test_restatement_against_plain_loops(kind, K, step):
    c = RC.case(kind, K, step)
    d = RC.argmax_depth(c.z64, c.len64) + 0.37                       # any depth: the statistics are about what is handed in
    got = RC.stats_about(c.z64, c.len64, d)
    for r in list(range(0, RC.R, 9)) + list(RC.SKIPPED):
        want = loop_stats(c.z64[r].tolist(), c.len64[r].tolist(), float(d[r]))
        np.testing.assert_allclose(got[r].numpy(), want, rtol=1e-12, atol=1e-12)
    assert float(got[list(RC.SKIPPED)].abs().max()) == 0.0
    assert got.dtype == torch.float64 and RC.stats_about(c.z32, c.len32, d.float()).dtype == torch.float32
    live = got[c.has_live]
    assert bool((live[:, 0] > 0).all()) and bool((live[:, 0] <= 1).all()) and bool((live[:, 3] >= 0).all())
    # the mean does not depend on the depth it is accumulated about; the spread about the mean is the smallest
    about_mean = RC.stats_about(c.z64, c.len64, got[:, 1])
    np.testing.assert_allclose(about_mean[:, 1].numpy(), got[:, 1].numpy(), rtol=1e-12, atol=1e-12)
    assert bool((about_mean[:, 2] <= got[:, 2] + 1e-12).all())


@pytest.mark.parametrize("K,step", RC.MARCHES, ids=[f"K{k}-step{s}" for k, s in RC.MARCHES])
def test_constant_volume_is_uniform_over_the_live_waypoints(K, step):
    """Every waypoint whose eight corners lie inside the volume samples the same value, so a ray whose live waypoints
    are all of that kind has p_max = 1 / n_live and entropy = log n_live."""
    c = RC.case("const", K, step)
    # the eight weights sum to 1 only up to rounding: the unpadded samples agree to a few ulp of 0.75
    interior = ((c.z64 - 0.75).abs() <= 4 * 2.0 ** -53) | ~c.live64
    rays = interior.all(1) & c.has_live
    print(f"rays with only interior live waypoints: {int(rays.sum())}")
    if K * step <= 40:
        assert int(rays.sum()) >= 10                                 # the short marches end inside the volume
    s = RC.stats_about(c.z64, c.len64, RC.argmax_depth(c.z64, c.len64))[rays]
    n = c.n_live[rays].double()
    np.testing.assert_allclose((s[:, 0] * n).numpy(), 1.0, rtol=0, atol=1e-12)
    np.testing.assert_allclose(s[:, 3].numpy(), n.log().numpy(), rtol=0, atol=1e-12)


# Which rays of the plane volume have their mass AT the plane.  Along a ray that crosses the layer x = 40 away from the
# volume's faces the logit is -2 + 16 max(0, 1 - |x - 40.5|).  With delta the distance in x from x = 40.5 to the nearest
# waypoint and s the waypoints' spacing in x (step times |d_x| >= 0.97 here) the other waypoints weigh, next to the best,
#   exp(-16 (s - 2 delta)), exp(-16 s), exp(-16 (2 s - 2 delta)), exp(-16 * 2 s) ... (inside the layer's two voxels) and
#   exp(-16 (1 - delta)) each (the background, at most 94 / step waypoints).
# step 1.0, delta <= 0.25: 2 exp(-8) + 94 exp(-12) = 1.3e-3, p_max > 0.998; the background's exp(-12) times its squared
#   distances (sum over l of (l - d)^2 <= (38^3 + 56^3) / 3 = 7.7e4 for d = 38 or 52.7) is 0.47, rms < 0.7.
# step 0.2, delta <= 0.004, s >= 0.194: exp(-2.98) + exp(-3.10) + exp(-6.08) + exp(-6.21) + ... + 470 exp(-15.9) < 0.105,
#   p_max > 0.905; a near tie (delta = 0.1) gives 0.5, so most crossing rays do NOT reach 0.9 at this step.  The neighbours
#   add 0.0035 to the squared spread; the background's 1.04e-7 per waypoint times sum (l - d)^2 = integral / 0.2 adds 0.037
#   on a ray that runs the volume's whole length -- by itself the square of one step -- and less than 0.030 when the ray has
#   at most 400 live waypoints (80 voxels: (52.9^3 + 27.1^3) / 3 / 0.2 * 1.04e-7 = 0.029): rms < 0.19 < 0.2 there.
PLANE_DELTA = {1.0: 0.25, 0.2: 0.004}
PLANE_MAX_LIVE = {1.0: 512, 0.2: 400}


@pytest.mark.parametrize("step", [1.0, 0.2])
def test_plane_volume_puts_the_mass_at_the_plane(step):
    """p_max > 0.9 and rms below one step, for the crossing rays the derivation above names.  Asked of EVERY crossing ray
    the two bounds fail in the fp64 restatement itself, whatever a kernel does: of the 48 rays that cross the plane, 34
    have p_max > 0.9 and 18 have rms < step at step 1.0, 9 and 7 at step 0.2 (where p_max is 0.9209 at best and 0.49 on a
    tie).  Held to the bounds here: 10 rays at step 1.0 (p_max 0.9992 - 0.9997, rms 0.47 - 0.66) and 4 at step 0.2
    (p_max 0.9188 - 0.9209; rms 0.180 and 0.191 on the two with at most 400 live waypoints, 0.209 and 0.212 on the two
    that run the volume's length)."""
    c = RC.case("plane", 512, step)
    delta, crosses = RC.plane_offsets(c.origin, c.pts, c.tindex, 512, step)
    d = RC.argmax_depth(c.z64, c.len64)
    s = RC.stats_about(c.z64, c.len64, d)
    resolved = crosses & (delta <= PLANE_DELTA[step])
    short = resolved & (c.n_live <= PLANE_MAX_LIVE[step])
    print(f"step {step}: {int(crosses.sum())} rays cross the plane, {int(resolved.sum())} with a waypoint within "
          f"{PLANE_DELTA[step]} of it: p_max {float(s[resolved, 0].min()):.4f} .. {float(s[resolved, 0].max()):.4f}, "
          f"rms {float(s[resolved, 2].min()):.4f} .. {float(s[resolved, 2].max()):.4f}; of all crossing rays "
          f"{int((s[crosses, 0] > 0.9).sum())} have p_max > 0.9 and {int((s[crosses, 2] < step).sum())} rms < step")
    assert int(crosses.sum()) >= 30 and int(short.sum()) >= 1
    assert bool(crosses[RC.AIMED]) and (step != 0.2 or bool(short[RC.AIMED]))
    assert bool((s[resolved, 0] > 0.9).all())
    assert bool((s[short, 2] < step).all())
    # the decoded depth is the plane: the arg-max waypoint is the one nearest to x = 40.5
    o = c.origin[c.tindex.long().clamp(0, RC.F_ - 1)].double()
    unit = c.pts.double() - o
    unit = unit / unit.norm(dim=1, keepdim=True)
    off = (o[:, 0] + d * unit[:, 0] - (RC.PLANE_X + 0.5)).abs()
    assert bool((off[crosses] <= delta[crosses] + 1e-6).all())


def test_yardstick_errors_are_those_of_fp32():
    """fp32 against fp64 restatement about one depth: small against the statistics' size (up to some 60 voxels), and of
    the size the docstring's table reports -- the GPU test recomputes them about the device's own depth."""
    worst = torch.zeros(4, dtype=torch.float64)
    for kind, K, step in RC.CASES:
        c = RC.case(kind, K, step)
        _, err = c.yardstick(RC.argmax_depth(c.z32, c.len32))
        print(f"{kind:6s} K {K:5d} step {step:5.3f}  " + "  ".join(f"{e:.1e}" for e in err.tolist()))
        worst = torch.maximum(worst, err)
    assert bool((worst > 0).all()) and float(worst.max()) < 1e-3


# ---- 3. masks, pictures, prototypes, argument handling -----------------------------------------------------------------
def test_confidence_mask_truth_table():
    nan = float("nan")
    stats = torch.tensor([[0.9, 10.0, 0.5, 0.1], [0.5, 10.0, 0.5, 0.7], [0.9, 10.0, 3.0, 0.1], [0.2, 10.0, 3.0, 1.0],
                          [0.0, 0.0, 0.0, 0.0], [nan, 1.0, 0.5, 0.1], [0.9, 1.0, nan, 0.1], [1.0, nan, 0.0, nan]])
    table = {
        (None, None): [1, 1, 1, 1, 1, 1, 1, 1],
        (0.6, None): [1, 0, 1, 0, 0, 0, 1, 1],
        (None, 1.0): [1, 1, 0, 0, 1, 1, 0, 1],
        (0.6, 1.0): [1, 0, 0, 0, 0, 0, 0, 1],
        (0.0, math.inf): [1, 1, 1, 1, 1, 0, 0, 1],                   # a NaN fails the threshold it is held against
        (0.5, 0.5): [1, 1, 0, 0, 0, 0, 0, 1],                        # the thresholds themselves pass
    }
    for (p, r), want in table.items():
        got = FC.confidence_mask(stats, min_prob=p, max_rms=r)
        assert got.dtype == torch.bool and got.tolist() == [bool(w) for w in want], (p, r)
    grid = FC.confidence_mask(stats.view(2, 4, 4), 0.6, 1.0)
    assert grid.shape == (2, 4) and grid.view(-1).tolist() == [bool(w) for w in table[(0.6, 1.0)]]
    assert FC.confidence_mask(torch.zeros(0, 4), 0.5).shape == (0,)


def test_confidence_overlay_by_hand():
    """2 x 2 values over a 4 x 4 frame at stride 2, alpha 160.  colour_table at index i is (clamp(384 - |4 i - 768|),
    clamp(384 - |4 i - 512|), clamp(384 - |4 i - 256|)) clamped to 0..255:
      p = 1.0  -> index 255 -> (132, 0, 0);  p = 0.5 -> floor(128.0) = 128 -> (128, 255, 128);
      p = 0.25 -> floor(64.25) = 64 -> (0, 128, 255);  p = 0 -> no return, the frame shows.
    blend = (160 c + 95 f + 127) // 255 over the frame value f = 100: 132 -> 120, 0 -> 37, 128 -> 118, 255 -> 197."""
    frame = torch.full((4, 4, 3), 100, dtype=torch.uint8)
    got = FC.confidence_overlay(torch.tensor([[1.0, 0.5], [0.25, 0.0]]), frame)
    want = np.empty((4, 4, 3), np.uint8)
    want[:2, :2] = (120, 37, 37)
    want[:2, 2:] = (118, 197, 118)
    want[2:, :2] = (37, 118, 197)
    want[2:, 2:] = (100, 100, 100)
    np.testing.assert_array_equal(got.numpy(), want)
    assert FC.colour_table()[[255, 128, 64]].tolist() == [[132, 0, 0], [128, 255, 128], [0, 128, 255]]
    nan = FC.confidence_overlay(torch.tensor([[float("nan"), 2.0], [-1.0, 1.0]]), frame, alpha=255)
    assert nan[0, 0].tolist() == [100] * 3 and nan[2, 0].tolist() == [100] * 3       # NaN and negative: no return
    assert nan[0, 2].tolist() == [132, 0, 0] and nan[2, 2].tolist() == [132, 0, 0]   # above 1 clamps to the red end
    with pytest.raises(ValueError):
        FC.confidence_overlay(torch.ones(3, 2), frame)


def test_header_declares_both_entries_returning_int():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "vidar_hip.h").read_text(), flags=re.S)
    protos = {name: (ret, [p.strip() for p in params.split(",")])
              for ret, name, params in re.findall(r"\b(\w+)\s+(vidar_ray_stats\w*)\s*\(([^()]*)\)\s*;", text)}
    assert sorted(protos) == ["vidar_ray_stats_cam_f32", "vidar_ray_stats_f32"]
    assert all(ret == "int" for ret, _ in protos.values())
    assert protos["vidar_ray_stats_f32"][1] == [
        "const float* sigma", "const float* origin", "const float* pts", "const float* tindex", "float* pred_dist",
        "float* gt_dist", "float* stats", "int F", "int R", "int Z", "int Y", "int X", "int K", "float step", "void* stream"]
    assert protos["vidar_ray_stats_cam_f32"][1] == [
        "const float* sigma", "const float* pix2vox", "float* dist", "float* stats", "int F", "int C", "int Hs", "int Ws",
        "float u0", "float v0", "float du", "float dv", "int Z", "int Y", "int X", "int K", "float step", "void* stream"]
    from vidar_amd import _lib
    assert _lib._ABI["vidar_ray_stats_f32"].split()[0] == "i" and _lib._ABI["vidar_ray_stats_cam_f32"].split()[0] == "i"


def test_entries_check_their_arguments_before_any_gpu_call():
    from vidar_amd._lib import BAD_ARG, lib
    L = lib()
    good = dict(F=2, C=6, Hs=225, Ws=400, u0=2.0, v0=2.0, du=4.0, dv=4.0)

    def listed(F=2, R=0, Z=16, Y=200, X=200, K=512, stats=None):
        return L.vidar_ray_stats_f32(None, None, None, None, None, None, stats, F, R, Z, Y, X, K, 1.0, None)

    def cam(K=512, Z=16, stats=None, **kw):
        g = dict(good, **kw)
        return L.vidar_ray_stats_cam_f32(None, None, None, stats, g["F"], g["C"], g["Hs"], g["Ws"], g["u0"], g["v0"],
                                         g["du"], g["dv"], Z, 200, 200, K, 1.0, None)

    assert listed() == 0 and cam(Hs=0) == 0 and cam(Ws=0) == 0                         # empty problem: no launch
    for kw in (dict(K=0), dict(K=L.vidar_ray_max_k() + 1), dict(F=0), dict(R=-1), dict(Z=0), dict(Y=0), dict(X=0),
               dict(stats=8)):                                                        # stats must be 16-byte aligned
        assert listed(**kw) == BAD_ARG, kw
    for kw in (dict(F=0), dict(C=0), dict(Hs=-1), dict(Ws=-1), dict(du=0.0), dict(dv=0.0), dict(u0=float("nan")),
               dict(dv=float("nan")), dict(F=6, C=6, Hs=9000, Ws=16000)):              # 5.2e9 rays: beyond 2^31
        assert cam(**kw) == BAD_ARG, kw
    assert cam(K=0, Hs=0) == BAD_ARG and cam(K=L.vidar_ray_max_k() + 1, Hs=0) == BAD_ARG
    assert cam(Z=0, Hs=0) == BAD_ARG and cam(stats=4, Hs=0) == BAD_ARG


def test_new_kernels_are_in_the_library_in_both_forms():
    import sys
    sys.path.insert(0, str(ROOT / "tools"))
    import kernel_resources
    from vidar_amd import build
    by = {r["kernel"]: r for r in kernel_resources.table(build.build(verbose=False))}
    for name in ("ray_stats_kernel", "ray_stats_any_kernel", "ray_stats_cam_kernel", "ray_stats_cam_any_kernel"):
        assert name in by, name
        r = by[name]
        assert r["wave"] == 64 and r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["lds"] == 0, r
        assert r["waves_per_simd"] == 8, r                           # the four sums do not cost the decode a wave slot
    assert by["ray_argmax_kernel"]["waves_per_simd"] == 8


# ---- ViDAR.forecast's argument handling, through a stub head on CPU tensors --------------------------------------------
class _StubHead(torch.nn.Module):
    """two frames of four known rays each: the last point of a frame lies outside the point-cloud range"""
    PTS = torch.tensor([[5.0, 5.0, 0.0], [-10.0, 20.0, 0.0], [1.0, 2.0, 0.5], [500.0, 0.0, 0.0]])
    STATS = torch.tensor([[0.9, 7.0, 0.4, 0.2], [0.3, 20.0, 6.0, 1.5], [0.6, 2.0, 1.0, 0.8], [0.95, 500.0, 0.1, 0.1]])

    def __init__(self):
        super().__init__()
        self.calls = []

    def render_rays(self, pred_dict, directions=None, *, img_metas=None, return_stats=False, **geom):
        self.calls.append(("rays", return_stats))
        pts = [[self.PTS.clone(), self.PTS * 0.1]]                   # frame 1: all four inside
        return (pts, [[self.STATS.clone(), self.STATS.flip(0)]]) if return_stats else pts

    def render_cameras(self, pred_dict, img_metas, cameras=None, stride=4, return_stats=False, **geom):
        self.calls.append(("cameras", return_stats))
        depth = torch.tensor([7.0, 20.0, 2.0, 0.0]).view(1, 1, 1, 2, 2).repeat(1, 2, 1, 1, 1)
        stats = self.STATS.clone()
        stats[3] = 0.0                                               # nothing met: four zeros
        return (depth, stats.view(1, 1, 1, 2, 2, 4).repeat(1, 2, 1, 1, 1, 1)) if return_stats else depth


def _stub_detector():
    from vidar_amd.plugin.detectors.vidar import ViDAR
    det = ViDAR.__new__(ViDAR)
    torch.nn.Module.__init__(det)
    det.future_pred_head = _StubHead()
    det.point_cloud_range = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
    det.bev_h = det.bev_w = 8
    det._future_pred_dict = lambda img_metas, img=None, img_feats=None: (
        dict(valid_frames=[0, 1], next_bev_preds=torch.zeros(2, 1, 1, 64, 4)), [dict(sample_idx="tok7")])
    return det


def _forecast(det, **kw):
    det.future_pred_head.calls.clear()
    out = det.forecast(img=torch.zeros(1, 1), img_metas=[None], rays=torch.zeros(4, 3), cameras="all", **kw)
    return out, list(det.future_pred_head.calls)


def test_forecast_argument_handling():
    det = _stub_detector()
    plain, calls = _forecast(det)
    assert calls == [("rays", False), ("cameras", False)]            # nothing new is asked of the head
    assert sorted(plain) == ["depth", "sweep", "sweep_index", "valid_frames"]
    assert [i.tolist() for i in plain["sweep_index"][0]] == [[0, 1, 2], [0, 1, 2, 3]]

    with_stats, calls = _forecast(det, stats=True)
    assert calls == [("rays", True), ("cameras", True)]
    assert sorted(with_stats) == ["depth", "depth_stats", "sweep", "sweep_index", "sweep_stats", "valid_frames"]
    assert torch.equal(with_stats["depth"], plain["depth"])
    for a, b in zip(with_stats["sweep"][0], plain["sweep"][0]):
        assert torch.equal(a, b)
    assert torch.equal(with_stats["sweep_stats"][0][0], _StubHead.STATS[:3])          # aligned with the cropped sweep
    assert torch.equal(with_stats["sweep_stats"][0][1], _StubHead.STATS.flip(0))
    assert with_stats["depth_stats"].shape == (1, 2, 1, 2, 2, 4)

    for kw in (dict(min_prob=0.5), dict(max_rms=1.0), dict(min_prob=0.5, max_rms=0.5)):
        out, calls = _forecast(det, **kw)                            # a threshold implies the statistics
        assert calls == [("rays", True), ("cameras", True)] and "sweep_stats" in out and "depth_stats" in out, kw
    out, _ = _forecast(det, min_prob=0.5)
    assert [i.tolist() for i in out["sweep_index"][0]] == [[0, 2], [0, 1, 3]]          # frame 1 holds the stats flipped
    assert torch.equal(out["sweep"][0][0], _StubHead.PTS[[0, 2]])
    assert torch.equal(out["sweep_stats"][0][0], _StubHead.STATS[[0, 2]])
    assert out["depth"][0, 0, 0].tolist() == [[7.0, 0.0], [2.0, 0.0]]                 # the dropped pixel: nothing met
    out, _ = _forecast(det, max_rms=0.5)
    assert [i.tolist() for i in out["sweep_index"][0]] == [[0], [0, 3]]
    assert out["depth"][0, 1, 0].tolist() == [[7.0, 0.0], [0.0, 0.0]]
    out, _ = _forecast(det, min_prob=0.0, max_rms=math.inf)
    assert [i.tolist() for i in out["sweep_index"][0]] == [[0, 1, 2], [0, 1, 2, 3]]
    assert torch.equal(out["depth"], plain["depth"])
    only, calls = _forecast(det, stats=False, min_prob=None, max_rms=None)
    assert calls == [("rays", False), ("cameras", False)] and sorted(only) == sorted(plain)
