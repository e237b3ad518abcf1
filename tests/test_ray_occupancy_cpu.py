"""CPU: occupancy evidence of the decode's softmax (vidar_ray_occupancy_f32 / ray_ops.ray_occupancy,
ViDAR.forecast(occupancy=...)) without a GPU.

1. the torch restatement of tests/ray_occupancy_cases.py against plain Python loops on a handful of rays (fp64);
2. properties of the restatement: p + b <= 1, b of the last live waypoint is 0, a ray whose live waypoints keep all eight
   corners adds exactly 1 to hit.sum(), skipped rays add nothing;
3. the definition on the plane volume: free before the layer, occupied in it, unseen behind it;
4. vidar_amd.forecast.occupancy_grid / occupancy_bev;
5. plumbing: the header's prototypes, the entries' argument checks (no GPU call is reached), ViDAR.forecast's handling of
   occupancy= / min_evidence= through a stub head, the coverage row."""
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import ray_occupancy_cases as RO
import ray_stats_cases as RC

ROOT = Path(__file__).resolve().parents[1]


# ---- 1. plain loops ----------------------------------------------------------------------------------------------------
def loops(sigma, origin, pts, tindex, K, step):
    """(hit, free) as nested Python loops over rays, waypoints and corners, fp64 numpy"""
    vol = sigma.double().numpy()
    Fn, Z, Y, X = vol.shape
    hit, free = np.zeros_like(vol), np.zeros_like(vol)
    for r in range(pts.shape[0]):
        t = float(tindex[r])
        if not (0 <= t < Fn):
            continue
        f = int(t)
        o = origin[f].double().numpy()
        d = pts[r].double().numpy() - o
        d = d / math.sqrt(float((d * d).sum()))
        corners, z = [], []
        for k in range(K):
            s = o + d * ((k + 0.5) * step)
            pix = s - 0.5                                              # align_corners=False: voxel i spans [i, i + 1)
            base = np.floor(pix)
            a = pix - base
            cs, val = [], 0.0
            for c in range(8):
                bit = (c & 1, (c >> 1) & 1, c >> 2)
                x, y, zz = (int(base[i]) + bit[i] for i in range(3))
                w = 1.0
                for i in range(3):
                    w *= a[i] if bit[i] else 1.0 - a[i]
                if 0 <= x < X and 0 <= y < Y and 0 <= zz < Z:
                    cs.append((zz, y, x, w))
                    val += w * vol[f, zz, y, x]
            corners.append(cs)
            z.append(val if val != 0.0 else -math.inf)
        live = [v != -math.inf for v in z]
        if not any(live):
            continue
        m = max(z)
        e = [math.exp(v - m) if l else 0.0 for v, l in zip(z, live)]
        S = sum(e)
        p = [v / S for v in e]
        for k in range(K):
            if not live[k]:
                continue
            b = sum(p[j] for j in range(k + 1, K) if live[j])
            for zz, y, x, w in corners[k]:
                hit[f, zz, y, x] += p[k] * w
                free[f, zz, y, x] += b * w
    return torch.from_numpy(hit), torch.from_numpy(free)


@pytest.mark.parametrize("kind,K,step", [("randn", 37, 1.0), ("plane", 65, 0.25)], ids=["randn-K37", "plane-K65"])
def test_restatement_against_plain_loops(kind, K, step):
    sigma = RC.volume(kind)
    origin, pts, tindex = RC.rays()
    sel = [0, 1, 5, 6, 7, 11, 40]                                     # both frames, a reversed ray, the two skipped ones
    got = RO.occupancy(sigma.double(), origin, pts[sel], tindex[sel], K, step)
    want = loops(sigma, origin, pts[sel], tindex[sel], K, step)
    for g, w in zip(got, want):
        assert float(w.max()) > 0
        torch.testing.assert_close(g, w, rtol=1e-12, atol=0)


# ---- 2. properties -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,K,step", RO.CASES, ids=RO.CASE_IDS)
def test_properties_of_the_restatement(kind, K, step):
    c = RO.case(kind, K, step)
    for p, b, z, dt in ((c.p32, c.b32, c.rs.z32, torch.float32), (c.p64, c.b64, c.rs.z64, torch.float64)):
        eps = torch.finfo(dt).eps
        live = z != -math.inf
        assert bool((p >= 0).all()) and bool((b >= 0).all())
        assert bool((p + b <= 1 + K * eps).all())
        assert float(p[~live].abs().max()) == 0.0 and float(b[~live].abs().max()) == 0.0
        has = live.any(1)
        last = (live * torch.arange(1, K + 1)).max(1)[0] - 1            # index of the last live waypoint
        assert float(b[has, last[has]].abs().max()) == 0.0
        assert float((p.sum(1)[has] - 1).abs().max()) <= K * eps
        assert float(p[~has].abs().max()) == 0.0 and not bool(has[list(RC.SKIPPED)].any())
    for w32, w64 in zip(c.want32, c.want64):
        assert float(w32.min()) >= 0.0 and float(w64.min()) >= 0.0
    # rays whose live waypoints all keep their eight corners add exactly sum p = 1 each; the others less
    origin, pts, tindex = c.origin, c.pts, c.tindex
    live = c.rs.live64
    n = RO.counts(c.sigma.shape, origin, pts, tindex, K, step, live)
    assert int(n.sum()) <= 8 * int(live.sum())
    whole = torch.zeros(RC.R, dtype=torch.bool)
    for r in range(RC.R):
        if bool(live[r].any()):
            one = RO.counts(c.sigma.shape, origin, pts[r:r + 1], tindex[r:r + 1], K, step, live[r:r + 1])
            whole[r] = int(one.sum()) == 8 * int(live[r].sum())
    if bool(whole.any()):
        sel = whole.nonzero().squeeze(-1)
        hit = RO.splat(c.sigma.shape, origin, pts[sel], tindex[sel], K, step, c.p64[sel])
        assert abs(float(hit.sum()) - int(whole.sum())) <= 1e-9 * int(whole.sum())
    assert float(c.want64[0].sum()) <= int(c.rs.has_live.sum()) + 1e-9
    print(f"rays with every live corner inside {int(whole.sum())}, hit.sum() {float(c.want64[0].sum()):.4f}")


def test_skipped_rays_add_nothing():
    c = RO.case("randn", 64, 0.5)
    keep = torch.ones(RC.R, dtype=torch.bool)
    keep[list(RC.SKIPPED)] = False
    without = RO.occupancy(c.sigma.double(), c.origin, c.pts[keep], c.tindex[keep], 64, 0.5)
    for a, b in zip(without, c.want64):
        assert torch.equal(a, b)
    only = RO.occupancy(c.sigma.double(), c.origin, c.pts[~keep], c.tindex[~keep], 64, 0.5)
    assert all(float(t.abs().max()) == 0.0 for t in only)


# ---- 3. the definition on the plane volume -----------------------------------------------------------------------------
def test_plane_is_free_in_front_occupied_inside_unseen_behind():
    """one ray along +x through voxel centres (y cell 5, z cell 2), a waypoint per voxel: everything lands on one voxel
    per waypoint, the layer x = 40 holds logit 14 against -2 elsewhere"""
    from vidar_amd import forecast as FC
    sigma = RC.volume("plane").double()
    origin = torch.tensor([[2.0, 5.5, 2.5], [0.0, 0.0, 0.0]])
    pts = torch.tensor([[12.0, 5.5, 2.5]])
    hit, free = RO.occupancy(sigma, origin, pts, torch.zeros(1), 90, 1.0)
    occ, evidence = FC.occupancy_grid(hit[0], free[0])
    line, ev = occ[2, 5], evidence[2, 5]
    assert bool((line[2:RC.PLANE_X] < 1e-3).all()) and bool((ev[2:RC.PLANE_X] > 0.9).all())       # passed: free
    assert float(line[RC.PLANE_X]) > 0.99 and float(ev[RC.PLANE_X]) > 0.9                          # the return
    assert bool(torch.isnan(line[RC.PLANE_X + 1:92]).all()) and bool((ev[RC.PLANE_X + 1:] < 1e-3).all())
    assert bool(torch.isnan(line[:2]).all())                                                       # behind the sensor
    seen = ~torch.isnan(occ)
    assert int(seen.sum()) == RC.PLANE_X - 2 + 1                       # nothing off the ray is seen
    assert abs(float(hit.sum()) - 1.0) < 1e-12


# ---- 4. occupancy_grid / occupancy_bev ---------------------------------------------------------------------------------
def test_occupancy_grid_floor_and_nan():
    from vidar_amd import forecast as FC
    hit = torch.tensor([0.0, 0.25, 0.5, 0.1, 3.0, float("nan")])
    free = torch.tensor([0.0, 0.24, 0.0, 0.4, 1.0, 1.0])
    occ, ev = FC.occupancy_grid(hit, free)
    assert torch.equal(ev[:5], (hit + free)[:5]) and math.isnan(float(ev[5]))
    assert torch.isnan(occ).tolist() == [True, True, False, False, False, True]      # 0.49 < 0.5 <= 0.5
    assert occ[2:5].tolist() == [1.0, pytest.approx(0.2), 0.75]
    occ, _ = FC.occupancy_grid(hit, free, min_evidence=0.25)
    assert torch.isnan(occ).tolist() == [True, False, False, False, False, True]
    occ, _ = FC.occupancy_grid(hit, free, min_evidence=4.5)
    assert bool(torch.isnan(occ).all())
    assert FC.occupancy_grid(hit.view(1, 2, 3), free.view(1, 2, 3))[0].shape == (1, 2, 3)


def test_occupancy_bev_colours_and_orientation():
    from vidar_amd import forecast as FC
    nan = float("nan")
    occ = torch.full((2, 2, 3), nan)                                  # [Z, H, W]
    occ[0, 0, 0] = 0.0                                                # y = 0, x = 0: free
    occ[1, 0, 0] = nan
    occ[0, 0, 2], occ[1, 0, 2] = 0.25, 1.0                            # the max over Z: occupied
    occ[1, 1, 1] = 0.5
    img = FC.occupancy_bev(occ)
    assert img.shape == (2, 3, 3) and img.dtype == torch.uint8
    u = list(FC.UNSEEN_COLOUR)
    assert img[1].tolist() == [[255] * 3, u, [0] * 3]                 # y = 0 is the bottom row; x to the right
    assert img[0].tolist() == [u, [127] * 3, u]                       # 255 - floor(127.5 + 0.5)
    assert u not in ([g] * 3 for g in range(256))                     # no grey: it cannot be taken for a probability
    big = FC.occupancy_bev(occ, size_px=6)
    assert big.shape == (6, 6, 3)
    assert torch.equal(big[:3], img[0:1].expand(3, -1, -1).repeat_interleave(2, 1))
    assert torch.equal(big[3:], img[1:2].expand(3, -1, -1).repeat_interleave(2, 1))
    assert FC.occupancy_bev(torch.tensor([[[1.7, -0.3]]])).view(-1, 3).tolist() == [[0] * 3, [255] * 3]   # clamped
    with pytest.raises(ValueError):
        FC.occupancy_bev(torch.zeros(2, 2))


# ---- 5. plumbing -------------------------------------------------------------------------------------------------------
def test_header_declares_the_three_entries():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "vidar_hip.h").read_text(), flags=re.S)
    protos = {name: (ret, [p.strip() for p in params.split(",")])
              for ret, name, params in re.findall(r"\b(\w+)\s+(vidar_ray_occupancy\w*)\s*\(([^()]*)\)\s*;", text)}
    assert sorted(protos) == ["vidar_ray_occupancy_cam_f32", "vidar_ray_occupancy_f32",
                              "vidar_ray_occupancy_workspace_bytes"]
    assert protos["vidar_ray_occupancy_workspace_bytes"] == ("int", ["int F", "int Z", "int Y", "int X", "int64_t* bytes"])
    tail = ["int Z", "int Y", "int X", "int K", "float step", "void* workspace", "size_t workspace_bytes", "void* stream"]
    assert protos["vidar_ray_occupancy_f32"] == ("int", [
        "const float* sigma", "const float* origin", "const float* pts", "const float* tindex", "float* hit",
        "float* free_", "int F", "int R"] + tail)
    assert protos["vidar_ray_occupancy_cam_f32"] == ("int", [
        "const float* sigma", "const float* pix2vox", "float* hit", "float* free_", "int F", "int C", "int Hs", "int Ws",
        "float u0", "float v0", "float du", "float dv"] + tail)
    from vidar_amd import _lib
    assert _lib._ABI["vidar_ray_occupancy_workspace_bytes"] == "i 4i p"
    assert _lib._ABI["vidar_ray_occupancy_f32"] == "i 6p 6i f p z p"
    assert _lib._ABI["vidar_ray_occupancy_cam_f32"] == "i 4p 4i 4f 4i f p z p"


def test_entries_check_their_arguments_before_any_gpu_call():
    from vidar_amd._lib import BAD_ARG, lib
    L = lib()
    good = dict(F=2, C=6, Hs=225, Ws=400, u0=2.0, v0=2.0, du=4.0, dv=4.0)

    def listed(F=2, R=8, Z=16, Y=200, X=200, K=512):
        return L.vidar_ray_occupancy_f32(None, None, None, None, None, None, F, R, Z, Y, X, K, 1.0, None, 0, None)

    def cam(K=512, Z=16, **kw):
        g = dict(good, **kw)
        return L.vidar_ray_occupancy_cam_f32(None, None, None, None, g["F"], g["C"], g["Hs"], g["Ws"], g["u0"], g["v0"],
                                             g["du"], g["dv"], Z, 200, 200, K, 1.0, None, 0, None)

    for kw in (dict(K=0), dict(K=L.vidar_ray_max_k() + 1), dict(F=0), dict(R=-1), dict(Z=0), dict(Y=0), dict(X=0)):
        assert listed(**kw) == BAD_ARG, kw
    for kw in (dict(F=0), dict(C=0), dict(Hs=-1), dict(Ws=-1), dict(du=0.0), dict(dv=0.0), dict(u0=float("nan")),
               dict(dv=float("nan")), dict(F=6, C=6, Hs=9000, Ws=16000), dict(K=0), dict(K=L.vidar_ray_max_k() + 1),
               dict(Z=0), dict(K=0, Hs=0)):
        assert cam(**kw) == BAD_ARG, kw
    from vidar_amd.plugin.dense_heads.ray_ops import occupancy_workspace_bytes as query
    cells = 2 * 16 * 200 * 200
    assert query(2, 16, 200, 200) in (4 * 8 * 2 * cells, 8 * (2 * cells + 2))
    assert L.vidar_ray_occupancy_workspace_bytes(2, 16, 200, 200, None) == BAD_ARG
    with pytest.raises(ValueError):
        query(0, 16, 200, 200)
    was = L.vidar_get_deterministic()
    L.vidar_set_deterministic(1)
    try:
        assert query(2, 16, 200, 200) == 8 * (2 * cells + 2)
        assert listed() == BAD_ARG and cam() == BAD_ARG               # the mode never falls back: no workspace, no run
        assert L.vidar_ray_occupancy_f32(None, None, None, None, None, None, 2, 8, 16, 200, 200, 512, 1.0, 4096, 64,
                                         None) == BAD_ARG             # too small
    finally:
        L.vidar_set_deterministic(was)
    assert query(2, 16, 200, 200) == (8 * (2 * cells + 2) if was else 4 * 8 * 2 * cells)


def test_coverage_row():
    from vidar_amd import deterministic
    row = ("ray_occupancy", "fixed-point", "vidar_ray_occupancy{,_cam}_f32 (hit, free)")
    assert row in deterministic.coverage()
    assert "| ray_occupancy | fixed-point | `vidar_ray_occupancy{,_cam}_f32 (hit, free)` |" in (ROOT / "README.md").read_text()
    assert {s for _, s, _ in deterministic.coverage()} == {"fixed-point", "fixed-order", "already deterministic", "not covered"}


class _StubHead(torch.nn.Module):
    EVIDENCE = torch.tensor([[0.6, 0.0], [0.2, 0.2], [0.0, 2.0], [0.0, 0.0]]).t().reshape(1, 1, 2, 1, 2, 2)

    def __init__(self):
        super().__init__()
        self.calls = []

    def render_rays(self, pred_dict, directions=None, *, img_metas=None, return_stats=False, **geom):
        self.calls.append("rays")
        return [[torch.tensor([[5.0, 5.0, 0.0]])]]

    def render_cameras(self, pred_dict, img_metas, cameras=None, stride=4, return_stats=False, **geom):
        self.calls.append("cameras")
        return torch.ones(1, 1, 1, 2, 2)

    def render_occupancy(self, pred_dict, directions=None, end_points=None, *, cameras=None, stride=4, img_metas=None,
                         **geom):
        assert sorted(geom) == ["tgt_bev_h", "tgt_bev_w", "tgt_pc_range"] and end_points is None
        self.calls.append(("occupancy", directions is not None, cameras, stride))
        return self.EVIDENCE.clone()


def _stub_detector():
    from vidar_amd.plugin.detectors.vidar import ViDAR
    det = ViDAR.__new__(ViDAR)
    torch.nn.Module.__init__(det)
    det.future_pred_head = _StubHead()
    det.point_cloud_range = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
    det.bev_h = det.bev_w = 2
    det._future_pred_dict = lambda img_metas, img=None, img_feats=None: (
        dict(valid_frames=[0], next_bev_preds=torch.zeros(1, 1, 1, 4, 1)), [dict(sample_idx="tok7")])
    return det


def test_forecast_argument_handling():
    det = _stub_detector()
    head = det.future_pred_head

    def forecast(rays=torch.zeros(4, 3), cameras="all", **kw):
        head.calls.clear()
        return det.forecast(img=torch.zeros(1, 1), img_metas=[None], rays=rays, cameras=cameras, stride=8, **kw), list(head.calls)
    plain, calls = forecast()
    assert calls == ["rays", "cameras"] and sorted(plain) == ["depth", "sweep", "sweep_index", "valid_frames"]
    same, calls = forecast(occupancy=False, min_evidence=3.0)
    assert calls == ["rays", "cameras"] and sorted(same) == sorted(plain)
    for value, want in ((True, (True, None)), ("sweep", (True, None)), ("cameras", (False, "all")), ("both", (True, "all"))):
        out, calls = forecast(occupancy=value)
        assert calls == ["rays", "cameras", ("occupancy", *want, 8)], value
        assert sorted(out) == sorted(list(plain) + ["evidence", "occupancy"])
        assert torch.equal(out["depth"], plain["depth"]) and torch.equal(out["sweep"][0][0], plain["sweep"][0][0])
        assert torch.equal(out["evidence"], _StubHead.EVIDENCE) and out["occupancy"].shape == (1, 1, 1, 2, 2)
        occ = out["occupancy"].view(-1)
        assert occ[0] == 1.0 and math.isnan(occ[1]) and occ[2] == 0.0 and math.isnan(occ[3])
    out, _ = forecast(occupancy=True, min_evidence=0.3)
    assert out["occupancy"].view(-1)[1] == 0.5
    out, calls = forecast(cameras=[1, 3], occupancy="cameras")
    assert calls[-1] == ("occupancy", False, [1, 3], 8)
    for bad in (dict(occupancy="lidar"), dict(occupancy="sweep", rays=None), dict(occupancy=True, rays=None),
                dict(occupancy="cameras", cameras=None), dict(occupancy="both", cameras=None)):
        with pytest.raises(ValueError):
            forecast(**bad)
