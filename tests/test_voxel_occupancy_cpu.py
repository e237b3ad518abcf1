"""CPU: the occupancy query at listed points and at every voxel's centre (vidar_point_occupancy_f32 /
vidar_voxel_occupancy_f32, ray_ops.point_occupancy / voxel_occupancy, ViDAR.forecast(occupancy="dense")) without a GPU.

1. the torch restatement of tests/voxel_occupancy_cases.py against plain Python loops on a handful of rays (fp64);
2. csrc/occ_at_math.h in a stand-alone host program (tests/occ_at_host.cpp) under the host sanitizers: the weights
   against fp64, partition of unity, the cases L < extent/2, L - extent/2 >= K step and step > extent;
3. the definition on the plane volume: free before the layer, occupied in it, no evidence behind it;
4. properties of the restatement: ranges, exact zeros beyond K step, continuity in L;
5. the exclusion cap of the precision comparison, on the restatements alone;
6. plumbing: the header's prototypes against _lib._ABI, the entries' argument checks (no GPU call is reached),
   ViDAR.forecast(occupancy="dense") through a stub head, eval_utils.set_occupancy_metrics(source=...)."""
import math
import os
import re
import subprocess
from pathlib import Path

import pytest
import torch

import ray_stats_cases as RS
import voxel_occupancy_cases as VC

ROOT = Path(__file__).resolve().parents[1]


# ---- 1. plain loops ----------------------------------------------------------------------------------------------------
def loops(sigma, origin, pts, tindex, K, step, extent):
    """[R, 2] (hit, free) as nested Python loops over rays, waypoints and corners, fp64"""
    vol = sigma.double().numpy()
    Fn, Z, Y, X = vol.shape
    out = torch.zeros(pts.shape[0], 2, dtype=torch.float64)
    for r in range(pts.shape[0]):
        t = float(tindex[r])
        if not (0 <= t < Fn):
            continue
        f = int(t)
        o = [float(v) for v in origin[f]]
        d = [float(pts[r, i]) - o[i] for i in range(3)]
        L = math.sqrt(sum(v * v for v in d))
        if L == 0.0:
            continue
        d = [v / L for v in d]
        z = []
        for k in range(K):
            pix = [o[i] + d[i] * ((k + 0.5) * step) - 0.5 for i in range(3)]   # align_corners=False: voxel i spans [i, i + 1)
            base = [math.floor(v) for v in pix]
            a = [pix[i] - base[i] for i in range(3)]
            val = 0.0
            for c in range(8):
                bit = (c & 1, (c >> 1) & 1, c >> 2)
                x, y, zz = (base[i] + bit[i] for i in range(3))
                w = 1.0
                for i in range(3):
                    w *= a[i] if bit[i] else 1.0 - a[i]
                if 0 <= x < X and 0 <= y < Y and 0 <= zz < Z:
                    val += w * vol[f, zz, y, x]
            z.append(val)
        live = [v != 0.0 for v in z]
        if not any(live):
            continue
        m = max(v for v, l in zip(z, live) if l)
        e = [math.exp(v - m) if l else 0.0 for v, l in zip(z, live)]
        S = sum(e)
        clamp = lambda v: min(max(v, 0.0), 1.0)
        for k in range(K):
            c_near = clamp((L - extent / 2 - k * step) / step)
            c_far = clamp((L + extent / 2 - k * step) / step)
            out[r, 0] += e[k] / S * (c_far - c_near)
            out[r, 1] += e[k] / S * (1.0 - c_far)
    return out


@pytest.mark.parametrize("kind,K,step,extent", [("randn", 37, 1.0, 1.0), ("plane", 65, 0.25, 2.5), ("randn", 64, 0.5, 0.3)],
                         ids=["randn-K37", "plane-K65", "randn-K64"])
def test_restatement_against_plain_loops(kind, K, step, extent):
    sigma = RS.volume(kind)
    origin, pts, tindex = RS.rays()
    sel = [0, 1, 5, 6, 7, 11, 40]                                     # both frames, a reversed ray, the two skipped ones
    pts, tindex = torch.cat([pts[sel], origin[:1]]), torch.cat([tindex[sel], torch.zeros(1)])   # and a query AT the origin
    got = VC.point_occupancy(sigma.double(), origin, pts, tindex, K, step, extent)
    want = loops(sigma, origin, pts, tindex, K, step, extent)
    assert got.dtype == torch.float64 and got.shape == (8, 2)
    torch.testing.assert_close(got, want, rtol=1e-11, atol=1e-13)
    assert float(got[[2, 3, 7]].abs().max()) == 0.0                   # skipped, skipped, at the origin
    assert float(got[0].sum()) > 0.0 and int((got.sum(1) > 0).sum()) >= 3


def test_voxel_centres_are_the_flattened_grids_order():
    pts, tindex = VC.voxel_centres((2, 3, 4, 5))
    assert pts.shape == (120, 3) and tindex.shape == (120,) and pts.dtype == tindex.dtype == torch.float32
    grid = pts.view(2, 3, 4, 5, 3)
    assert grid[1, 2, 3, 4].tolist() == [4.5, 3.5, 2.5] and grid[0, 0, 0, 1].tolist() == [1.5, 0.5, 0.5]
    assert tindex.view(2, 3, 4, 5)[1].unique().tolist() == [1.0] and tindex[:60].unique().tolist() == [0.0]


# ---- 2. the header on the host -----------------------------------------------------------------------------------------
def test_occ_at_math_host_program(tmp_path):
    exe = tmp_path / "occ_at_host"
    base = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", f"-I{ROOT / 'vidar_amd' / 'csrc'}",
            str(ROOT / "tests" / "occ_at_host.cpp"), "-o", str(exe)]
    # a stand-alone program with its own main: the host sanitizers apply when the toolchain ships their runtimes
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.run(base, check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    print(run.stdout)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    assert "7200 queries" in run.stdout and "\n0 checks missed" in run.stdout


# ---- 3. the definition on the plane volume -----------------------------------------------------------------------------
def test_plane_volume_free_before_occupied_in_nothing_behind():
    """frame 0 looks along +x from x = 2.5 at the layer x = 40 of logit 14 in a volume of -2; K = 512, step 0.2, extent 1.
    Interior rows only: rows next to the y / z faces mix in padding."""
    q = VC.dense("plane", 512, 0.2)
    grid = q.want64[1.0].view(RS.F_, RS.Z, RS.Y, RS.X, 2)[0]
    ev = grid.sum(-1)
    occ = grid[..., 0] / ev
    row_occ, row_ev = occ[2, 5], ev[2, 5]
    print(f"row z=2 y=5: occ[30] {row_occ[30]:.3e} occ[40] {row_occ[40]:.5f} ev[40] {row_ev[40]:.5f} ev[41] {row_ev[41]:.3e}")
    assert float(row_occ[30]) == pytest.approx(1.3e-6, rel=0.05)
    assert float(row_occ[40]) == pytest.approx(0.9995, abs=1e-4)
    assert float(row_ev[40]) == pytest.approx(1.000, abs=1e-3)
    assert float(row_ev[41]) == pytest.approx(5.2e-4, rel=0.05)
    # the rows about the origin's (y = 5.2, z = 2.1), from x = 25 on: their rays reach the layer well inside the volume (a
    # ray that leaves through a side first never meets it, and its softmax spreads over the few waypoints it has)
    inner = (slice(1, 3), slice(4, 7))
    assert float(occ[inner][..., 25:39].max()) < 1e-4                 # free all the way to the layer
    assert float(ev[inner][..., 25:39].min()) > 0.999                 # and seen: the ray still has its mass there
    assert float(occ[inner][..., 40].min()) > 0.99
    assert float(ev[inner][..., 42:80].max()) < 1e-3                  # behind the layer the mass is spent: unseen
    from vidar_amd import forecast as FC
    answer, _ = FC.occupancy_grid(grid[..., 0], grid[..., 1], 0.5)
    assert bool(torch.isnan(answer[inner][..., 42:80]).all()) and not bool(torch.isnan(answer[inner][..., 25:41]).any())


# ---- 4. properties -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,K,step", [("randn", 37, 1.0), ("const", 65, 0.25), ("plane", 512, 1.0)],
                         ids=["randn-K37", "const-K65", "plane-K512"])
def test_ranges_and_exact_zeros_beyond_the_marched_range(kind, K, step):
    q = VC.dense(kind, K, step)
    for want in (q.want32[1.0], q.want64[1.0]):
        assert bool((want >= 0).all()) and float(want.sum(1).max()) <= 1 + 1e-6
    beyond = q.L64 - 0.5 >= K * step
    if (K, step) == (37, 1.0):
        assert 0.55 < float(beyond.float().mean()) < 0.61             # 58 % of the voxels
    assert float(q.want64[1.0][beyond].abs().max() if beyond.any() else 0.0) == 0.0
    assert int((~q.has_live).sum()) == 0 or float(q.want64[1.0][~q.has_live].abs().max()) == 0.0


def test_answers_are_continuous_in_the_length():
    """piecewise linear in L with slopes of at most max p / step: queries 1e-4 apart along one ray differ by little, also
    across the boundaries of the waypoints' stretches"""
    sigma = RS.volume("randn").double()
    origin = RS.rays()[0]
    d = torch.tensor([1.0, 0.1, 0.01], dtype=torch.float64)
    d = d / d.norm()
    L = torch.cat([torch.arange(2.0, 12.0, 0.25, dtype=torch.float64) + off for off in (-1e-4, 0.0, 1e-4)])
    pts = origin[0].double() + d * L.view(-1, 1)
    z, _, _ = VC.query_logits(sigma, origin, pts.float(), torch.zeros(len(L)), 64, 0.5)
    got = VC.query(z[:1].expand(len(L), -1), L, 0.5, 1.0).view(3, -1, 2)    # one ray's logits, the exact lengths
    assert float((got[1] - got[0]).abs().max()) < 1e-4 / 0.5 and float((got[2] - got[1]).abs().max()) < 1e-4 / 0.5


# ---- 5. the exclusion cap ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,K,step", VC.CASES, ids=VC.CASE_IDS)
def test_exclusion_cap(kind, K, step):
    """queries whose fp32 and fp64 live sets differ are left out of the precision comparison: at most 2 of the listed rays
    and 0.1 % of the voxels.  If a case breaks the cap, change the case, not the cap."""
    listed, dense = VC.listed(kind, K, step), VC.dense(kind, K, step)
    print(f"listed: excluded {listed.excluded()} of {int(listed.candidates().sum())}; dense: excluded {dense.excluded()} "
          f"of {int(dense.candidates().sum())}; yardstick listed "
          + ", ".join(f"{e}: {listed.yardstick(e)[0]:.1e} / {listed.yardstick(e)[1]:.1e}" for e in VC.EXTENTS)
          + f"; dense {dense.yardstick(1.0)[0]:.1e} / {dense.yardstick(1.0)[1]:.1e}")
    assert int(listed.candidates().sum()) == 128 and listed.excluded() <= VC.MAX_EXCLUDED_RAYS
    n = RS.F_ * RS.Z * RS.Y * RS.X
    assert int(dense.candidates().sum()) == n and dense.excluded() <= VC.MAX_EXCLUDED_VOXELS * n
    assert all(y > 0 for e in VC.EXTENTS for y in listed.yardstick(e)) and all(y > 0 for y in dense.yardstick(1.0))


# ---- 6. plumbing -------------------------------------------------------------------------------------------------------
def test_header_prototypes_equal_the_abi_rows():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "vidar_hip.h").read_text(), flags=re.S)
    protos = {name: (ret, [p.strip() for p in params.split(",")])
              for ret, name, params in re.findall(r"\b(\w+)\s+(vidar_(?:point|voxel)_occupancy\w*)\s*\(([^()]*)\)\s*;", text)}
    assert sorted(protos) == ["vidar_point_occupancy_f32", "vidar_voxel_occupancy_f32"]
    tail = ["int Z", "int Y", "int X", "int K", "float step", "float extent", "void* stream"]
    assert protos["vidar_point_occupancy_f32"] == ("int", [
        "const float* sigma", "const float* origin", "const float* pts", "const float* tindex", "float* out", "int F",
        "int R"] + tail)
    assert protos["vidar_voxel_occupancy_f32"] == ("int", [
        "const float* sigma", "const float* origin", "float* hit", "float* free_", "int F"] + tail)
    from vidar_amd import _lib
    assert _lib._ABI["vidar_point_occupancy_f32"] == "i 5p 6i 2f p"
    assert _lib._ABI["vidar_voxel_occupancy_f32"] == "i 4p 5i 2f p"
    assert not any(n.startswith("vidar_ray_occupancy") for n in protos)
    assert not re.search(r"size_t\s+vidar_(point|voxel)_occupancy", text)          # no workspace, no query


def test_entries_check_their_arguments_before_any_gpu_call():
    from vidar_amd._lib import BAD_ARG, lib
    L = lib()
    fake = 4096                                                       # a non-NULL address that is never dereferenced

    def point(F=2, R=8, Z=16, Y=200, X=200, K=512, extent=1.0, ptrs=(fake,) * 5):
        return L.vidar_point_occupancy_f32(*ptrs, F, R, Z, Y, X, K, 1.0, extent, None)

    def voxel(F=2, Z=16, Y=200, X=200, K=512, extent=1.0, ptrs=(fake,) * 4):
        return L.vidar_voxel_occupancy_f32(*ptrs, F, Z, Y, X, K, 1.0, extent, None)

    bad_extents = (0.0, -1.0, float("nan"), float("inf"), float("-inf"))
    for kw in [dict(K=0), dict(K=L.vidar_ray_max_k() + 1), dict(F=0), dict(F=-1), dict(R=-1), dict(Z=0), dict(Y=0),
               dict(X=0)] + [dict(extent=e) for e in bad_extents]:
        assert point(**kw) == BAD_ARG, kw
    for kw in [dict(K=0), dict(K=L.vidar_ray_max_k() + 1), dict(F=-1), dict(Z=0), dict(Y=0), dict(X=0),
               dict(F=60, Z=600, Y=600, X=600)] + [dict(extent=e) for e in bad_extents]:      # beyond the 32-bit ray index
        assert voxel(**kw) == BAD_ARG, kw
    for i in range(5):                                                # a NULL pointer with work to do
        assert point(ptrs=tuple(None if j == i else fake for j in range(5))) == BAD_ARG, i
    for i in range(4):
        assert voxel(ptrs=tuple(None if j == i else fake for j in range(4))) == BAD_ARG, i
    # the empty problems succeed, whatever the pointers, and a bad argument is still one
    assert point(R=0) == 0 and point(R=0, ptrs=(None,) * 5) == 0 and point(R=0, K=0) == BAD_ARG
    assert point(R=0, extent=0.0) == BAD_ARG
    assert voxel(F=0) == 0 and voxel(F=0, ptrs=(None,) * 4) == 0 and voxel(F=0, K=0) == BAD_ARG


class _StubHead(torch.nn.Module):
    EVIDENCE = torch.tensor([[0.6, 0.0], [0.2, 0.2], [0.0, 1.0], [0.0, 0.0]]).t().reshape(1, 1, 2, 1, 2, 2)

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
        self.calls.append(("occupancy", directions is not None, end_points is not None, cameras))
        return self.EVIDENCE.clone() * 3

    def render_occupancy_dense(self, pred_dict, *, extent=1.0, img_metas=None, **geom):
        assert sorted(geom) == ["tgt_bev_h", "tgt_bev_w", "tgt_pc_range"] and extent == 1.0
        self.calls.append(("dense", img_metas))
        return self.EVIDENCE.clone()

    def measured_occupancy(self, pred_dict, gt_points, **geom):
        self.calls.append("measured")
        return self.EVIDENCE.clone() * 5


METAS = [dict(sample_idx="tok7")]


def _stub_detector():
    from vidar_amd.plugin.detectors.vidar import ViDAR
    det = ViDAR.__new__(ViDAR)
    torch.nn.Module.__init__(det)
    det.future_pred_head = _StubHead()
    det.point_cloud_range = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
    det.bev_h = det.bev_w = 2
    det._future_pred_dict = lambda img_metas, img=None, img_feats=None: (
        dict(valid_frames=[0], next_bev_preds=torch.zeros(1, 1, 1, 4, 1)), METAS)
    return det


def test_forecast_dense_needs_no_rays_and_calls_the_dense_method_once():
    det = _stub_detector()
    head = det.future_pred_head

    def forecast(**kw):
        head.calls.clear()
        return det.forecast(img=torch.zeros(1, 1), img_metas=[None], **kw), list(head.calls)
    out, calls = forecast(occupancy="dense")                          # neither rays nor cameras
    assert calls == [("dense", METAS)] and sorted(out) == ["evidence", "occupancy", "valid_frames"]
    assert torch.equal(out["evidence"], _StubHead.EVIDENCE)
    occ = out["occupancy"].view(-1)
    assert out["occupancy"].shape == (1, 1, 1, 2, 2)
    assert occ[0] == 1.0 and math.isnan(occ[1]) and occ[2] == 0.0 and math.isnan(occ[3])
    assert forecast(occupancy="dense", min_evidence=0.3)[0]["occupancy"].view(-1)[1] == 0.5
    # next to the other outputs: they keep their bits, and the dense method is still called once
    rays = torch.zeros(4, 3)
    plain, calls = forecast(rays=rays, cameras="all", stride=8)
    assert calls == ["rays", "cameras"]
    out, calls = forecast(rays=rays, cameras="all", stride=8, occupancy="dense")
    assert calls == ["rays", "cameras", ("dense", METAS)]
    assert sorted(out) == sorted(list(plain) + ["evidence", "occupancy"])
    assert torch.equal(out["depth"], plain["depth"]) and torch.equal(out["sweep"][0][0], plain["sweep"][0][0])
    # the ray sources are what they were
    out, calls = forecast(rays=rays, occupancy=True)
    assert calls == ["rays", ("occupancy", True, False, None)] and torch.equal(out["evidence"], _StubHead.EVIDENCE * 3)
    for bad in (dict(occupancy="voxels"), dict(occupancy="Dense"), dict(occupancy="lidar"), dict(occupancy="sweep"),
                dict(occupancy="cameras"), dict(occupancy="both", rays=rays)):
        with pytest.raises(ValueError):
            forecast(**bad)


def test_occupancy_metrics_source(monkeypatch):
    from vidar_amd import forecast as FC
    from vidar_amd.plugin.utils import eval_utils
    det = _stub_detector()
    head = det.future_pred_head
    seen = []

    def score(pred, meas, **kw):
        seen.append((pred.clone(), meas.clone(), kw))
        return torch.zeros(1, 1, len(FC.occupancy_columns(kw.get("thresholds", FC.OCC_THRESHOLDS), kw.get("bins", FC.OCC_BINS))))
    monkeypatch.setattr(FC, "occupancy_score", score)
    monkeypatch.delenv("VIDAR_OCC_METRICS", raising=False)
    gt = [torch.zeros(3, 4)]

    def table():
        head.calls.clear(); seen.clear()
        options = eval_utils.occupancy_metrics()
        _, names = det._occupancy_table(dict(valid_frames=[0]), gt, METAS, options)
        return list(head.calls), seen[0], names, options
    try:
        eval_utils.set_occupancy_metrics(True, thresholds=(0.3,), bins=4)             # the default source: today's calls
        calls, (pred, meas, kw), names, options = table()
        assert options == dict(thresholds=(0.3,), bins=4)
        assert calls == [("occupancy", False, True, None), "measured"]
        assert torch.equal(pred, _StubHead.EVIDENCE * 3) and torch.equal(meas, _StubHead.EVIDENCE * 5)
        assert kw == dict(thresholds=(0.3,), bins=4) and names == FC.occupancy_columns((0.3,), 4)
        eval_utils.set_occupancy_metrics(True, source="rays", min_evidence=0.25)
        assert eval_utils.occupancy_metrics() == dict(min_evidence=0.25)
        assert table()[0] == [("occupancy", False, True, None), "measured"]

        eval_utils.set_occupancy_metrics(True, source="dense", thresholds=(0.3,), min_evidence=0.25)
        calls, (pred, meas, kw), names, options = table()
        assert calls == [("dense", METAS), "measured"]
        assert torch.equal(pred, _StubHead.EVIDENCE) and torch.equal(meas, _StubHead.EVIDENCE * 5)
        assert kw == dict(thresholds=(0.3,), min_evidence=0.25) and "source" not in kw
        assert names == FC.occupancy_columns((0.3,), FC.OCC_BINS)
        assert options["source"] == "dense"                           # _occupancy_table left the caller's dict alone

        for bad in ("voxels", None, "Dense"):
            with pytest.raises(ValueError):
                eval_utils.set_occupancy_metrics(True, source=bad)
        with pytest.raises(TypeError):
            eval_utils.set_occupancy_metrics(True, source="dense", threshold=0.3)
        assert eval_utils.occupancy_metrics()["source"] == "dense"    # a refused call changes nothing
        eval_utils.set_occupancy_metrics(True)
        assert eval_utils.occupancy_metrics() == {}                   # and the source does not stick
    finally:
        eval_utils.set_occupancy_metrics(None)


def test_command_line_tools_know_the_dense_source():
    for tool, flag in (("forecast.py", "--occupancy"), ("test.py", "--occ-source")):
        text = (ROOT / "tools" / tool).read_text()
        m = re.search(r'add_argument\("%s".*?choices=\[([^\]]*)\]' % re.escape(flag), text, flags=re.S)
        assert m and '"dense"' in m.group(1), tool
