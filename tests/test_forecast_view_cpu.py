"""CPU: the pictures and the geometry helpers of vidar_amd/forecast.py against plain Python loops (exact to the byte),
the `_viz_pcd_flag` files of ViDAR.forward_test through a stubbed decode, the new entry points' argument checks (no GPU
call is reached), and csrc/cam_ray.h -- the pixel -> ray function both camera kernels inline -- compiled into the
stand-alone host program tests/cam_ray_host.cpp (under the host sanitizers where the toolchain has them) against fp64."""
import math
import os
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from vidar_amd import forecast as FC

ROOT = Path(__file__).resolve().parents[1]
SIZE = 64
WHITE = (255, 255, 255)


# ---- bev_image ---------------------------------------------------------------------------------------------------
def loop_pixel(x, y, size, limit):
    """(row, col) or None: the floor of the position in pixel units, y up; the window is [-limit, limit)"""
    if not (math.isfinite(x) and math.isfinite(y)):        # NaN is skipped; an infinite point is outside any window
        return None
    col = math.floor((x + limit) / (2.0 * limit) * size)
    up = math.floor((y + limit) / (2.0 * limit) * size)
    if not (0 <= col < size and 0 <= up < size):
        return None
    return size - 1 - up, col


def loop_cross(img, at, arm, colour):
    if at is None:
        return
    size = len(img)
    for k in range(-arm, arm + 1):
        for r, c in ((at[0] + k, at[1] + k), (at[0] + k, at[1] - k)):
            if 0 <= r < size and 0 <= c < size:
                img[r][c] = colour


def loop_bev(points, labels, centres, size, limit):
    img = [[WHITE for _ in range(size)] for _ in range(size)]
    for p, lab in zip(points, labels):                 # in order: a later point paints over an earlier one
        at = loop_pixel(float(p[0]), float(p[1]), size, limit)
        if at is not None:
            img[at[0]][at[1]] = FC.LABEL_COLOURS[lab]
    arm = max(2, size // 64)
    for c in centres:
        loop_cross(img, loop_pixel(float(c[0]), float(c[1]), size, limit), arm, FC.LABEL_COLOURS[0])
    loop_cross(img, loop_pixel(0.0, 0.0, size, limit), arm, FC.LABEL_COLOURS[2])
    return np.array(img, dtype=np.uint8)


def bev_case():
    g = torch.Generator().manual_seed(5)
    limit = 40.0
    pts = (torch.rand(400, 3, generator=g) * 2 - 1) * 48.0            # a fifth falls outside the window
    lab = torch.randint(0, 3, (400,), generator=g)
    cell = 2 * limit / SIZE
    # overlapping points of different labels in ONE pixel, in both orders: the later one wins
    same = torch.tensor([[10.1, 10.1, 0.0], [10.2, 10.3, 0.0], [10.3, 10.2, 0.0],
                         [-20.1, 5.1, 0.0], [-20.2, 5.2, 0.0]])
    assert len({loop_pixel(float(p[0]), float(p[1]), SIZE, limit) for p in same[:3]}) == 1
    assert len({loop_pixel(float(p[0]), float(p[1]), SIZE, limit) for p in same[3:]}) == 1
    same_lab = torch.tensor([0, 1, 2, 1, 0])
    # on and outside the window edge: -limit is inside (closed), +limit outside (open), a cell border, far away
    edge = torch.tensor([[-limit, -limit, 0.0], [limit, 0.0, 0.0], [0.0, limit, 0.0], [-limit, limit - 1e-3, 0.0],
                         [limit - 1e-3, -limit, 0.0], [3 * cell, -7 * cell, 0.0], [-limit - 1e-3, 0.0, 0.0],
                         [1e9, 1e9, 0.0], [-1e9, 3.0, 0.0]])
    edge_lab = torch.tensor([1, 1, 1, 0, 2, 1, 0, 0, 0])
    nan = torch.tensor([[float("nan"), 1.0, 0.0], [1.0, float("nan"), 0.0], [float("nan"), float("nan"), 0.0],
                        [float("inf"), 0.0, 0.0]])
    nan_lab = torch.tensor([0, 1, 2, 1])
    # the first `same` pixel is painted again at the very end by an early-label point
    again = same[:1].clone()
    points = torch.cat([pts[:200], same, edge, nan, pts[200:], again])
    labels = torch.cat([lab[:200], same_lab, edge_lab, nan_lab, lab[200:], torch.tensor([1])])
    return points, labels, limit


@pytest.mark.parametrize("centre", [None, [[12.5, -30.0, 0.0]], [[39.9, 39.9, 1.0], [-100.0, 0.0, 0.0]]],
                         ids=["no-centre", "centre", "corner-and-outside"])
def test_bev_image_equals_the_plain_loop(centre):
    points, labels, limit = bev_case()
    ctr = None if centre is None else torch.tensor(centre)
    got = FC.bev_image(points, labels, ctr, SIZE, limit)
    assert got.dtype == torch.uint8 and got.shape == (SIZE, SIZE, 3)
    want = loop_bev(points.tolist(), labels.tolist(), centre or [], SIZE, limit)
    np.testing.assert_array_equal(got.numpy(), want)
    # the picture is not trivially white, and all three label colours made it
    for colour in FC.LABEL_COLOURS:
        assert (want.reshape(-1, 3) == np.array(colour, np.uint8)).all(1).any()


def test_bev_image_later_point_wins_and_edges():
    limit = 40.0
    pts = torch.tensor([[10.1, 10.1, 0.0], [10.2, 10.3, 0.0], [10.3, 10.2, 0.0], [-limit, -limit, 0.0],
                        [limit, limit, 0.0], [float("nan"), 0.0, 0.0]])
    lab = torch.tensor([0, 2, 1, 1, 1, 0])
    img = FC.bev_image(pts, lab, None, SIZE, limit).numpy()
    r, c = loop_pixel(10.1, 10.1, SIZE, limit)
    assert tuple(img[r, c]) == FC.LABEL_COLOURS[1]                    # the last of the three
    assert tuple(img[SIZE - 1, 0]) == FC.LABEL_COLOURS[1]             # (-limit, -limit): bottom-left pixel
    assert tuple(img[0, SIZE - 1]) == WHITE                           # (+limit, +limit) is outside
    painted = (img.reshape(-1, 3) != 255).any(1).sum()
    arm = max(2, SIZE // 64)
    assert painted == 2 + (4 * arm + 1)                               # two point pixels + the red cross at (0, 0)
    empty = FC.bev_image(torch.zeros(0, 3), torch.zeros(0, dtype=torch.int64), None, SIZE, limit).numpy()
    assert (empty.reshape(-1, 3) != 255).any(1).sum() == 4 * arm + 1


# ---- depth_overlay -----------------------------------------------------------------------------------------------
def loop_table():
    return [tuple(min(255, max(0, 384 - abs(4 * i - peak))) for peak in (768, 512, 256)) for i in range(256)]


def loop_overlay(depth, frame, near, far, alpha):
    H, W = len(frame), len(frame[0])
    Hs = len(depth)
    s = -(-H // Hs)
    table = loop_table()
    out = [[None] * W for _ in range(H)]
    for y in range(H):
        for x in range(W):
            d = depth[y // s][x // s]
            px = frame[y][x]
            if math.isnan(d) or math.isinf(d) or d <= 0:
                out[y][x] = tuple(px)
                continue
            i = min(255, max(0, math.floor((far - d) / (far - near) * 255.0 + 0.5)))
            out[y][x] = tuple((alpha * c + (255 - alpha) * p + 127) // 255 for c, p in zip(table[i], px))
    return np.array(out, dtype=np.uint8)


@pytest.mark.parametrize("stride,alpha", [(1, 160), (4, 160), (3, 255), (5, 0), (4, 1)])
def test_depth_overlay_equals_the_plain_loop(stride, alpha):
    g = torch.Generator().manual_seed(stride)
    H = W = SIZE
    Hs = -(-H // stride)
    frame = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
    near, far = 1.0, 60.0
    depth = torch.rand(Hs, Hs, generator=g, dtype=torch.float64).float() * 80.0 - 5.0     # below near, beyond far, negative
    depth[0, 0] = 0.0; depth[1, 2] = float("nan"); depth[2, 1] = float("inf")
    depth[3, 3] = near; depth[4, 4] = far; depth[5, 5] = (near + far) / 2
    got = FC.depth_overlay(depth, frame, near, far, alpha)
    assert got.dtype == torch.uint8 and got.shape == (H, W, 3)
    want = loop_overlay(depth.double().tolist(), frame.tolist(), near, far, alpha)
    np.testing.assert_array_equal(got.numpy(), want)
    if alpha == 0:
        assert torch.equal(got, frame)
    assert torch.equal(got[0, 0], frame[0, 0])                        # no return: the image shows


def test_colour_table_and_bad_grids():
    np.testing.assert_array_equal(FC.colour_table().numpy(), np.array(loop_table(), np.uint8))
    frame = torch.zeros(SIZE, SIZE, 3, dtype=torch.uint8)
    with pytest.raises(ValueError):
        FC.depth_overlay(torch.ones(15, 16), frame)                   # 64 / 4 = 16 rows
    with pytest.raises(ValueError):
        FC.depth_overlay(torch.ones(16, 16), frame, alpha=256)
    with pytest.raises(ValueError):
        FC.depth_overlay(torch.ones(16, 16), frame, near=5.0, far=5.0)


# ---- lidar_pattern / pix2vox ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("beams,az,elev", [(32, 1080, (-30.67, 10.67)), (4, 16, (-30.67, 10.67)), (1, 7, (-5.0, 5.0)),
                                           (3, 1, (-90.0, 90.0))])
def test_lidar_pattern(beams, az, elev):
    d = FC.lidar_pattern(beams, az, elev)
    assert d.shape == (beams * az, 3) and d.dtype == torch.float32
    np.testing.assert_allclose(d.double().norm(dim=1).numpy(), 1.0, atol=2 ** -22)
    el = torch.rad2deg(torch.asin(d[:, 2].double().clamp(-1, 1))).view(beams, az)
    assert float(el.min()) >= elev[0] - 1e-4 and float(el.max()) <= elev[1] + 1e-4
    assert float((el - el[:, :1]).abs().max()) < 1e-4                 # beam-major: one elevation per beam
    if beams > 1:
        np.testing.assert_allclose(el[:, 0].numpy(), np.linspace(elev[0], elev[1], beams), atol=1e-4)
    if abs(elev[0]) < 89 and az > 1:
        a = torch.atan2(d[:, 1].double(), d[:, 0].double()).view(beams, az)
        assert float(a.min()) >= -math.pi - 1e-6 and float(a.max()) < math.pi
        gaps = (a[:, 1:] - a[:, :-1])
        np.testing.assert_allclose(gaps.numpy(), 2 * math.pi / az, atol=1e-5)   # evenly spaced, increasing


def test_lidar_pattern_defaults_and_bad_arguments():
    assert FC.lidar_pattern().shape == (32 * 1080, 3)
    with pytest.raises(ValueError):
        FC.lidar_pattern(0, 4)


def test_pix2vox_inverts_the_projection_in_fp64():
    from vidar_amd.synthetic import PC_RANGE, camera_matrices, metric_to_voxel
    l2i = camera_matrices()[:3]
    m = FC.pix2vox(l2i, PC_RANGE, 200, 200, 16)
    assert m.shape == (1, 3, 4, 4) and m.dtype == torch.float32
    rng = np.random.default_rng(0)
    xyz = rng.uniform(-30, 30, (50, 3))
    for c in range(3):
        pix = (l2i[c] @ np.concatenate([xyz, np.ones((50, 1))], 1).T).T          # (u d, v d, d, 1)
        vox = (m[0, c].double().numpy() @ pix.T).T[:, :3]
        np.testing.assert_allclose(vox, metric_to_voxel(xyz.astype(np.float32), 200, 200, 16), atol=2e-2)
    with pytest.raises(ValueError):
        bad = l2i.copy(); bad[0, 3, 2] = 1.0
        FC.pix2vox(bad, PC_RANGE, 200, 200, 16)


# ---- _viz_pcd_flag ---------------------------------------------------------------------------------------------------
class _StubHead(torch.nn.Module):
    """stands in for the future-prediction head: two frames of known points, one ground-truth point out of range"""
    def __init__(self):
        super().__init__()
        self.bev_pred_head = [None]

    def get_point_cloud_prediction(self, pred_dict, gt_points, *a, **kw):
        gt = torch.tensor([[5.0, 5.0, 0.0], [-10.0, 20.0, 0.0], [500.0, 0.0, 0.0]])
        pred = gt + torch.tensor([1.0, -1.0, 0.0])
        return dict(pred_pcds=[[pred, pred * 0.5]], gt_pcds=[[gt, gt * 0.5]], origin=torch.zeros(1, 2, 3))


def _stub_detector(tmp_path, flag):
    from vidar_amd.plugin.detectors.vidar import ViDAR
    det = ViDAR.__new__(ViDAR)
    torch.nn.Module.__init__(det)
    det.future_pred_head = _StubHead()
    det.point_cloud_range = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
    det.bev_h = det.bev_w = 8
    det._submission = False
    det._viz_pcd_flag = flag
    det._viz_pcd_path = str(tmp_path / "dbg" / "pred_pcd")
    det._future_pred_dict = lambda img_metas, img=None, img_feats=None: (
        dict(valid_frames=[0, 1]), [dict(sample_idx="tok7")])
    return det


def test_viz_pcd_flag_writes_the_named_files(tmp_path, monkeypatch):
    from PIL import Image
    from vidar_amd.plugin.utils import e2e_predictor_utils as U, eval_utils
    monkeypatch.setattr(U, "compute_chamfer_distance_inner", lambda *a, **k: 0.0)
    monkeypatch.setattr(eval_utils, "compute_ray_errors", lambda *a, **k: (0.0, 0.0))
    monkeypatch.setattr(eval_utils, "device_metrics", lambda: False)
    off = _stub_detector(tmp_path / "off", False)
    res_off = off.forward_test([None], img=torch.zeros(1, 1))
    assert not (tmp_path / "off").exists()                                 # flag off: nothing is written
    on = _stub_detector(tmp_path / "on", True)
    res_on = on.forward_test([None], img=torch.zeros(1, 1))
    assert res_on == res_off                                               # the metrics do not change
    files = sorted(p.name for p in (tmp_path / "on" / "dbg").iterdir())
    assert files == ["pred_pcd_tok7_0.png", "pred_pcd_tok7_1.png"]
    # the picture: prediction and ground truth of the rays whose GT point is inside the range, GT painted last
    d = on.future_pred_head.get_point_cloud_prediction(None, None)
    for f in range(2):
        pred, gt = d["pred_pcds"][0][f], d["gt_pcds"][0][f]
        inside = U.get_inside_mask(gt, on.point_cloud_range)
        assert inside.tolist() == [True, True, False]
        want = FC.sweep_bev(pred[inside], gt[inside], centre=torch.zeros(1, 3))
        got = np.asarray(Image.open(tmp_path / "on" / "dbg" / f"pred_pcd_tok7_{f}.png").convert("RGB"))
        np.testing.assert_array_equal(got, want.numpy())
        colours = {tuple(c) for c in got.reshape(-1, 3).tolist()}
        assert set(FC.LABEL_COLOURS) | {WHITE} == colours


def test_constructor_keeps_the_viz_arguments():
    import inspect
    from vidar_amd.plugin.detectors.vidar import ViDAR
    src = inspect.getsource(ViDAR.__init__)
    assert "self._viz_pcd_flag = _viz_pcd_flag" in src and "self._viz_pcd_path = _viz_pcd_path" in src


# ---- the entry points without a GPU ------------------------------------------------------------------------------------
def test_camera_entry_points_check_their_arguments_before_any_gpu_call():
    from vidar_amd._lib import BAD_ARG, lib
    L = lib()
    cam = L.vidar_ray_argmax_cam_f32
    rays = L.vidar_cam_rays_f32
    good = dict(F=2, C=6, Hs=225, Ws=400, u0=2.0, v0=2.0, du=4.0, dv=4.0)

    def call_cam(K=512, Z=16, **kw):
        g = dict(good, **kw)
        return cam(None, None, None, g["F"], g["C"], g["Hs"], g["Ws"], g["u0"], g["v0"], g["du"], g["dv"], Z, 200, 200,
                   K, 1.0, None)

    def call_rays(**kw):
        g = dict(good, **kw)
        return rays(None, None, None, g["F"], g["C"], g["Hs"], g["Ws"], g["u0"], g["v0"], g["du"], g["dv"], None)

    assert call_cam(Hs=0) == 0 and call_cam(Ws=0) == 0 and call_rays(Hs=0) == 0        # empty grid: no launch
    for kw in (dict(F=0), dict(C=0), dict(Hs=-1), dict(Ws=-1), dict(du=0.0), dict(dv=0.0), dict(u0=float("nan")),
               dict(dv=float("nan")), dict(F=6, C=6, Hs=9000, Ws=16000)):                # 5.2e9 rays: beyond 2^31
        assert call_cam(**kw) == BAD_ARG, kw
        assert call_rays(**kw) == BAD_ARG, kw
    assert call_cam(K=0, Hs=0) == BAD_ARG and call_cam(K=L.vidar_ray_max_k() + 1, Hs=0) == BAD_ARG
    assert call_cam(Z=0, Hs=0) == BAD_ARG


def test_camera_kernels_are_in_the_library():
    import sys
    sys.path.insert(0, str(ROOT / "tools"))
    import kernel_resources
    from vidar_amd import build
    by = {r["kernel"]: r for r in kernel_resources.table(build.build(verbose=False))}
    for name in ("ray_argmax_cam_kernel", "ray_argmax_cam_any_kernel", "cam_rays_kernel"):
        assert name in by, name
        assert by[name]["scratch"] == 0 and by[name]["vgpr_spill"] == 0


# ---- csrc/cam_ray.h on the host ------------------------------------------------------------------------------------
def build_host_program(directory):
    exe = Path(directory) / "cam_ray_host"
    base = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", f"-I{ROOT / 'vidar_amd' / 'csrc'}",
            str(ROOT / "tests" / "cam_ray_host.cpp"), "-o", str(exe)]
    # a stand-alone program with its own main: the host sanitizers apply when the toolchain ships their runtimes
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.run(base, check=True)
    return exe


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    return build_host_program(tmp_path_factory.mktemp("cam_ray_host"))


def run_host(exe, tmp, pix2vox, hw, u0, v0, du, dv):
    """-> (origin [F,C,3], pts [F,C,Hs,Ws,3]) float32, what vidar_cam_rays_f32 writes"""
    F_, C = pix2vox.shape[:2]
    Hs, Ws = hw
    src, dst = Path(tmp) / "cam_in.bin", Path(tmp) / "cam_out.bin"
    src.write_bytes(struct.pack("<4i4f", F_, C, Hs, Ws, u0, v0, du, dv) + np.ascontiguousarray(pix2vox, "<f4").tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stderr[-2000:]
    data = np.frombuffer(dst.read_bytes(), "<f4")
    n = F_ * C
    assert data.size == n * 3 + n * Hs * Ws * 3
    return data[:n * 3].reshape(F_, C, 3).copy(), data[n * 3:].reshape(F_, C, Hs, Ws, 3).copy()


def test_pixel_ray_on_the_host_against_fp64(host_program, tmp_path):
    """the geometries of tests/test_forecast_view_gpu.py (forecast_view_cases.py): every end point within the fp32
    rounding of its four-term sum, the origin exact, unwritten output would show as NaN"""
    from forecast_view_cases import GRIDS, camera_set
    m32 = camera_set().numpy()
    m = m32.astype(np.float64)
    for (Hs, Ws, u0, v0, du, dv) in GRIDS:
        origin, pts = run_host(host_program, tmp_path, m32, (Hs, Ws), u0, v0, du, dv)
        np.testing.assert_array_equal(origin, m32[..., :3, 3])
        u = np.float32(u0) + np.arange(Ws, dtype=np.float32) * np.float32(du)       # fp32, as the function forms them
        v = np.float32(v0) + np.arange(Hs, dtype=np.float32) * np.float32(dv)
        uu, vv = np.meshgrid(u.astype(np.float64), v.astype(np.float64))
        pix = np.stack([uu, vv, np.ones_like(uu), np.ones_like(uu)], -1)           # [Hs, Ws, 4]
        want = np.einsum("fcij,yxj->fcyxi", m[..., :3, :], pix)
        # 2 products + 3 sums, each within half an ulp of a partial sum no larger than the sum of magnitudes
        mag = np.einsum("fcij,yxj->fcyxi", np.abs(m[..., :3, :]), np.abs(pix))
        assert np.isfinite(pts).all()
        assert (np.abs(pts - want) <= 5 * 2.0 ** -24 * mag).all()
