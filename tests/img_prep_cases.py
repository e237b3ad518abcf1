"""Shared inputs of tests/test_img_prep_cpu.py and tests/test_img_prep_gpu.py (no tests in here): the adversarial
photometric image and parameter grid, `_distort` replayed with scripted draws, the host build of csrc/img_prep_math.h, and
a small nuScenes-like fixture on disk."""
import ctypes
import itertools
import pickle
import subprocess
from pathlib import Path
from unittest import mock

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "vidar_amd" / "csrc" / "img_prep_math.h"

# Largest |host build of img_prep_math.h - reader.normalise_pad(scale=2/3)| over the 45 x 80 and 37 x 53 cases of the
# tests (caffe mean, std 1), measured by test_scaled_host_build_against_normalise_pad and recorded in DESIGN.md.  The GPU
# test's absolute bound is four times this (a different summation order of the four taps); anything above 1e-3 would mean
# a wrong source index, not rounding.
SCALED_HOST_DIFF = 1.52587890625e-05           # 2^-16: one ulp of a value in [128, 256)
SCALED_CASES = [(45, 80), (37, 53)]
CAFFE_MEAN, UNIT_STD = [103.530, 116.280, 123.675], [1.0, 1.0, 1.0]


def adversarial_image():
    """uint8 [32, 32, 3] BGR: grey (d == 0), black, pure primaries, channel ties, values the shift drives negative and the
    shift / gain drive above 255, hues within the turn (18 degrees) of 0 and of 360, noise for the rest"""
    px = []
    px += [(k, k, k) for k in (0, 1, 2, 17, 31, 32, 33, 100, 128, 200, 223, 224, 254, 255)]            # grey incl. black
    px += [(0, 0, 0)] * 4
    for v in (255, 128, 1):
        px += [(v, 0, 0), (0, v, 0), (0, 0, v), (v, v, 0), (0, v, v), (v, 0, v)]                          # primaries, ties
    px += [(200, 200, 10), (10, 200, 200), (200, 10, 200), (90, 90, 91), (91, 90, 90), (90, 91, 90),
           (255, 255, 254), (254, 255, 255), (5, 5, 6), (6, 5, 5)]                                         # ties of max / min
    px += [(b, g, r) for b in (0, 3, 20) for g in (0, 5, 31) for r in (1, 12, 30)]                        # negative after shift
    px += [(b, g, r) for b in (255, 240, 225) for g in (255, 250, 230) for r in (254, 235, 226)]          # above 255
    for r in (255, 200, 60):                                                                              # hue near 0 / 360
        for e in (1, 2, 5, 9, 15):
            lo = r // 4
            px += [(lo, lo + e, r), (lo + e, lo, r), (lo, min(lo + e * 3, r - 1), r), (min(lo + e * 3, r - 1), lo, r)]
    img = np.random.default_rng(7).integers(0, 256, (32 * 32, 3), dtype=np.uint8)
    assert len(px) <= len(img)
    img[:len(px)] = np.asarray(px, np.uint8)
    return img.reshape(32, 32, 3)


def photo_grid():
    """float32 [144, 12]: shift on/off x contrast none / before / after the HSV stage x saturation x hue x all six channel
    permutations, magnitudes spread over the released ranges (both signs)"""
    rng = np.random.default_rng(11)
    rows = []
    for k, (shift, contrast, sat, hue, perm) in enumerate(itertools.product(
            (0, 1), (0, 1, 2), (0, 1), (0, 1), itertools.permutations(range(3)))):
        row = np.zeros(12, np.float32)
        flags = 0
        if shift:
            row[0] = (-1) ** k * rng.uniform(20, 32); flags |= 1
        if contrast == 1:
            row[1] = rng.uniform(0.5, 1.5); flags |= 2
        if sat:
            row[2] = rng.uniform(0.5, 1.5); flags |= 4
        if hue:
            row[3] = (-1) ** (k // 2) * rng.uniform(1, 18); flags |= 8
        if contrast == 2:
            row[4] = rng.uniform(0.5, 1.5); flags |= 16
        row[5] = flags
        row[6:9] = perm
        rows.append(row)
    return np.stack(rows)


def replay_distort(img, row):
    """the EXISTING `PhotoMetricDistortionMultiViewImage._distort` with numpy's generator scripted to draw `row`"""
    from vidar_amd.data.augment import PhotoMetricDistortionMultiViewImage
    flags = int(row[5])
    coins, uniforms = [], []

    def coin_uniform(bit, k):
        coins.append(1 if flags & bit else 0)
        if flags & bit:
            uniforms.append(float(row[k]))
    coin_uniform(1, 0)
    first = bool(flags & 2) or not flags & 16
    coins.append(1 if first else 0)
    if first:
        coin_uniform(2, 1)
    coin_uniform(4, 2)
    coin_uniform(8, 3)
    if not first:
        coin_uniform(16, 4)
    coins.append(1)
    coins, uniforms = iter(coins), iter(uniforms)
    with mock.patch("numpy.random.randint", lambda *a, **k: next(coins)), \
            mock.patch("numpy.random.uniform", lambda *a, **k: next(uniforms)), \
            mock.patch("numpy.random.permutation", lambda n: np.asarray(row[6:9], np.int64)):
        out = PhotoMetricDistortionMultiViewImage()._distort(img)
    assert next(coins, None) is None and next(uniforms, None) is None
    return out


def host_cast_u8(x):
    """int(x) & 255 on every element (Python integers: the definition, not numpy's cast)"""
    flat = np.asarray(x, np.float32).ravel()
    return np.array([int(v) & 255 for v in flat.tolist()], np.uint8).reshape(np.shape(x))


def build_host_math(out_dir):
    """csrc/img_prep_math.h compiled for the host with -ffp-contract=off -> ctypes library"""
    so = Path(out_dir) / "libimg_prep_host.so"
    subprocess.run(["c++", "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared",
                    "-DVIDAR_IMG_PREP_HOST_BUILD", str(HEADER), "-o", str(so)], check=True)
    L = ctypes.CDLL(str(so))
    vp = ctypes.c_void_p
    L.vidar_img_host_photometric.argtypes = [vp, vp, vp, vp, ctypes.c_int, ctypes.c_long]
    L.vidar_img_host_photometric.restype = None
    L.vidar_img_host_normalise.argtypes = [vp, vp] + [ctypes.c_int] * 4 + [vp, vp, ctypes.c_int]
    L.vidar_img_host_normalise.restype = None
    return L


def host_photometric(L, imgs_u8, rows):
    imgs_u8 = np.ascontiguousarray(imgs_u8, np.uint8)
    rows = np.ascontiguousarray(rows, np.float32)
    f32 = np.empty(imgs_u8.shape, np.float32)
    u8 = np.empty(imgs_u8.shape, np.uint8)
    n = imgs_u8.shape[0]
    L.vidar_img_host_photometric(imgs_u8.ctypes.data, rows.ctypes.data, f32.ctypes.data, u8.ctypes.data, n,
                                 imgs_u8[0].size // 3)
    return f32, u8


def host_normalise(L, img_u8, oh, ow, mean, std, to_rgb):
    img_u8 = np.ascontiguousarray(img_u8, np.uint8)
    out = np.empty((3, oh, ow), np.float32)
    m, s = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    L.vidar_img_host_normalise(img_u8.ctypes.data, out.ctypes.data, img_u8.shape[0], img_u8.shape[1], oh, ow, m.ctypes.data,
                               s.ctypes.data, int(to_rgb))
    return out


def scaled_case(h, w):
    return np.random.default_rng(h * 1000 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)


def mini_dataset(root, n_frames=6, cams=3, hw=(45, 80), lo=80, hi=130):
    """one scene of `n_frames` frames on disk: lidar .bin files and `cams` PNG images of `hw` with every channel in
    [lo, hi] (any photometric draw then stays inside [0, 256): the host's uint8 cast is defined on every platform)"""
    from PIL import Image
    rng = np.random.default_rng(5)
    root = Path(root)
    infos = []
    for k in range(n_frames):
        lidar = root / f"lidar_{k}.bin"
        rng.uniform(-40, 40, (300, 5)).astype(np.float32).tofile(lidar)
        cam_infos = {}
        for c in range(cams):
            p = root / f"img_{k}_{c}.png"
            Image.fromarray(rng.integers(lo, hi + 1, (*hw, 3), dtype=np.uint8)).save(p)
            yaw = c * 2 * np.pi / cams
            cam_infos[f"CAM_{c}"] = dict(
                data_path=str(p), cam_intrinsic=np.array([[50.0, 0, hw[1] / 2], [0, 50.0, hw[0] / 2], [0, 0, 1]]),
                sensor2lidar_rotation=np.array([[np.cos(yaw), 0, np.sin(yaw)], [np.sin(yaw), 0, -np.cos(yaw)], [0, -1.0, 0]]),
                sensor2lidar_translation=np.array([0.5 * c, 0.0, 1.5]))
        a = 0.05 * k
        infos.append(dict(token=f"tok{k}", lidar_path=str(lidar), timestamp=int((100 + 0.5 * k) * 1e6), sweeps=[],
                          ego2global_translation=[2.0 * k, 0.3 * k, 0.0],
                          ego2global_rotation=[np.cos(a / 2), 0.0, 0.0, np.sin(a / 2)],
                          lidar2ego_translation=[0.9, 0.0, 1.8], lidar2ego_rotation=[1.0, 0.0, 0.0, 0.0],
                          prev="" if k == 0 else f"tok{k - 1}", next="" if k == n_frames - 1 else f"tok{k + 1}",
                          scene_token="scene-a", can_bus=np.zeros(18), frame_idx=k, cams=cam_infos))
    with open(root / "infos.pkl", "wb") as f:
        pickle.dump(dict(infos=infos, metadata=dict(version="v1.0-mini")), f)
    return root / "infos.pkl"


def assert_same_metas(a, b):
    """two img_metas dicts {t: meta} hold the same keys and values"""
    assert sorted(a) == sorted(b)
    for t in a:
        assert sorted(a[t]) == sorted(b[t]), (sorted(a[t]), sorted(b[t]))
        for k in a[t]:
            _same(a[t][k], b[t][k], f"img_metas[{t}][{k!r}]")


def _same(x, y, what):
    if isinstance(x, dict):
        assert sorted(x) == sorted(y), what
        for k in x:
            _same(x[k], y[k], f"{what}[{k!r}]")
    elif isinstance(x, (list, tuple)) and not all(np.isscalar(v) for v in x):
        assert len(x) == len(y), what
        for i, (u, v) in enumerate(zip(x, y)):
            _same(u, v, f"{what}[{i}]")
    elif isinstance(x, (np.ndarray, list, tuple)) or hasattr(x, "numpy"):
        np.testing.assert_array_equal(np.asarray(x), np.asarray(y), err_msg=what)
    else:
        assert x == y, what
