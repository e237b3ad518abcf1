"""Device-side image pipeline: raw uint8 HWC BGR frames -> the fp32 [n, 3, Hp, Wp] network input (csrc/img_prep.hip).

The dataloader workers only decode and DRAW (augment.py `draw`), the arithmetic of the released pipelines runs on the GPU
with the host path's bits:
  nuScenes train   photometric (fp32) -> uint8 cast -> crop -> PIL bicubic resize -> flip -> normalise -> pad
  nuScenes test    normalise -> pad
  OpenScene        [photometric ->] normalise -> bilinear resize by img_scale -> pad
A `plan` (dict, built by the reader per sample) holds what was drawn:
  photo        float32 [n, 12] per-image photometric rows (PhotoMetricDistortionMultiViewImage.draw) or None
  resize_dims  (w, h) of CropResizeFlipImage or None        crop  (x0, y0, x1, y1)        flip  bool
  img_scale    None or the OpenScene factor
The float -> uint8 rule between the photometric stage and PIL is: truncate toward zero to int32, keep the low 8 bits.

`resample_table` restates PIL's 8-bit coefficient computation (src/libImaging/Resample.c: precompute_coeffs +
normalize_coeffs_8bpc, bicubic a = -0.5) in float64 on the host; tests/test_img_prep_cpu.py pins it against PIL."""
from __future__ import annotations

import ctypes
import math
import warnings
from functools import lru_cache

import numpy as np
import torch

PRECISION_BITS = 22
PHOTO_FLOATS = 12


def _bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def bicubic_ksize(n_in, n_out):
    return 2 * int(math.ceil(2.0 * max(n_in / n_out, 1.0))) + 1


@lru_cache(maxsize=64)
def resample_table(n_in: int, n_out: int):
    """-> (bounds int32 [n_out, 2] = (first source index, tap count), coefficients int32 [n_out, ksize]) of one axis"""
    scale = filterscale = n_in / n_out
    if filterscale < 1.0:
        filterscale = 1.0
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((n_out, 2), np.int32)
    kk = np.zeros((n_out, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), n_in) - xmin
        w = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            kk[xx, x] = int(v * (1 << PRECISION_BITS) - 0.5) if v < 0 else int(v * (1 << PRECISION_BITS) + 0.5)
        bounds[xx] = (xmin, n)
    bounds.setflags(write=False); kk.setflags(write=False)
    return bounds, kk


def resample_axis_numpy(a, axis, n_out):
    """one pass of PIL's resampler on a uint8 array, in numpy integers (the definition the kernel follows)"""
    a = np.moveaxis(np.asarray(a, np.uint8), axis, 0)
    bounds, kk = resample_table(a.shape[0], n_out)
    out = np.empty((n_out,) + a.shape[1:], np.uint8)
    for xx in range(n_out):
        x0, n = bounds[xx]
        acc = np.tensordot(kk[xx, :n].astype(np.int64), a[x0:x0 + n].astype(np.int64), 1) + (1 << (PRECISION_BITS - 1))
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize_numpy(a, out_w, out_h):
    """PIL `Image.resize((out_w, out_h))` (bicubic) of a uint8 [H, W, C] array: horizontal pass, then vertical; a pass
    whose size does not change is skipped"""
    if a.shape[1] != out_w:
        a = resample_axis_numpy(a, 1, out_w)
    if a.shape[0] != out_h:
        a = resample_axis_numpy(a, 0, out_h)
    return a


def cast_u8(x):
    """the pipeline's float -> uint8 rule: truncate toward zero to int32, keep the low 8 bits"""
    return (np.trunc(np.asarray(x, np.float32)).astype(np.int32) & 255).astype(np.uint8)


def out_shape(plan, H, W):
    """(h, w) of the image content after the pipeline, before padding"""
    if plan.get("resize_dims") is not None:
        H, W = int(plan["resize_dims"][1]), int(plan["resize_dims"][0])
    if plan.get("img_scale") is not None:
        H, W = int(H * plan["img_scale"]), int(W * plan["img_scale"])
    return H, W


def crop_inside(crop, H, W):
    x0, y0, x1, y1 = (int(v) for v in crop)
    return 0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H


def host_prep(raw_u8, plan, mean, std, to_rgb, size_divisor):
    """the host pipeline on drawn parameters (numpy / PIL): what the default path computes, and the fallback of
    `DeviceImagePrep` for geometry the kernels do not take (a crop box that leaves the image: PIL pads it with zeros)"""
    from .augment import CropResizeFlipImage, PhotoMetricDistortionMultiViewImage
    from .reader import normalise_pad
    imgs = [a.astype(np.float32) for a in np.asarray(raw_u8)]
    if plan.get("photo") is not None:
        imgs = PhotoMetricDistortionMultiViewImage.apply(imgs, plan["photo"])
    if plan.get("resize_dims") is not None:
        imgs = CropResizeFlipImage.apply(imgs, (None, plan["resize_dims"], plan["crop"], plan["flip"]))
    return normalise_pad(imgs, mean, std, to_rgb, size_divisor, scale=plan.get("img_scale"))[0]


class DeviceImagePrep:
    """`prep(raw_u8 [n, H, W, 3] uint8 on the GPU, plan)` -> float32 [n, 3, Hp, Wp]; at most four kernel launches"""

    def __init__(self, mean=None, std=None, to_rgb=None, size_divisor=32):
        from .reader import IMG_NORM
        self.mean = [float(v) for v in (IMG_NORM["mean"] if mean is None else mean)]
        self.std = [float(v) for v in (IMG_NORM["std"] if std is None else std)]
        self.to_rgb = bool(IMG_NORM["to_rgb"] if to_rgb is None else to_rgb)
        self.size_divisor = int(size_divisor)
        if self.size_divisor % 4:
            raise ValueError("DeviceImagePrep: size_divisor must be a multiple of 4 (16-byte stores of the padded rows)")
        self._mean = (ctypes.c_float * 3)(*self.mean)
        self._std = (ctypes.c_float * 3)(*self.std)
        self._tables = {}

    def _table(self, n_in, n_out, device):
        """device copy of an axis' table ([out, 2] bounds then [out, ksize] coefficients), cached per (in, out)"""
        key = (n_in, n_out, str(device))
        if key not in self._tables:
            bounds, kk = resample_table(n_in, n_out)
            flat = np.concatenate([bounds.ravel(), kk.ravel()])
            self._tables[key] = (torch.from_numpy(flat).to(device), kk.shape[1])
        return self._tables[key]

    def padded(self, h, w):
        d = self.size_divisor
        return (h + d - 1) // d * d, (w + d - 1) // d * d

    def __call__(self, raw_u8, plan):
        from .._lib import check, lib, ptr, stream_of, workspace
        if not (raw_u8.is_cuda and raw_u8.dtype == torch.uint8 and raw_u8.dim() == 4 and raw_u8.shape[-1] == 3):
            raise ValueError("DeviceImagePrep: expected a uint8 [n, H, W, 3] tensor on the GPU")
        raw_u8 = raw_u8.contiguous()
        n, H, W, _ = raw_u8.shape
        L, dev, st = lib(), raw_u8.device, stream_of(raw_u8)
        photo = plan.get("photo")
        resize_dims = plan.get("resize_dims")
        if resize_dims is not None and not crop_inside(plan["crop"], H, W):
            warnings.warn("DeviceImagePrep: crop box outside the image, this sample takes the host path")
            return host_prep(raw_u8.cpu().numpy(), plan, self.mean, self.std, self.to_rgb, self.size_divisor).to(dev)
        photo_dev = None
        if photo is not None:
            photo = np.ascontiguousarray(photo, np.float32)
            assert photo.shape == (n, PHOTO_FLOATS), photo.shape
            photo_dev = torch.from_numpy(photo).to(dev, non_blocking=True)
        src, h, w = raw_u8, H, W
        if resize_dims is not None:                                  # nuScenes train: uint8 all the way to the normalise
            if photo_dev is not None:
                dist = torch.empty_like(raw_u8)
                check(L.vidar_img_photometric_u8(ptr(raw_u8), ptr(photo_dev), ptr(dist), n, H, W, st), "img_photometric")
                src, photo_dev = dist, None
            x0, y0, x1, y1 = (int(v) for v in plan["crop"])
            cw, ch, ow, oh = x1 - x0, y1 - y0, int(resize_dims[0]), int(resize_dims[1])
            flip = bool(plan.get("flip"))
            if not ((x0, y0, cw, ch) == (0, 0, W, H) and (ow, oh) == (cw, ch) and not flip):
                need_x = ow != cw or flip
                need_y = oh != ch or not need_x                      # a bare crop is the identity table on the rows
                tx, kx = self._table(cw, ow, dev) if need_x else (None, 0)
                ty, ky = self._table(ch, oh, dev) if need_y else (None, 0)
                out = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device=dev)
                ws, ws_ptr, ws_n = workspace(L.vidar_img_resample_workspace_bytes, n, ch, ow, like=raw_u8) \
                    if need_x and need_y else (None, None, 0)
                check(L.vidar_img_resample_u8(ptr(src), ptr(out), n, H, W, x0, y0, cw, ch, ow, oh, ptr(tx), kx, ptr(ty), ky,
                                              int(flip), ws_ptr, ws_n, st), "img_resample")
                src, h, w = out, oh, ow
        oh, ow = out_shape(plan, H, W)
        Hp, Wp = self.padded(oh, ow)
        img = torch.empty((n, 3, Hp, Wp), dtype=torch.float32, device=dev)
        check(L.vidar_img_normalise_f32(ptr(src), ptr(photo_dev), ptr(img), n, h, w, oh, ow, Hp, Wp, self._mean, self._std,
                                        int(self.to_rgb), st), "img_normalise")
        return img
