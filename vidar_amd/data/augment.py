"""Host-side image augmentation of the training pipeline (config :308-311), for `ViDARSequenceDataset(augment=)`.

  CropResizeFlipImage   projects/mmdet3d_plugin/datasets/pipelines/augmentation.py:10-203 -- one crop / resize /
                        flip drawn per SAMPLE and replayed on every frame of its queue through `aug_param`
                        (nuscenes_vidar_dataset_template.py:116-124); rescales cam2img and rebuilds lidar2img; the
                        detector flips the FPN features back when the flip bit is set (detectors/vidar.py:123-126).
                        Pinned against the reference class (tests/golden/make_augment_golden.py).
  PhotoMetricDistortion pipelines/transform_3d.py:99-190 -- brightness / contrast / saturation / hue / channel swap
                        with the reference's draw order.  The BGR<->HSV conversion is mmcv's (cv2, float32: H in
                        degrees, S in [0,1], V = max channel) [3P, restated: cv2 is not installed here] -> UNPINNED.
Both work on a record dict(img [cams,3,H,W] float tensor BEFORE normalisation, img_metas) -- i.e. they are meant to
run between `load_images(..., normalise=False)` and the normalisation; `make_train_augment` wires that order."""
from __future__ import annotations

import copy
import random

import numpy as np
import torch

IDA_AUG_CONF = {"reisze": [720, 765, 810, 855, 900, 945, 990, 1035, 1080], "crop": (0, 0, 1600, 900),
                "H": 900, "W": 1600, "rand_flip": True}                           # config :41-47 (sic: "reisze")


class CropResizeFlipImage:
    def __init__(self, data_aug_conf=None, training=True):
        self.conf = dict(data_aug_conf or IDA_AUG_CONF)
        self.training = training

    def sample(self, aug_param):
        """(resize, resize_dims, crop, flip): replayed from `aug_param` when the queue already drew it (:179-203)"""
        if "CropResizeFlipImage_param" in aug_param:
            return aug_param["CropResizeFlipImage_param"]
        crop = self.conf["crop"]
        resized_h = random.choice(self.conf["reisze"])
        if not self.training:
            assert len(self.conf["reisze"]) == 1
        resized_w = resized_h / (crop[3] - crop[1]) * (crop[2] - crop[0])
        resize = resized_h / (crop[3] - crop[1])
        flip = bool(self.training and self.conf["rand_flip"] and np.random.choice([0, 1]))
        aug_param["CropResizeFlipImage_param"] = (resize, (int(resized_w), int(resized_h)), crop, flip)
        return aug_param["CropResizeFlipImage_param"]

    def draw(self, meta, aug_param, n_imgs=None):
        """the device path's half of `__call__`: same draws (`sample`), same cam2img / lidar2img update, no pixels.
        -> (resize, resize_dims, crop, flip)"""
        resize, resize_dims, crop, flip = self.sample(aug_param)
        ida = np.eye(3)
        ida[:2, :2] *= resize
        ida[:2, 2] = -np.array(crop[:2]) * resize
        for i in range(len(meta["cam2img"]) if n_imgs is None else n_imgs):
            meta["cam2img"][i][:3, :3] = np.matmul(ida, meta["cam2img"][i][:3, :3])
        meta["lidar2img"] = [np.matmul(meta["cam2img"][i], meta["lidar2cam"][i]) for i in range(len(meta["lidar2cam"]))]
        return resize, resize_dims, crop, flip

    @staticmethod
    def apply(imgs, param):
        """the pixel half of `__call__` for drawn parameters: list of HxWx3 arrays -> list of float32 arrays"""
        from PIL import Image
        _, resize_dims, crop, flip = param
        out = []
        for img in imgs:
            im = Image.fromarray(np.uint8(img)).crop(crop).resize(resize_dims)
            if flip:
                im = im.transpose(method=Image.FLIP_LEFT_RIGHT)
            out.append(np.array(im).astype(np.float32))
        return out

    def __call__(self, imgs, meta, aug_param):
        """imgs: list of HxWx3 float arrays (BGR, 0..255); meta: needs cam2img + lidar2cam.  -> new list;
        meta['cam2img'] / ['lidar2img'] updated in place (:88-89, :137-138)."""
        from PIL import Image
        resize, resize_dims, crop, flip = self.sample(aug_param)
        out = []
        ida = np.eye(3)
        ida[:2, :2] *= resize
        ida[:2, 2] = -np.array(crop[:2]) * resize
        for i, img in enumerate(imgs):
            im = Image.fromarray(np.uint8(img)).crop(crop).resize(resize_dims)
            if flip:
                im = im.transpose(method=Image.FLIP_LEFT_RIGHT)
            out.append(np.array(im).astype(np.float32))
            meta["cam2img"][i][:3, :3] = np.matmul(ida, meta["cam2img"][i][:3, :3])
        meta["lidar2img"] = [np.matmul(meta["cam2img"][i], meta["lidar2cam"][i]) for i in range(len(meta["lidar2cam"]))]
        return out


def bgr2hsv(img):
    """[3P] cv2.COLOR_BGR2HSV on float32: V = max, S = (V - min) / V (0 where V == 0), H in degrees [0, 360)"""
    b, g, r = img[..., 0], img[..., 1], img[..., 2]
    v = img.max(-1)
    d = v - img.min(-1)
    s = np.where(v > 0, d / np.where(v > 0, v, 1), 0)
    dd = np.where(d > 0, d, 1)
    h = np.where(v == r, (g - b) / dd, np.where(v == g, 2 + (b - r) / dd, 4 + (r - g) / dd)) * 60
    h = np.where(d > 0, h, 0)
    h = np.where(h < 0, h + 360, h)
    return np.stack([h, s, v], -1).astype(np.float32)


def hsv2bgr(img):
    """[3P] cv2.COLOR_HSV2BGR on float32"""
    h, s, v = img[..., 0] / 60.0, img[..., 1], img[..., 2]
    i = np.floor(h).astype(np.int32) % 6
    f = h - np.floor(h)
    p, q, t = v * (1 - s), v * (1 - s * f), v * (1 - s * (1 - f))
    r = np.choose(i, [v, q, p, p, t, v])
    g = np.choose(i, [t, v, v, q, p, p])
    b = np.choose(i, [p, p, t, v, v, q])
    return np.stack([b, g, r], -1).astype(np.float32)


class PhotoMetricDistortionMultiViewImage:
    def __init__(self, brightness_delta=32, contrast_range=(0.5, 1.5), saturation_range=(0.5, 1.5), hue_delta=18):
        self.brightness_delta = brightness_delta
        self.contrast_lower, self.contrast_upper = contrast_range
        self.saturation_lower, self.saturation_upper = saturation_range
        self.hue_delta = hue_delta

    @staticmethod
    def _coin_uniform(lo, hi):
        """the reference's draw pattern: a fair coin first, the magnitude only when the coin says yes"""
        return np.random.uniform(lo, hi) if np.random.randint(2) else None

    def _distort(self, img):
        img = np.array(img, dtype=np.float32)
        shift = self._coin_uniform(-self.brightness_delta, self.brightness_delta)
        if shift is not None:
            img += shift
        contrast_first = np.random.randint(2) == 1               # "mode": contrast before or after the HSV stage
        gain = self._coin_uniform(self.contrast_lower, self.contrast_upper) if contrast_first else None
        if gain is not None:
            img *= gain
        hsv = bgr2hsv(img)
        sat = self._coin_uniform(self.saturation_lower, self.saturation_upper)
        if sat is not None:
            hsv[..., 1] *= sat
        turn = self._coin_uniform(-self.hue_delta, self.hue_delta)
        if turn is not None:
            hue = hsv[..., 0] + turn
            hue[hue > 360] -= 360
            hue[hue < 0] += 360
            hsv[..., 0] = hue
        img = hsv2bgr(hsv)
        gain = None if contrast_first else self._coin_uniform(self.contrast_lower, self.contrast_upper)
        if gain is not None:
            img *= gain
        if np.random.randint(2):
            img = img[..., np.random.permutation(3)]
        return img

    # ---- the device path: draw without touching pixels, apply later (vidar_amd/data/device_prep.py) ----
    # one image's parameters as the float32 row the kernels read (include/vidar_hip.h): shift, gain before the HSV stage,
    # saturation, hue turn, gain after it, flags, the channel permutation, 3 reserved
    SHIFT, GAIN_FIRST, SAT, TURN, GAIN_LAST = 1, 2, 4, 8, 16

    def draw_one(self):
        """consumes numpy's global generator exactly like `_distort` -> float32 [12]"""
        row = np.zeros(12, np.float32)
        row[6:9] = (0, 1, 2)
        flags = 0
        shift = self._coin_uniform(-self.brightness_delta, self.brightness_delta)
        if shift is not None:
            row[0] = shift; flags |= self.SHIFT
        contrast_first = np.random.randint(2) == 1
        gain = self._coin_uniform(self.contrast_lower, self.contrast_upper) if contrast_first else None
        if gain is not None:
            row[1] = gain; flags |= self.GAIN_FIRST
        sat = self._coin_uniform(self.saturation_lower, self.saturation_upper)
        if sat is not None:
            row[2] = sat; flags |= self.SAT
        turn = self._coin_uniform(-self.hue_delta, self.hue_delta)
        if turn is not None:
            row[3] = turn; flags |= self.TURN
        gain = None if contrast_first else self._coin_uniform(self.contrast_lower, self.contrast_upper)
        if gain is not None:
            row[4] = gain; flags |= self.GAIN_LAST
        if np.random.randint(2):
            row[6:9] = np.random.permutation(3)
        row[5] = flags
        return row

    def draw(self, n_imgs):
        """-> float32 [n_imgs, 12], every image its own draws, in order (what `__call__` does to the generator)"""
        return np.stack([self.draw_one() for _ in range(n_imgs)])

    @classmethod
    def apply_one(cls, img, row):
        """`_distort` with drawn parameters: the same numpy operations in the same order (float32 scalars: the value
        numpy's float32 arithmetic rounds a Python float to)"""
        img = np.array(img, dtype=np.float32)
        flags = int(row[5])
        f32 = lambda k: np.float32(row[k])
        if flags & cls.SHIFT:
            img += f32(0)
        if flags & cls.GAIN_FIRST:
            img *= f32(1)
        hsv = bgr2hsv(img)
        if flags & cls.SAT:
            hsv[..., 1] *= f32(2)
        if flags & cls.TURN:
            hue = hsv[..., 0] + f32(3)
            hue[hue > 360] -= 360
            hue[hue < 0] += 360
            hsv[..., 0] = hue
        img = hsv2bgr(hsv)
        if flags & cls.GAIN_LAST:
            img *= f32(4)
        perm = [int(k) for k in row[6:9]]
        if perm != [0, 1, 2]:
            img = img[..., perm]
        return img

    @classmethod
    def apply(cls, imgs, rows):
        return [cls.apply_one(img, row) for img, row in zip(imgs, rows)]

    def __call__(self, imgs):
        """every image of the rig draws its own distortion, in order (numpy's global generator, like the reference's
        `from numpy import random`)"""
        return [self._distort(img) for img in imgs]
