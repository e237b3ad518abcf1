"""GPU: the image pipeline's kernels (csrc/img_prep.hip) through the C ABI against numpy / PIL / reader.normalise_pad, and
`device_images` samples + `finish_batch` against the host path end to end."""
import ctypes
import random
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).parent))
import img_prep_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu
BAD_ARG = -22


def _lib():
    from vidar_amd._lib import lib
    return lib()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    from vidar_amd._lib import ptr
    return ptr(t)


def _table(n_in, n_out):
    from vidar_amd.data.device_prep import resample_table
    bounds, kk = resample_table(n_in, n_out)
    return _dev(np.concatenate([bounds.ravel(), kk.ravel()])), kk.shape[1]


def _f3(v):
    return (ctypes.c_float * 3)(*v)


@pytest.fixture(scope="module")
def photo_reference():
    """numpy's `_distort` on the adversarial image for the whole parameter grid, computed once"""
    img, rows = C.adversarial_image(), C.photo_grid()
    want = np.stack([C.replay_distort(img.astype(np.float32), r) for r in rows])
    return img, rows, want


def test_photometric_kernel_is_numpy_bit_for_bit(photo_reference):
    img, rows, want = photo_reference
    n = len(rows)
    src, par = _dev(np.stack([img] * n)), _dev(rows)
    u8 = torch.full((n, 32, 32, 3), 7, dtype=torch.uint8, device="cuda")
    f32 = torch.full((n, 32, 32, 3), float("nan"), device="cuda")
    assert _lib().vidar_img_photometric_u8(_p(src), _p(par), _p(u8), n, 32, 32, None) == 0
    assert _lib().vidar_img_photometric_f32(_p(src), _p(par), _p(f32), n, 32, 32, None) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(f32.cpu().numpy().view(np.uint32), want.view(np.uint32))
    np.testing.assert_array_equal(u8.cpu().numpy(), C.host_cast_u8(want))          # int(x) & 255, not np.uint8
    assert ((want < 0) | (want >= 256)).mean() > 0.01


def test_photometric_kernel_tail_and_unaligned_images():
    """5 x 7 = 35 pixels per image: no multiple of 4, every second image starts off a dword boundary"""
    from vidar_amd.data.augment import PhotoMetricDistortionMultiViewImage as P
    rows = C.photo_grid()[[5, 77, 143]]
    imgs = np.random.default_rng(1).integers(0, 256, (3, 5, 7, 3), dtype=np.uint8)
    want = np.stack(P.apply(list(imgs.astype(np.float32)), rows))
    guard = torch.full((3 * 35 * 3 + 16,), 9, dtype=torch.uint8, device="cuda")
    assert _lib().vidar_img_photometric_u8(_p(_dev(imgs)), _p(_dev(rows)), _p(guard), 3, 5, 7, None) == 0
    torch.cuda.synchronize()
    got = guard.cpu().numpy()
    np.testing.assert_array_equal(got[:315].reshape(3, 5, 7, 3), C.host_cast_u8(want))
    assert (got[315:] == 9).all()


def _resample_cases():
    out = []
    for h, w in [(9, 16), (37, 53), (45, 80)]:
        full = (0, 0, w, h)
        dn, up = (max(int(h * 0.8), 2), max(int(w * 0.8), 2)), (int(h * 1.2) + 1, int(w * 1.2) + 1)
        out += [((h, w), full, dn, False), ((h, w), full, dn, True), ((h, w), full, up, False), ((h, w), full, up, True),
                ((h, w), full, (dn[0], w), False),              # horizontal pass skipped
                ((h, w), full, (h, up[1]), True),               # vertical pass skipped
                ((h, w), full, (h, w), True),                   # flip only
                ((h, w), (3, 2, w - 2, h - 1), dn, True), ((h, w), (3, 2, w - 2, h - 1), up, False),
                ((h, w), (1, 3, w - 4, h - 2), None, False)]                    # a bare crop: size unchanged
    return out


@pytest.mark.parametrize("hw,box,out_hw,flip", _resample_cases())
def test_resample_kernel_matches_pil(hw, box, out_hw, flip):
    from PIL import Image
    from vidar_amd.data.device_prep import bicubic_ksize
    H, W = hw
    x0, y0, x1, y1 = box
    cw, ch = x1 - x0, y1 - y0
    oh, ow = (ch, cw) if out_hw is None else out_hw
    n = 2
    imgs = np.random.default_rng(H * W + oh).integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    imgs[0, H // 3: H // 2] = 255; imgs[0, :, W // 2: W // 2 + 2] = 0            # edges that overshoot: the clip matters
    want = []
    for a in imgs:
        im = Image.fromarray(a).crop(box).resize((ow, oh))
        want.append(np.array(im.transpose(method=Image.FLIP_LEFT_RIGHT) if flip else im))
    need_x = ow != cw or flip
    need_y = oh != ch or not need_x
    tx, kx = _table(cw, ow) if need_x else (None, 0)
    ty, ky = _table(ch, oh) if need_y else (None, 0)
    if need_x and ow < cw:
        assert kx >= 7
    if need_x and ow > cw:
        assert kx == 5 == bicubic_ksize(cw, ow)
    L = _lib()
    nbytes = L.vidar_img_resample_workspace_bytes(n, ch, ow)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.full((n * oh * ow * 3 + 16,), 9, dtype=torch.uint8, device="cuda")
    rc = L.vidar_img_resample_u8(_p(_dev(imgs)), _p(dst), n, H, W, x0, y0, cw, ch, ow, oh, _p(tx), kx, _p(ty), ky, int(flip),
                                 _p(ws), nbytes, None)
    torch.cuda.synchronize()
    assert rc == 0
    got = dst.cpu().numpy()
    np.testing.assert_array_equal(got[:-16].reshape(n, oh, ow, 3), np.stack(want))
    assert (got[-16:] == 9).all()


@pytest.mark.parametrize("hw", [(37, 53), (45, 80), (32, 64)])
@pytest.mark.parametrize("to_rgb", [False, True])
def test_normalise_pad_kernel_is_bit_equal(hw, to_rgb):
    from vidar_amd.data.reader import normalise_pad
    H, W = hw
    mean, std = ([123.675, 116.28, 103.53], [58.395, 57.12, 57.375]) if to_rgb else (C.CAFFE_MEAN, [1.0, 2.5, 0.75])
    imgs = np.random.default_rng(H).integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    want, shape = normalise_pad(list(imgs.astype(np.float32)), mean, std, to_rgb, 32)
    Hp, Wp = shape[:2]
    assert hw == (32, 64) or (Hp > H and Wp > W)                                 # padding on both axes
    dst = torch.full((3, 3, Hp, Wp), float("nan"), device="cuda")
    rc = _lib().vidar_img_normalise_f32(_p(_dev(imgs)), None, _p(dst), 3, H, W, H, W, Hp, Wp, _f3(mean), _f3(std), int(to_rgb),
                                        None)
    torch.cuda.synchronize()
    assert rc == 0
    np.testing.assert_array_equal(dst.cpu().numpy().view(np.uint32), want.numpy().view(np.uint32))


@pytest.mark.parametrize("hw", C.SCALED_CASES)
def test_scaled_normalise_kernel_against_normalise_pad(hw):
    """OpenScene's 2/3 bilinear resize of the normalised values.  Bound: four times the host build's own distance to
    torch on these shapes (img_prep_cases.SCALED_HOST_DIFF, measured in tests/test_img_prep_cpu.py)"""
    from vidar_amd.data.reader import normalise_pad
    H, W = hw
    a = C.scaled_case(H, W)
    oh, ow = int(H * (2 / 3)), int(W * (2 / 3))
    want, shape = normalise_pad([a.astype(np.float32)], C.CAFFE_MEAN, C.UNIT_STD, False, 32, scale=2 / 3)
    Hp, Wp = shape[:2]
    dst = torch.full((1, 3, Hp, Wp), float("nan"), device="cuda")
    rc = _lib().vidar_img_normalise_f32(_p(_dev(a[None])), None, _p(dst), 1, H, W, oh, ow, Hp, Wp, _f3(C.CAFFE_MEAN),
                                        _f3(C.UNIT_STD), 0, None)
    torch.cuda.synchronize()
    assert rc == 0
    got = dst.cpu().numpy()
    d = float(np.abs(got - want.numpy()).max())
    print(f"scaled {H}x{W}: max |kernel - normalise_pad| = {d:.9g} (bound {4 * C.SCALED_HOST_DIFF:.9g})")
    assert d <= 4 * C.SCALED_HOST_DIFF
    assert (got[:, :, oh:] == 0).all() and (got[:, :, :, ow:] == 0).all()


def _read(ann, device_images, seed, **kw):
    from vidar_amd.data.reader import ViDARSequenceDataset
    ds = ViDARSequenceDataset(ann, queue_length=1, future_length=1, device_images=device_images, **kw)
    random.seed(seed); np.random.seed(seed)
    return ds[1]


def test_end_to_end_device_images_equal_the_host_path(tmp_path):
    """T = 2, 3 cameras, 45 x 80, pixels in [80, 130] (every draw stays inside [0, 256)), one smaller and one larger
    `reisze` height: same seed, `img` bit-equal, metas equal"""
    from vidar_amd.data.device_prep import DeviceImagePrep
    from vidar_amd.data.loader import collate, finish_batch
    from vidar_amd.data.reader import TrainAugment
    ann = C.mini_dataset(tmp_path)
    conf = {"reisze": [36, 54], "crop": (0, 0, 80, 45), "H": 45, "W": 80, "rand_flip": True}
    prep = DeviceImagePrep()
    seen, seed_of = set(), {}
    for seed in range(6):
        host = _read(ann, False, seed, augment=TrainAugment(conf))
        dev = _read(ann, True, seed, augment=TrainAugment(conf))
        batch = finish_batch(collate([dev]), torch.device("cuda"), prep)
        assert "img_raw" not in batch and batch["img"].is_cuda
        np.testing.assert_array_equal(batch["img"][0].cpu().numpy().view(np.uint32), host["img"].numpy().view(np.uint32))
        C.assert_same_metas(host["img_metas"], batch["img_metas"][0])
        p = dev["img_plan"]
        seen.add((p["resize_dims"], p["flip"]))
        seed_of[p["resize_dims"]] = seed
    assert len({s[0] for s in seen}) == 2 and len({s[1] for s in seen}) == 2      # both sizes, flipped and not
    # two samples of different resized sizes in one batch are padded to the larger, like collate does on the host
    pair = []
    for device_images in (False, True):
        a, b = (_read(ann, device_images, s, augment=TrainAugment(conf)) for s in sorted(seed_of.values()))
        pair.append(collate([a, b]))
    got = finish_batch(pair[1], torch.device("cuda"), prep)["img"]
    assert torch.equal(got.cpu(), pair[0]["img"])


def test_end_to_end_test_and_openscene_pipelines(tmp_path):
    from vidar_amd.data.loader import collate, finish_batch
    from vidar_amd.data.reader import TrainAugment
    ann = C.mini_dataset(tmp_path)
    host, dev = (_read(ann, d, 0, test_mode=True) for d in (False, True))
    got = finish_batch(collate([dev]), torch.device("cuda"))["img"][0].cpu()
    assert torch.equal(got, host["img"])
    # OpenScene train: photometric in fp32 (no uint8 cast), normalise, 2/3 bilinear.  The pixels stay in (0, 256), so the
    # scaled path's bound (values below 256 in magnitude, the same four taps) applies unchanged.
    kw = dict(augment=TrainAugment(photometric=True, crop_resize_flip=False), img_scale=2 / 3)
    host, dev = (_read(ann, d, 3, **kw) for d in (False, True))
    got = finish_batch(collate([dev]), torch.device("cuda"))["img"][0].cpu()
    assert got.shape == host["img"].shape
    d = float((got - host["img"]).abs().max())
    print(f"OpenScene train: max |device - host| = {d:.9g}")
    assert d <= 4 * C.SCALED_HOST_DIFF
    C.assert_same_metas(host["img_metas"], dev["img_metas"])


def test_bad_arguments_launch_nothing():
    L = _lib()
    H, W, n = 9, 16, 1
    src = _dev(np.zeros((n, H, W, 3), np.uint8))
    dst = torch.full((4096,), 9, dtype=torch.uint8, device="cuda")
    fdst = torch.full((3 * 32 * 32,), 5.0, device="cuda")
    ws = torch.empty(4096, dtype=torch.uint8, device="cuda")
    tx, kx = _table(16, 12)
    ty, ky = _table(9, 7)

    def resample(x0=0, y0=0, cw=16, ch=9, ow=12, oh=7, tx_=tx, kx_=kx, ty_=ty, ky_=ky, n_=n, wsn=4096):
        return L.vidar_img_resample_u8(_p(src), _p(dst), n_, H, W, x0, y0, cw, ch, ow, oh, _p(tx_), kx_, _p(ty_), ky_, 0, _p(ws),
                                       wsn, None)
    assert resample(x0=1) == BAD_ARG and resample(y0=1) == BAD_ARG and resample(x0=-1, cw=16) == BAD_ARG   # box leaves the image
    assert resample(cw=0) == BAD_ARG and resample(oh=0) == BAD_ARG and resample(n_=0) == BAD_ARG            # zero sizes
    assert resample(kx_=kx + 2) == BAD_ARG and resample(ky_=5) == BAD_ARG                                  # table / ksize mismatch
    assert resample(tx_=None, kx_=0) == BAD_ARG                                                             # skipped pass, in != out
    assert resample(wsn=16) == BAD_ARG
    par = _dev(C.photo_grid()[:1])
    assert L.vidar_img_photometric_u8(_p(src), _p(par), _p(dst), n, 0, W, None) == BAD_ARG
    assert L.vidar_img_photometric_u8(_p(src), None, _p(dst), n, H, W, None) == BAD_ARG
    m, s = _f3(C.CAFFE_MEAN), _f3(C.UNIT_STD)
    assert L.vidar_img_normalise_f32(_p(src), None, _p(fdst), n, H, W, H, W, 8, 32, m, s, 0, None) == BAD_ARG   # Hp < out_h
    assert L.vidar_img_normalise_f32(_p(src), None, _p(fdst), n, H, W, H, W, 32, 30, m, s, 0, None) == BAD_ARG  # Wp % 4
    assert L.vidar_img_normalise_f32(_p(src), None, _p(fdst), n, H, 0, H, W, 32, 32, m, s, 0, None) == BAD_ARG
    torch.cuda.synchronize()
    assert (dst == 9).all() and (fdst == 5.0).all()
    assert resample() == 0                                                                                  # and the good call works
    torch.cuda.synchronize()
    assert not (dst[:n * 7 * 12 * 3] == 9).all()
