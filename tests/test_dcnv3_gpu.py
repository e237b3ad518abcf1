"""GPU: the DCNv3 HIP kernels (csrc/dcnv3.hip) against the reference's own kernels compiled for the host in fp64
(oracle/_ref/ref_dcnv3.so: `dcnv3_im2col_gpu_kernel`, `dcnv3_col2im_gpu_kernel_gm`) evaluated on the fp32-rounded
operands, against the reference goldens, and up through the `DCNv3` module, the InternImage backbone and one whole
training step.  Reads oracle/_ref and tests/golden only.

Bounds (those of tests/test_dcn_gpu.py for the same kind of sum): output rtol 1e-4 / atol 1e-4, gradients
rtol 2e-4 / atol 2e-4 * max(1, |ref|_max).  grad_offset is discontinuous where a location crosses an integer: its
elements whose fp64 location lies within 1e-4 px of an integer in either coordinate are left out, at most 0.5 % per case
(asserted; expected ~4e-4 for continuous random offsets).  Nothing is left out of output, grad_input, grad_mask."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from test_dcnv3_cpu import GOLD, INTERNIMAGE_CASES, away_from_minus_one, kernel_locations

pytestmark = pytest.mark.gpu
sys.path.insert(0, str(GOLD))


def out_size(n, k, s, p, d):
    return (n + 2 * p - (d * (k - 1) + 1)) // s + 1


def operands(seed, N, H, W, G, gc, kh, kw, sh, sw, ph, pw, dh, dw, sigma, integer=False):
    g = torch.Generator().manual_seed(seed)
    Ho, Wo, P = out_size(H, kh, sh, ph, dh), out_size(W, kw, sw, pw, dw), kh * kw
    x = torch.randn(N, H, W, G * gc, generator=g)
    if integer:
        off = torch.randint(-3, 4, (N, Ho, Wo, G * P * 2), generator=g).float()
    else:
        off = torch.randn(N, Ho, Wo, G * P * 2, generator=g) * sigma
    mask = torch.softmax(torch.randn(N, Ho, Wo, G, P, generator=g), -1).reshape(N, Ho, Wo, G * P)
    gout = torch.randn(N, Ho, Wo, G * gc, generator=g)
    return x, off, mask, gout


def hip(x, off, mask, gout, geo):
    from vidar_amd.third_lib import dcnv3
    d = [t.cuda() for t in (x, off, mask, gout)]
    out = dcnv3.dcnv3_forward(d[0], d[1], d[2], *geo, 256)
    grads = dcnv3.dcnv3_backward(d[0], d[1], d[2], *geo, d[3], 256)
    torch.cuda.synchronize()
    return out.cpu(), [g.cpu() for g in grads]


def compare(what, got_out, got_grads, ref_out, ref_grads, off, geo14):
    """geo14 = (H, W, kh, kw, sh, sw, ph, pw, dh, dw, G, offset_scale)"""
    err = float((got_out.double() - ref_out).abs().max())
    print(f"{what}: out max |diff| {err:.3e}")
    torch.testing.assert_close(got_out.double(), ref_out, rtol=1e-4, atol=1e-4, msg=lambda m: f"{what} out: {m}")
    for nm, a, b in zip(("grad_input", "grad_offset", "grad_mask"), got_grads, ref_grads):
        a = a.double()
        atol = 2e-4 * max(1.0, float(b.abs().max()))
        if nm == "grad_offset":
            h, w = kernel_locations(off, *geo14)
            near = ((h - h.round()).abs() < 1e-4) | ((w - w.round()).abs() < 1e-4)          # [N,Ho,Wo,G,P]
            share = float(near.float().mean())
            print(f"{what}: grad_offset elements left out {share:.2e}")
            assert share <= 5e-3, f"{what}: {share:.3%} of grad_offset within 1e-4 px of an integer"
            keep = (~near).unsqueeze(-1).expand(*near.shape, 2).reshape(b.shape)
            a, b = a[keep], b[keep]
        print(f"{what}: {nm} max |diff| {float((a - b).abs().max()) if a.numel() else 0.0:.3e} (atol {atol:.1e})")
        torch.testing.assert_close(a, b, rtol=2e-4, atol=atol, msg=lambda m: f"{what} {nm}: {m}")


#        name                 N  H    W    G   gc  k  s  p  d  offset_scale sigma
SQUARE = [
    ("t_stage0_reduced",      2, 29,  50,  4,  16, 3, 1, 1, 1, 1.0, 1.5),
    ("t_stage1_reduced",      2, 15,  25,  8,  16, 3, 1, 1, 1, 1.0, 1.5),
    ("t_stage2_reduced",      2, 8,   13,  16, 16, 3, 1, 1, 1, 1.0, 1.5),
    ("t_stage3_reduced",      2, 4,   7,   32, 16, 3, 1, 1, 1, 1.0, 1.5),
    ("t_stage0_full",         1, 232, 400, 4,  16, 3, 1, 1, 1, 1.0, 1.5),
    ("gc32",                  2, 12,  14,  3,  32, 3, 1, 1, 1, 1.0, 1.5),
    ("gc3",                   2, 12,  14,  5,  3,  3, 1, 1, 1, 1.0, 1.5),
    ("gc7",                   2, 12,  14,  3,  7,  3, 1, 1, 1, 2.5, 1.5),
    ("gc12_idle_lane",        1, 10,  11,  2,  12, 3, 1, 1, 1, 1.0, 1.5),
    ("k5_pad2",               2, 14,  12,  2,  16, 5, 1, 2, 1, 1.0, 1.5),
    ("stride2_pad0",          2, 15,  17,  4,  16, 3, 2, 0, 1, 1.0, 1.5),
    ("stride2_pad2_dil2",     2, 15,  17,  2,  7,  3, 2, 2, 2, 2.5, 1.5),
    ("dil2_pad2",             1, 13,  16,  4,  16, 3, 1, 2, 2, 1.0, 1.5),
    ("scale2.5",              2, 12,  14,  4,  16, 3, 1, 1, 1, 2.5, 1.5),
    ("far_field",             2, 29,  50,  4,  16, 3, 1, 1, 1, 1.0, 12.0),
    ("far_field_gc3",         1, 20,  18,  2,  3,  3, 1, 0, 1, 1.0, 12.0),
]


@pytest.mark.parametrize("case", SQUARE, ids=[c[0] for c in SQUARE])
def test_kernels_match_the_reference_kernels_fp64(case, ref_modules):
    ref = ref_modules("ref_dcnv3")
    name, N, H, W, G, gc, k, s, p, d, os_, sigma = case
    x, off, mask, gout = operands(200 + [c[0] for c in SQUARE].index(name), N, H, W, G, gc, k, k, s, s, p, p, d, d, sigma)
    got_out, got_grads = hip(x, off, mask, gout, (k, k, s, s, p, p, d, d, G, gc, os_))
    xd, od, md, gd = (t.double() for t in (x, off, mask, gout))
    want = ref.im2col(xd, od, md, k, k, s, p, d, G, gc, os_)
    want_grads = ref.col2im(gd, xd, od, md, k, k, s, p, d, G, gc, os_)
    compare(name, got_out, got_grads, want, want_grads, off, (H, W, k, k, s, s, p, p, d, d, G, os_))


def test_integer_offsets_leave_nothing_out(ref_modules):
    """offset_scale = 1 and integer offsets: locations are exact in fp32, the in/out decision and the cell are the reference's"""
    ref = ref_modules("ref_dcnv3")
    N, H, W, G, gc, k = 2, 12, 14, 4, 16, 3
    x, off, mask, gout = operands(5, N, H, W, G, gc, k, k, 1, 1, 1, 1, 1, 1, 0.0, integer=True)
    got_out, got_grads = hip(x, off, mask, gout, (k, k, 1, 1, 1, 1, 1, 1, G, gc, 1.0))
    xd, od, md, gd = (t.double() for t in (x, off, mask, gout))
    want, want_grads = ref.im2col(xd, od, md, k, k, 1, 1, 1, G, gc, 1.0), ref.col2im(gd, xd, od, md, k, k, 1, 1, 1, G, gc, 1.0)
    torch.testing.assert_close(got_out.double(), want, rtol=1e-4, atol=1e-4)
    for a, b in zip(got_grads, want_grads):
        torch.testing.assert_close(a.double(), b, rtol=2e-4, atol=2e-4 * max(1.0, float(b.abs().max())))


@pytest.mark.parametrize("gc", [16, 3])
def test_all_outside_gives_exact_zeros(gc):
    x, off, mask, gout = operands(6, 2, 9, 11, 2, gc, 3, 3, 1, 1, 1, 1, 1, 1, 1.5)
    off = off.abs() + 1000.0
    out, grads = hip(x, off, mask, gout, (3, 3, 1, 1, 1, 1, 1, 1, 2, gc, 1.0))
    assert not out.any() and all(not g.any() for g in grads)


@pytest.mark.parametrize("geo", [(1, 3, 1, 2, 0, 1, 1, 2), (3, 1, 2, 1, 2, 0, 2, 1), (3, 5, 1, 1, 1, 2, 1, 1)],
                         ids=["1x3", "3x1", "3x5"])
def test_h_and_w_geometry_differ(geo):
    """the host-compiled reference takes one stride / pad / dilation for both axes: compared with `dcnv3_core_pytorch`
    (pinned to the reference kernels in tests/test_dcnv3_cpu.py) in fp64 on the GPU"""
    from vidar_amd.plugin.ops_dcnv3 import dcnv3_core_pytorch
    kh, kw, sh, sw, ph, pw, dh, dw = geo
    N, H, W, G, gc, os_ = 2, 11, 14, 3, 8, 1.5
    x, off, mask, gout = operands(7, N, H, W, G, gc, kh, kw, sh, sw, ph, pw, dh, dw, 1.5)
    assert away_from_minus_one(off, (H, W, kh, kw, sh, sw, ph, pw, dh, dw, G, os_))
    got_out, got_grads = hip(x, off, mask, gout, (*geo, G, gc, os_))
    xs, os, ms = (t.double().cuda().requires_grad_(True) for t in (x, off, mask))
    want = dcnv3_core_pytorch(xs, os, ms, *geo, G, gc, os_)
    want_grads = torch.autograd.grad((want * gout.double().cuda()).sum(), [xs, os, ms])
    compare("hw", got_out, got_grads, want.detach().cpu(), [g.cpu() for g in want_grads], off,
            (H, W, kh, kw, sh, sw, ph, pw, dh, dw, G, os_))


def test_kernels_match_the_reference_goldens():
    from make_dcnv3_golden import CORE_CASES
    data = np.load(GOLD / "dcnv3_core.npz")
    for case in CORE_CASES:
        n, N, H, W, G, gc = case[:6]
        x, off, mask, gout = (torch.from_numpy(data[f"{n}.{k}"]).float() for k in ("input", "offset", "mask", "grad_out"))
        got_out, got_grads = hip(x, off, mask, gout, (*case[6:14], G, gc, case[14]))
        compare(n, got_out, got_grads, torch.from_numpy(data[f"{n}.out"]),
                [torch.from_numpy(data[f"{n}.{k}"]) for k in ("grad_input", "grad_offset", "grad_mask")], off,
                (H, W, *case[6:14], G, case[14]))


def test_backward_twice_is_reproducible():
    from vidar_amd.third_lib import dcnv3
    geo = (3, 3, 1, 1, 1, 1, 1, 1, 4, 16, 1.0)
    d = [t.cuda() for t in operands(8, 2, 29, 50, 4, 16, 3, 3, 1, 1, 1, 1, 1, 1, 1.5)]
    a = dcnv3.dcnv3_backward(d[0], d[1], d[2], *geo, d[3], 256)
    b = dcnv3.dcnv3_backward(d[0], d[1], d[2], *geo, d[3], 256)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])          # plain stores, fixed order
    torch.testing.assert_close(a[0], b[0], rtol=1e-5, atol=1e-6)        # atomics: summation order


def test_non_default_stream_and_non_contiguous_grad_output():
    from vidar_amd.plugin.ops_dcnv3 import DCNv3Function, dcnv3_core_pytorch
    geo = (3, 3, 1, 1, 1, 1, 1, 1, 2, 16, 1.0)
    x, off, mask, gout = operands(9, 2, 10, 12, 2, 16, 3, 3, 1, 1, 1, 1, 1, 1, 1.5)
    gout_nc = gout.cuda().permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
    assert not gout_nc.is_contiguous()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops = [t.cuda().requires_grad_(True) for t in (x, off, mask)]
        y = DCNv3Function.apply(*ops, *geo, 256)
        grads = torch.autograd.grad(y, ops, grad_outputs=gout_nc)
    side.synchronize()
    ref_ops = [t.double().requires_grad_(True) for t in (x, off, mask)]
    want = dcnv3_core_pytorch(*ref_ops, *geo)
    want_grads = torch.autograd.grad((want * gout.double()).sum(), ref_ops)
    compare("stream", y.detach().cpu(), [g.cpu() for g in grads], want.detach(), want_grads, off,
            (10, 12, 3, 3, 1, 1, 1, 1, 1, 1, 2, 1.0))


def test_half_operands_are_computed_in_fp32_and_returned_in_their_dtype():
    from vidar_amd.plugin.ops_dcnv3 import DCNv3Function
    geo = (3, 3, 1, 1, 1, 1, 1, 1, 2, 16, 1.0)
    x, off, mask, gout = operands(10, 1, 8, 9, 2, 16, 3, 3, 1, 1, 1, 1, 1, 1, 1.5)
    for dt in (torch.float16, torch.bfloat16):
        ops = [t.cuda().to(dt).requires_grad_(True) for t in (x, off, mask)]
        y = DCNv3Function.apply(*ops, *geo, 256)
        grads = torch.autograd.grad(y, ops, grad_outputs=gout.cuda().to(dt))
        assert y.dtype == dt and all(g.dtype == dt for g in grads)
        ops32 = [t.detach().float().requires_grad_(True) for t in ops]
        y32 = DCNv3Function.apply(*ops32, *geo, 256)
        assert torch.equal(y, y32.to(dt))


def _randomise(module, seed, scale=0.05):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for _, p in sorted(module.named_parameters()):
            p.add_(scale * torch.randn(p.shape, generator=g).to(p.device))


@pytest.mark.parametrize("kw", [dict(channels=64, group=4), dict(channels=21, group=3, dw_kernel_size=5,
                                                                 center_feature_scale=True, offset_scale=2.0)],
                         ids=["gc16", "gc7_cfs"])
def test_module_hip_matches_module_pytorch(kw):
    import warnings
    from vidar_amd.plugin.ops_dcnv3 import DCNv3, DCNv3_pytorch
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a, b = DCNv3(**kw), DCNv3_pytorch(**kw)
    _randomise(a, 3)
    b.load_state_dict(a.state_dict(), strict=True)
    a.cuda(); b.double().cuda()
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 14, 17, kw["channels"], generator=g)
    gout = torch.randn(2, 14, 17, kw["channels"], generator=g).cuda()
    xa, xb = x.cuda().requires_grad_(True), x.double().cuda().requires_grad_(True)
    ya, yb = a(xa), b(xb)
    ga = torch.autograd.grad((ya * gout).sum(), [xa] + [p for _, p in sorted(a.named_parameters())])
    gb = torch.autograd.grad((yb * gout.double()).sum(), [xb] + [p for _, p in sorted(b.named_parameters())])
    names = ["out", "grad_input"] + [k for k, _ in sorted(a.named_parameters())]
    for nm, u, v in zip(names, (ya.detach(),) + ga, (yb.detach(),) + gb):
        atol = 2e-4 * max(1.0, float(v.abs().max()))
        print(f"{nm}: max |diff| {float((u.double() - v).abs().max()):.3e} (atol {atol:.1e})")
        torch.testing.assert_close(u.double(), v.detach(), rtol=2e-4, atol=atol, msg=lambda m: f"{nm}: {m}")


def _internimage(name, **over):
    import warnings
    from vidar_amd.plugin.registry import build_backbone
    meta = json.loads((GOLD / f"internimage_{name}.json").read_text())
    data = np.load(GOLD / f"internimage_{name}.npz")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = build_backbone(dict(type="InternImage", **dict(meta["kwargs"], core_op="DCNv3", **over)))
    model.load_state_dict({k[2:]: torch.from_numpy(data[k]) for k in data.files if k.startswith("w.")}, strict=True)
    return model.cuda(), data


def _internimage_grads(model, data):
    x = torch.from_numpy(data["input"]).cuda().requires_grad_(True)
    outs = model(x)
    loss = sum((o * torch.from_numpy(data[f"cot.{i}"]).cuda()).sum() for i, o in enumerate(outs))
    params = sorted(model.named_parameters())
    return outs, params, torch.autograd.grad(loss, [x] + [p for _, p in params])


@pytest.mark.parametrize("name", INTERNIMAGE_CASES)
def test_internimage_hip_matches_the_reference_golden(name):
    """fp32 through 5 DCNv3 layers against the reference in fp64: per tensor rtol 1e-3, atol 1e-3 * max(1, |ref|_max)"""
    model, data = _internimage(name)
    outs, params, grads = _internimage_grads(model, data)
    pairs = [(f"out.{i}", o, data[f"out.{i}"]) for i, o in enumerate(outs)] + [("grad_input", grads[0], data["grad_input"])]
    pairs += [("grad " + k, g, data["g." + k]) for (k, _), g in zip(params, grads[1:])]
    worst = 0.0
    for nm, got, want in pairs:
        want = torch.from_numpy(want)
        scale = max(1.0, float(want.abs().max()))
        worst = max(worst, float((got.detach().cpu().double() - want).abs().max()) / scale)
        torch.testing.assert_close(got.detach().cpu().double(), want, rtol=1e-3, atol=1e-3 * scale, msg=lambda m: f"{name} {nm}: {m}")
    print(f"{name}: worst |diff| / max(1, |ref|_max) over {len(pairs)} tensors {worst:.3e}")


def test_internimage_with_cp_gives_the_same_gradients():
    model, data = _internimage("base")
    cp_model, _ = _internimage("base", with_cp=True)
    _, _, a = _internimage_grads(model, data)
    _, _, b = _internimage_grads(cp_model, data)
    for u, v in zip(a, b):
        torch.testing.assert_close(u, v, rtol=1e-5, atol=1e-6 * max(1.0, float(v.abs().max())))


def test_whole_step_with_internimage_t_backbone():
    import copy
    import vidar_amd.plugin as P
    from vidar_amd.configs import get_config
    from vidar_amd.plugin.internimage import InternImage
    from vidar_amd.synthetic import make_sample
    torch.manual_seed(0); np.random.seed(0)
    cfg = get_config("vidar_1_8_nusc_1future", bev_h=50, bev_w=50, with_backbone="internimage_t")
    cfg["model"]["img_backbone"]["depths"] = [1, 1, 2, 1]
    cfg["model"]["use_grid_mask"] = False
    hw = (128, 224)
    model = P.build_detector(cfg["model"])
    assert isinstance(model.img_backbone, InternImage) and model.img_backbone.core_op == "DCNv3"
    _randomise(model.img_backbone, 5, scale=0.02)                       # offsets off the pixel centres of the zero init
    for m in model.modules():
        if hasattr(m, "random_drop_prev_rate"):
            m.random_drop_prev_rate = 0.0
    metas, gt = make_sample(0, future_frames=cfg["future_frames"], rays_per_frame=400, num_cams=cfg["num_cams"], img_hw=hw)
    img = torch.randn(1, len(metas), cfg["num_cams"], 3, *hw, generator=torch.Generator().manual_seed(2))
    model.cuda().train()
    losses = model(return_loss=True, img=img.cuda(), img_metas=[copy.deepcopy(metas)], gt_points=[torch.from_numpy(gt).cuda()])
    total = sum(losses.values())
    assert losses and all(torch.isfinite(v) for v in losses.values())
    total.backward()
    dead = [n for n, p in model.img_backbone.named_parameters() if p.grad is None or not torch.isfinite(p.grad).all() or not p.grad.any()]
    # the 1/4-resolution level 0 map is not an output (out_indices = (1, 2, 3)) but feeds level 1: everything has a path
    assert not dead, dead


@pytest.fixture
def variant():
    from vidar_amd._lib import lib
    prev = lib().vidar_dcnv3_set_variant(-1)
    yield lib().vidar_dcnv3_set_variant
    lib().vidar_dcnv3_set_variant(prev)


VARIANT_CASES = [c for c in SQUARE if c[0] in ("t_stage0_reduced", "gc32", "gc3", "gc12_idle_lane", "k5_pad2", "stride2_pad2_dil2",
                                               "scale2.5", "far_field", "far_field_gc3")]


@pytest.mark.parametrize("case", VARIANT_CASES, ids=[c[0] for c in VARIANT_CASES])
@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_every_backward_variant_matches_the_reference_kernels_fp64(case, which, variant, ref_modules):
    """the four forms of the grad_input accumulation (vidar_dcnv3_set_variant): same bounds, and the same grad_offset / grad_mask bits"""
    ref = ref_modules("ref_dcnv3")
    name, N, H, W, G, gc, k, s, p, d, os_, sigma = case
    x, off, mask, gout = operands(300 + VARIANT_CASES.index(case), N, H, W, G, gc, k, k, s, s, p, p, d, d, sigma)
    geo = (k, k, s, s, p, p, d, d, G, gc, os_)
    variant(which & 1)
    _, base = hip(x, off, mask, gout, geo)
    variant(which)
    got_out, got_grads = hip(x, off, mask, gout, geo)
    if which >= 2:      # the window changes where grad_input is summed, nothing else (bit 0 changes the lane order of the channel sums)
        assert torch.equal(got_grads[1], base[1]) and torch.equal(got_grads[2], base[2])
    xd, od, md, gd = (t.double() for t in (x, off, mask, gout))
    compare(f"{name} variant {which}", got_out, got_grads, ref.im2col(xd, od, md, k, k, s, p, d, G, gc, os_),
            ref.col2im(gd, xd, od, md, k, k, s, p, d, G, gc, os_), off, (H, W, k, k, s, s, p, p, d, d, G, os_))


def test_window_too_large_for_lds_takes_the_plain_form(variant, ref_modules):
    """gc = 160 with a 5x5 kernel: no tile's window fits 64 KiB, the call falls back to plain atomics"""
    ref = ref_modules("ref_dcnv3")
    N, H, W, G, gc, k = 1, 9, 10, 1, 160, 5
    x, off, mask, gout = operands(12, N, H, W, G, gc, k, k, 1, 1, 2, 2, 1, 1, 1.5)
    variant(3)
    got_out, got_grads = hip(x, off, mask, gout, (k, k, 1, 1, 2, 2, 1, 1, G, gc, 1.0))
    xd, od, md, gd = (t.double() for t in (x, off, mask, gout))
    compare("no_window", got_out, got_grads, ref.im2col(xd, od, md, k, k, 1, 2, 1, G, gc, 1.0),
            ref.col2im(gd, xd, od, md, k, k, 1, 2, 1, G, gc, 1.0), off, (H, W, k, k, 1, 1, 2, 2, 1, 1, G, 1.0))


def test_unaligned_buffers_take_the_scalar_form():
    """gc % 4 == 0 but input / grad_output / output views start one element into their storage (4-byte aligned only)"""
    from vidar_amd._lib import lib, ptr
    from vidar_amd.third_lib import dcnv3
    geo = (3, 3, 1, 1, 1, 1, 1, 1, 2, 16, 1.0)
    x, off, mask, gout = (t.cuda() for t in operands(13, 2, 9, 11, 2, 16, 3, 3, 1, 1, 1, 1, 1, 1, 1.5))
    shifted = lambda t: torch.cat([t.new_zeros(1), t.reshape(-1)])[1:].view(t.shape)
    xs, gs = shifted(x), shifted(gout)
    assert xs.is_contiguous() and xs.data_ptr() % 16 == 4 and gs.data_ptr() % 16 == 4
    want = dcnv3.dcnv3_forward(x, off, mask, *geo, 256)
    assert torch.equal(dcnv3.dcnv3_forward(xs, off, mask, *geo, 256), want)
    # an unaligned OUTPUT buffer through the C entry point
    buf = torch.empty(want.numel() + 1, device="cuda")
    rc = lib().vidar_dcnv3_forward_f32(ptr(x), ptr(off), ptr(mask), buf.data_ptr() + 4, 2, 9, 11, 3, 3, 1, 1, 1, 1, 1, 1,
                                       2, 16, 1.0, None)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(buf[1:].view(want.shape), want)
    a = dcnv3.dcnv3_backward(x, off, mask, *geo, gout, 256)
    b = dcnv3.dcnv3_backward(xs, off, mask, *geo, gs, 256)
    torch.testing.assert_close(b[0], a[0], rtol=1e-5, atol=1e-6)
    for u, v in zip(a[1:], b[1:]):                                       # another lane order of the channel sums
        torch.testing.assert_close(v, u, rtol=1e-5, atol=1e-5)


def test_bad_arguments_are_answered_without_a_launch():
    from vidar_amd._lib import BAD_ARG, lib, ptr
    L = lib()
    t = torch.zeros(64, device="cuda")
    f = 1.0

    def fwd(N, H, W, kh, kw, sh, sw, ph, pw, dh, dw, G, gc):
        return L.vidar_dcnv3_forward_f32(ptr(t), ptr(t), ptr(t), ptr(t), N, H, W, kh, kw, sh, sw, ph, pw, dh, dw, G, gc, f, None)

    def bwd(N, H, W, kh, kw, sh, sw, ph, pw, dh, dw, G, gc):
        return L.vidar_dcnv3_backward_f32(ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), N, H, W, kh, kw, sh, sw, ph, pw,
                                          dh, dw, G, gc, f, None, 0, None)
    bad = [(1, 40, 40, 25, 41, 1, 1, 20, 20, 1, 1, 1, 4),            # kh*kw = 1025 points
           (1, 4, 4, 7, 7, 1, 1, 1, 1, 1, 1, 1, 4),                  # kernel extent beyond the padded input
           (1, 4, 4, 3, 3, 1, 1, 0, 0, 2, 2, 1, 4),                  # dilated extent 5 > 4
           (1, 4, 4, 3, 3, 0, 1, 1, 1, 1, 1, 1, 4),                  # stride 0
           (1, 4, 4, 3, 3, 1, 1, -1, 1, 1, 1, 1, 4),                 # negative pad
           (1, 4, 4, 3, 3, 1, 1, 1, 1, 1, 1, 0, 4),                  # no groups
           (8, 8192, 8192, 3, 3, 1, 1, 1, 1, 1, 1, 4, 16),           # input of 2^35 elements
           (1, 8192, 8192, 3, 3, 1, 1, 1, 1, 1, 1, 4, 4)]            # input fits, offset [.., G*P*2] does not
    for args in bad:
        assert fwd(*args) == BAD_ARG and bwd(*args) == BAD_ARG, args
    assert fwd(0, 4, 4, 3, 3, 1, 1, 1, 1, 1, 1, 1, 4) == 0           # an empty batch is not an error
    torch.cuda.synchronize()
