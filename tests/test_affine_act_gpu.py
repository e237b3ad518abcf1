"""GPU: the kernels of csrc/affine_act.hip through the C ABI against the restatement of tests/affine_act_cases.py
(pinned to torch's operators by tests/test_affine_act_cases_cpu.py).

1. forward: every element within 4 * 2^-24 * (|x s| + |b| + |r|) of the fp64 reference (derived in affine_act_cases.py),
   non-finite inputs give the reference's own value, NaN under ReLU is 0;
2. backward: grad_residual = (y > 0 ? gy : 0), grad_x = grad_residual * s[c], bit for bit; without ReLU `y` is NaN-filled
   and must not matter;
3. both for relu in {0, 1} x residual in {NULL, given}, scale of both signs, at tiny planes, at and past one pass of the
   capped grid of the float4 and of the scalar kernels, with each operand in turn 4 bytes off a 16-byte boundary (every
   conjunct of the float4 test decides once), and at and past 65535 planes (N * C is gridDim.y);
4. every output is a window of a NaN-filled buffer: the 64 floats on each side are still NaN afterwards;
5. N = 0 is an empty problem, N < 0 / C <= 0 / HW <= 0 are VIDAR_ERR_BAD_ARG, and neither writes;
6. the stem: bit-identical to affine_act(relu=1) + max_pool2d, within the pooled bound of the fp64 reference, its
   argument limits, and the planted planes (negative scale, all-negative -> 0, maximum in the left halo column)."""
import math

import pytest
import torch
import torch.nn.functional as F

import affine_act_cases as AC

pytestmark = pytest.mark.gpu
G = AC.GUARD
CROSS = [(relu, res) for relu in (0, 1) for res in (False, True)]
CROSS_IDS = [f"relu{relu}-{'res' if res else 'nores'}" for relu, res in CROSS]


def abi():
    from vidar_amd._lib import lib, ptr, stream_of, BAD_ARG
    return lib(), ptr, stream_of, BAD_ARG


def window(n, off=0):
    """(buffer, window): `n` floats inside a NaN-filled buffer, G floats of guard on each side; the window starts
    4 * off bytes past a 16-byte boundary"""
    buf = torch.full((G + off + n + G,), math.nan, device="cuda")
    win = buf[G + off:G + off + n]
    assert win.data_ptr() % 16 == 4 * off
    return buf, win


def guards_intact(buf, win):
    lo = (win.data_ptr() - buf.data_ptr()) // 4
    return bool(torch.isnan(buf[:lo]).all()) and bool(torch.isnan(buf[lo + win.numel():]).all())


def placed(t, off=0):
    """`t` on the device, flat, 4 * off bytes past a 16-byte boundary"""
    buf = torch.empty(off + t.numel(), device="cuda")
    out = buf[off:]
    out.copy_(t.reshape(-1))
    assert out.data_ptr() % 16 == 4 * off
    return out


def run_fwd(c, shape, relu, res, off=()):
    """-> (y on the CPU [N, C, HW], return code); asserts the guards"""
    L, ptr, stream_of, _ = abi()
    N, C, HW = shape
    x = placed(c["x"], "x" in off)
    r = placed(c["r"], "residual" in off) if res else None
    s, b = c["s"].cuda(), c["b"].cuda()
    buf, y = window(N * C * HW, "y" in off)
    rc = L.vidar_affine_act_fwd_f32(ptr(x), ptr(s), ptr(b), ptr(r), ptr(y), N, C, HW, relu, stream_of(x))
    torch.cuda.synchronize()
    assert guards_intact(buf, y)
    return y.cpu().view(N, C, HW), rc


def check_fwd(c, shape, relu, res, off=()):
    y, rc = run_fwd(c, shape, relu, res, off)
    assert rc == 0, f"vidar_affine_act_fwd_f32 returned {rc}"
    r = c["r"] if res else None
    ref, bnd = AC.forward(c["x"], c["s"], c["b"], r, relu), AC.bound(c["x"], c["s"], c["b"], r)
    fin = torch.isfinite(bnd)
    print(f"largest error / bound {float(((y.double() - ref).abs()[fin] / bnd[fin]).max()):.3f}")
    assert AC.within(y, ref, bnd)
    return y


def check_bwd(c, shape, relu, res, off=()):
    L, ptr, stream_of, _ = abi()
    N, C, HW = shape
    n = N * C * HW
    # the mask comes from the y handed in: the fp32 forward of the case with ReLU, NaN without
    y_host = (AC.forward(c["x"], c["s"], c["b"], c["r"] if res else None, True).float() if relu
              else torch.full((N, C, HW), math.nan))
    gy, y = placed(c["gy"], "grad_y" in off), placed(y_host, "y" in off)
    s = c["s"].cuda()
    bx, gx = window(n, "grad_x" in off)
    br, gr = window(n, "grad_residual" in off) if res else (None, None)
    rc = L.vidar_affine_act_bwd_f32(ptr(gy), ptr(y), ptr(s), ptr(gx), ptr(gr), N, C, HW, relu, stream_of(gy))
    torch.cuda.synchronize()
    assert rc == 0, f"vidar_affine_act_bwd_f32 returned {rc}"
    assert guards_intact(bx, gx) and (not res or guards_intact(br, gr))
    want_x, want_r = AC.backward(c["gy"], y_host, c["s"], relu)
    assert AC.same_bits(gx.cpu().view(N, C, HW), want_x)
    if res:
        assert AC.same_bits(gr.cpu().view(N, C, HW), want_r)
    if relu and n >= 12:
        assert 0 < int((y_host > 0).sum()) < n                           # the mask passes some and stops some


@pytest.mark.parametrize("relu,res", CROSS, ids=CROSS_IDS)
@pytest.mark.parametrize("shape", AC.SHAPES, ids=AC.shape_id)
def test_forward_within_the_rounding_bound(shape, relu, res):
    check_fwd(AC.case(*shape), shape, relu, res)


@pytest.mark.parametrize("relu,res", CROSS, ids=CROSS_IDS)
@pytest.mark.parametrize("shape", AC.SHAPES, ids=AC.shape_id)
def test_backward_bits(shape, relu, res):
    check_bwd(AC.case(*shape), shape, relu, res)


def misplaced(operands, optional):
    """(operand, relu, res) for every operand that the (relu, res) crossing has"""
    cases = [(o, relu, res) for o in operands for relu, res in CROSS if res or o != optional]
    return dict(argvalues=cases, ids=[f"{o}-relu{relu}-{'res' if res else 'nores'}" for o, relu, res in cases])


@pytest.mark.parametrize("operand,relu,res", **misplaced(AC.FWD_OPERANDS, "residual"))
def test_forward_with_one_operand_off_alignment(operand, relu, res):
    check_fwd(AC.case(*AC.ALIGN_SHAPE), AC.ALIGN_SHAPE, relu, res, off=(operand,))


@pytest.mark.parametrize("operand,relu,res", **misplaced(AC.BWD_OPERANDS, "grad_residual"))
def test_backward_with_one_operand_off_alignment(operand, relu, res):
    check_bwd(AC.case(*AC.ALIGN_SHAPE), AC.ALIGN_SHAPE, relu, res, off=(operand,))


@pytest.mark.parametrize("relu,res", CROSS, ids=CROSS_IDS)
def test_scalar_loop_behind_the_alignment_route(relu, res):
    shape = AC.ALIGN_LOOP_SHAPE
    check_fwd(AC.case(*shape), shape, relu, res, off=("x",))
    check_bwd(AC.case(*shape), shape, relu, res, off=("grad_y",))


@pytest.mark.parametrize("relu,res", CROSS, ids=CROSS_IDS)
def test_planted_values(relu, res):
    """exact zero sum, -0.0, a denormal, +-inf; NaN is 0 under ReLU and NaN without"""
    c = AC.planted()
    y = check_fwd(c, AC.PLANTED_SHAPE, relu, res)
    assert float(y[0, 0, 0]) == 0.0
    nan = y[0, :, 5]
    assert bool((nan == 0).all()) if relu else bool(torch.isnan(nan).all())
    assert float(y[0, 0, 3]) == math.inf and float(y[0, 0, 4]) == (0.0 if relu else -math.inf)


def test_empty_and_bad_arguments_write_nothing():
    L, ptr, stream_of, BAD_ARG = abi()
    c = AC.case(*AC.ALIGN_SHAPE)
    x, r, s, b = placed(c["x"]), placed(c["r"]), c["s"].cuda(), c["b"].cuda()
    buf, y = window(x.numel())
    buf2, y2 = window(x.numel())
    st = stream_of(x)
    for dims, want in (((0, 3, 8), 0), ((-1, 3, 8), BAD_ARG), ((2, 0, 8), BAD_ARG), ((2, -3, 8), BAD_ARG),
                       ((2, 3, 0), BAD_ARG), ((2, 3, -8), BAD_ARG)):
        for relu in (0, 1):
            assert L.vidar_affine_act_fwd_f32(ptr(x), ptr(s), ptr(b), ptr(r), ptr(y), *dims, relu, st) == want
            assert L.vidar_affine_act_bwd_f32(ptr(x), ptr(r), ptr(s), ptr(y), ptr(y2), *dims, relu, st) == want
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all()) and bool(torch.isnan(buf2).all())


# ---- the stem ----------------------------------------------------------------------------------------------------------
def run_stem(c, shape, x_off=0, y_off=0):
    L, ptr, stream_of, _ = abi()
    N, C, H, W = shape
    Ho, Wo = (H - 1) // 2 + 1, W // 2
    x, s, b = placed(c["x"], x_off), c["s"].cuda(), c["b"].cuda()
    buf, y = window(N * C * Ho * Wo, y_off)
    rc = L.vidar_stem_bn_relu_pool_f32(ptr(x), ptr(s), ptr(b), ptr(y), N, C, H, W, stream_of(x))
    torch.cuda.synchronize()
    assert guards_intact(buf, y)
    return y.view(N, C, Ho, Wo), rc, buf


@pytest.mark.parametrize("shape", AC.STEM_SHAPES, ids=AC.shape_id)
def test_stem_equals_the_two_kernel_path_and_the_fp64_reference(shape):
    L, ptr, stream_of, _ = abi()
    c = AC.stem_case(*shape)
    N, C, H, W = shape
    y, rc, _ = run_stem(c, shape)
    assert rc == 0
    x, s, b = placed(c["x"]), c["s"].cuda(), c["b"].cuda()
    full = torch.empty(N * C * H * W, device="cuda")
    assert L.vidar_affine_act_fwd_f32(ptr(x), ptr(s), ptr(b), None, ptr(full), N, C, H * W, 1, stream_of(x)) == 0
    two = F.max_pool2d(full.view(N, C, H, W), 3, stride=2, padding=1)
    assert AC.same_bits(y.cpu(), two.cpu())
    assert AC.within(y.cpu(), AC.stem64(c["x"], c["s"], c["b"]), AC.stem_bound(c["x"], c["s"], c["b"]))
    assert bool(torch.isfinite(y).all()) and float(y.min()) >= 0.0       # -inf never leaves the kernel, NaN is 0
    if 2 <= N * C <= 16:
        assert float(y.view(N * C, -1)[1].abs().max()) == 0.0            # the all-negative plane


def test_stem_argument_limits():
    L, ptr, stream_of, BAD_ARG = abi()
    from vidar_amd.plugin.backbones import FrozenBN, stem_bn_relu_pool
    big = AC.STEM_TOO_MANY
    g = torch.Generator().manual_seed(5)
    s, b = AC.scale_shift(big[1], g)
    c = dict(x=torch.randn(*big, generator=g), s=s, b=b)
    _, rc, buf = run_stem(c, big)                                         # N * C = 65536
    assert rc == BAD_ARG and bool(torch.isnan(buf).all())
    small = (1, 2, 3, 8)
    for kw in (dict(x_off=1), dict(y_off=1)):                             # x not 16-byte, y not 8-byte aligned
        _, rc, buf = run_stem(AC.stem_case(*small), small, **kw)
        assert rc == BAD_ARG and bool(torch.isnan(buf).all())
    bn = FrozenBN(big[1]).cuda()
    with torch.no_grad():
        assert stem_bn_relu_pool(c["x"].cuda(), bn) is None                # the caller's two-kernel path
        assert stem_bn_relu_pool(torch.randn(1, 65535, 1, 4, device="cuda"), FrozenBN(65535).cuda()) is not None
