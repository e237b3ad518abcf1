"""Shared inputs and the plain restatement of tests/test_affine_act_{cases_cpu,gpu}.py: the frozen-BN epilogue
(vidar_affine_act_fwd_f32 / vidar_affine_act_bwd_f32) and the fused stem (vidar_stem_bn_relu_pool_f32) of
csrc/affine_act.hip.  torch only, no GPU, no kernel of the product.

forward(): in fp64,  v = x * s[c] + b[c] (+ r),  y = relu ? (v > 0 ? v : 0) : v.  The comparison form of the ReLU is
    the rule the kernels follow (fmaxf): NaN under ReLU comes out as 0, without ReLU it propagates.
bound(): the kernel rounds at most three times (the product or the fused multiply-add, the shift, the residual add),
    each by at most 2^-24 relative to a magnitude no larger than |x s| + |b| + |r|, so
        |y - ref| <= 4 * 2^-24 * (|x s| + |b| + |r|)
    elementwise; under ReLU the same absolute bound covers an element whose sign flips at zero (|max(a,0) - max(b,0)|
    <= |a - b|).  Where the bound itself is not finite (an infinite or NaN input) the reference is exact: +-inf, NaN or
    the 0 the ReLU makes of -inf / NaN, and `within` asks for that very value.
backward(): in fp32, as the kernel states it:  grad_residual = relu ? (y > 0 ? gy : 0) : gy,  grad_x = grad_residual *
    s[c] -- a select and one multiply, so the device must give these bits.
stem64(): max_pool2d(forward(relu=1), 3, stride 2, pad 1) in fp64.  max is 1-Lipschitz in the sup norm, so the pooled
    value is within the largest elementwise bound of its window: stem_bound() = max_pool2d(bound).
"""
import functools
import math

import torch
import torch.nn.functional as F

EPS = 2.0 ** -24
GUARD = 64                                       # floats of NaN on each side of every output window

# (N, C, HW): tiny planes; one pass of the capped 64-workgroup grid and one past it, for the float4 kernels
# (64 * 256 * 4 = 65536) and for the scalar ones (64 * 256 = 16384); at and past 65535 planes, the plane index being gridDim.y, float4 and scalar
TINY = [(2, 3, 1), (1, 5, 3), (2, 3, 4), (1, 2, 5), (1, 2, 1024), (1, 2, 1028)]
LOOPS = [(1, 2, 65536), (1, 2, 65544), (1, 2, 16385), (1, 2, 16387)]
MANY = [(1, 65535, 4), (1, 65537, 4), (33, 2048, 4), (33, 2048, 3)]
SHAPES = TINY + LOOPS + MANY
FWD_OPERANDS = ("x", "residual", "y")
BWD_OPERANDS = ("grad_y", "y", "grad_x", "grad_residual")
ALIGN_SHAPE = (2, 3, 8)                          # each operand in turn 4 bytes off a 16-byte boundary
ALIGN_LOOP_SHAPE = (1, 2, 16388)                 # HW % 4 == 0, x offset: the scalar kernel's loop by the alignment route

# (N, C, H, W) of the stem
STEM_SHAPES = [(1, 1, 1, 4), (1, 2, 2, 4), (1, 2, 3, 8), (2, 3, 5, 260), (1, 1, 33, 4), (1, 65535, 1, 4)]
STEM_TOO_MANY = (1, 65536, 1, 4)


def shape_id(s):
    return "x".join(str(v) for v in s)


def _seed(shape):
    return sum((i + 1) * 7919 * int(v) for i, v in enumerate(shape)) % (2 ** 31)


def scale_shift(C, g):
    """scale with both signs, |scale| in [0.5, 1.5] (a frozen BN weight can be negative), shift ~ N(0, 1); fp32"""
    mag = torch.rand(C, generator=g) + 0.5
    sign = torch.where(torch.arange(C) % 2 == 0, -1.0, 1.0)           # half of each; a lone channel is negative
    if C > 2:
        sign = sign[torch.randperm(C, generator=g)]
    return (mag * sign).float(), torch.randn(C, generator=g)


@functools.lru_cache(maxsize=None)
def case(N, C, HW):
    """-> dict x, r, gy [N, C, HW], s, b [C], fp32, seeded by the shape"""
    g = torch.Generator().manual_seed(_seed((N, C, HW)))
    s, b = scale_shift(C, g)
    x, r, gy = (torch.randn(N, C, HW, generator=g) for _ in range(3))
    return dict(x=x, r=r, gy=gy, s=s, b=b)


PLANTED_SHAPE = (1, 4, 8)
DENORMAL = 1e-40


@functools.lru_cache(maxsize=None)
def planted():
    """case(1, 4, 8) with channel 0 = (s 1, b -1) and, in every channel, x = [1, -0.0, denormal, +inf, -inf, NaN, ...]:
    x = 1 in channel 0 is the exact zero sum.  r is 0 at the planted positions of channel 0, finite elsewhere."""
    c = {k: v.clone() for k, v in case(*PLANTED_SHAPE).items()}
    c["s"][0], c["b"][0] = 1.0, -1.0
    c["x"][0, :, :6] = torch.tensor([1.0, -0.0, DENORMAL, math.inf, -math.inf, math.nan])
    c["r"][0, 0, :3] = 0.0
    assert 0 < float(c["x"][0, 0, 2]) < 2.0 ** -126 and float(c["b"].abs().min()) > 1e-3
    return c


def _per_channel(t, like):
    return t.view(1, -1, *([1] * (like.dim() - 2)))


def forward(x, s, b, r, relu):
    """fp64 reference; x [N, C, ...], s, b [C], r like x or None"""
    v = x.double() * _per_channel(s.double(), x) + _per_channel(b.double(), x)
    if r is not None:
        v = v + r.double()
    return torch.where(v > 0, v, torch.zeros_like(v)) if relu else v


def bound(x, s, b, r):
    m = (x.double() * _per_channel(s.double(), x)).abs() + _per_channel(b.double(), x).abs()
    if r is not None:
        m = m + r.double().abs()
    return 4 * EPS * m


def within(y, ref, bnd):
    """every element: |y - ref| <= bnd where bnd is finite, the reference's own value (NaN == NaN) where it is not"""
    y = y.double()
    loose = torch.isfinite(bnd)
    ok = torch.where(loose, (y - ref).abs() <= bnd, (y == ref) | (torch.isnan(y) & torch.isnan(ref)))
    return bool(ok.all())


def backward(gy, y, s, relu):
    """-> (grad_x, grad_residual) in fp32, the kernel's own statement"""
    gres = torch.where(y > 0, gy, torch.zeros_like(gy)) if relu else gy.clone()
    return gres * _per_channel(s, gy), gres


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- the stem ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stem_case(N, C, H, W):
    """x [N, C, H, W], s, b.  Planted planes (by flat plane index p = n * C + c, where the shape has them):
    p = 0: NaN at [0, 0] (ReLU makes it 0);  p = 1: every x s + b < 0, the pooled plane is 0;  W >= 8, the last plane
    (plane 0 of a two-plane map): its largest value in column 4 t - 1 of the last float4 column t, the kernel's left
    halo p[-1]."""
    g = torch.Generator().manual_seed(_seed((N, C, H, W)))
    s, b = scale_shift(C, g)
    x = torch.randn(N, C, H, W, generator=g)
    flat = x.view(N * C, H, W)
    if N * C <= 16:
        flat[0, 0, 0] = math.nan
        if N * C >= 2:
            c = 1 % C
            flat[1] = -(flat[1].abs() + b[c].abs() + 1.0) / s[c]
        if W >= 8:
            p = N * C - 1 if N * C >= 3 else 0
            flat[p, H // 2, 4 * (W // 4 - 1) - 1] = 100.0 * torch.sign(s[p % C])
    return dict(x=x, s=s, b=b)


def pool(t):
    return F.max_pool2d(t, 3, stride=2, padding=1)


def stem64(x, s, b):
    return pool(forward(x, s, b, None, True))


def stem_bound(x, s, b):
    bnd = bound(x, s, b, None)
    return pool(torch.where(torch.isfinite(bnd), bnd, torch.zeros_like(bnd)))      # NaN -> 0 exactly: adds nothing
