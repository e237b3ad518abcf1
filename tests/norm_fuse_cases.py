"""Shared inputs and the plain restatements of tests/test_norm_fuse_{cases_cpu,direct_gpu}.py: the five entries of
csrc/norm_fuse.hip (vidar_drop_add_ln_{fwd,bwd}_f32, vidar_relu_drop_{fwd,bwd}_f32, vidar_colsum_f32).  torch and numpy
only, no GPU, no kernel of the product.  E = 2^-24 is the unit roundoff of fp32; second-order terms (E^2) are dropped
throughout and covered by the slack named with each constant.

keep(): the dropout rule, restated in numpy uint32 / uint64.  Element i (the flat index into the [rows, 256] or [n]
    tensor, 64 bits) is kept iff
        h = (uint32)i * 0x9E3779B9 ^ (uint32)(i >> 32) * 0x85EBCA6B ^ seed ;  h = murmur3_finaliser(h)
        (h >> 8) * 2^-24 >= p                                   (an fp32 comparison; both sides are exact in fp32)
    and p <= 0 keeps everything.  The mask is therefore a function of (seed, i, p) that does not come from the kernel.
    The `i >> 32` term is zero below 2^32 elements (16 GiB of fp32): it is restated but NOT tested, and neither are row
    counts beyond 2^31.  scale32(p) = fl(1 / fl(1 - p)) is the kernel's fp32 scale of a kept element.

ln_forward(): in fp64, with sc = 1 / (1 - p) of the fp32 p and the fp32 eps the entry receives,
        S = x * keep * sc + r ;  mean, var (biased) over the 256 channels ;  rstd = 1 / sqrt(var + eps) ;
        y = (S - mean) * rstd * gamma + beta.
    |S| beyond about 1e19 overflows d * d in fp32 (var = inf, rstd = 0): outside the kernel's domain; the families below
    stay under 1e16.

ln_fwd_bound(): elementwise, from the kernel's operation count.  The file is built with -ffp-contract=fast; a fused
    multiply-add rounds once where the separate form rounds twice, so counting the separate form covers both.
    d = S - mean, h = d * rstd, averages over the row:
        ds   = 2E (|x sc| + |r|)  [+ 2E |x sc| at p > 0]
               s = fl(fl(x * sc) + r): the product and the sum round once each, the sum is no larger than |x sc| + |r|;
               at p > 0 the fp32 scale fl(1 / fl(1 - p)) itself carries two roundings (the loosening over the p = 0 form)
        dm   = mean(ds) + 12E mean|S|
               the row sum is 3 in-lane additions and 6 butterfly steps, a tree of depth 9, so each term is rounded at
               most 9 times (the factor 1/256 is exact); 12 leaves 3 for the second order
        dd   = ds + dm + E |d|                              one subtraction
        dv   = 2 mean(|d| dd) + 14E var
               d^2 moves by 2 |d| dd; the product rounds once and the same depth-9 tree follows: 10, and 4 of slack
        rho  = (dv + E (var + eps)) / (2 (var + eps)) + 2E
               the relative error of rstd: var + eps rounds once, the square root halves the relative error of its
               argument, sqrtf and the division are correctly rounded (E each)
        |y - ref| <= |gamma| rstd (dd + |d| rho) + 4E |h gamma| + E |beta|
               d * rstd, * gamma and + beta round once each, the last on a value within |h gamma| + |beta|: 3, 1 of slack
    and with it  |sum_out - S| <= ds,  |mean_out - mean| <= dm,  |rstd_out - rstd| <= rho rstd.
    The constants count a TREE: a sequential 256-term sum exceeds the bound (ratio 2.1 on the spike family), so the fp32
    restatement ln_forward32() follows the kernel's order -- ((a + b) + c) + d in the lane, then the xor butterfly
    32, 16, .. 1.  A row of 256 equal values v sums exactly (2v, 3v rounded by at most half an ulp, 4v exactly again --
    a tie goes to the even mantissa, which 4v has -- then doublings), so on constant rows d = 0, y = beta bit for bit and
    rstd = fl(1 / fl(sqrt(eps))).

ln_backward(): in fp64 from the GIVEN fp32 sum_in, mean_in, rstd_in (the rounded fp64 forward, never an output of the
    kernel under test: a forward mistake cannot cancel in the backward),
        h = (s - mean) rstd ;  t = gy gamma ;  grad_residual = rstd (t - mean(t) - h mean(t h)) ;
        grad_x = grad_residual * keep * sc ;  dgamma = sum_rows gy h ;  dbeta = sum_rows gy.
    Input gradients:  K E rstd (|t| + mean|t| + |h| mean|t h|),  K = 20.  Counted: h carries 2 roundings, t 1; c1 =
        mean(t) 1 + 9 (tree); c2 = mean(t h) 1 + 2 + 1 + 9 = 13; h c2 13 + 2 + 1 = 16; the two subtractions and the
        product with rstd one each on everything before them: |t| 4, mean|t| 13, |h| mean|t h| 18 -- at most 18, 2 of
        slack.  grad_x = grad_residual * scale32 adds one product and the two roundings of the scale: K + 3.
    dgamma:  (rows + 3) E sum_rows |gy h|  -- each term carries 3 roundings (h 2, the product 1) and a sum of `rows` terms
        in ANY order at most rows - 1 more per term: the default mode combines the row slices with atomics.
    dbeta:  gy is integer-valued with rows * max|gy| <= 2^24, so every partial sum in any order is an integer below 2^24
        and exact: dbeta must EQUAL the integer sum.

relu_drop(): in fp32, as the kernel states it.  forward (x > 0 ? x : 0) * (keep ? scale32 : 0) -- a select and one
    product, so the device must give these bits: NaN -> 0 (the comparison form is fmaxf's rule), -0 -> +0, a dropped +inf
    -> inf * 0 = NaN.  backward y > 0 ? gy * fl(1 / (1 - p)) : 0.

colsum: integer-valued x with rows * max|x| <= 2^24 must be exact for the same reason as dbeta; colsum_int() is a function
    of (row, column) that tells rows and columns apart, so a dropped or doubled row and a shifted or swapped column
    change the sums.  Real-valued inputs only at rows <= 300, within the any-order bound rows E sum_r |x[r, c]|.
"""
import functools
import math

import numpy as np
import torch

import affine_act_cases as AC

E = AC.EPS
GUARD = AC.GUARD
same_bits = AC.same_bits
C = 256


# ---- the keep rule -----------------------------------------------------------------------------------------------------
def keep(seed, n, p, start=0):
    """bool numpy [n]: is element start + k kept?"""
    if p <= 0:
        return np.ones(n, dtype=bool)
    idx = np.arange(start, start + n, dtype=np.uint64)
    lo, hi = idx.astype(np.uint32), (idx >> np.uint64(32)).astype(np.uint32)
    h = lo * np.uint32(0x9E3779B9) ^ hi * np.uint32(0x85EBCA6B) ^ np.uint32(seed)
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return (h >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24) >= np.float32(p)


def scale32(p):
    return np.float32(1) / (np.float32(1) - np.float32(p)) if p > 0 else np.float32(1)


def scale64(p):
    return 1.0 / (1.0 - float(np.float32(p))) if p > 0 else 1.0


def keep_t(seed, shape, p):
    return torch.from_numpy(keep(seed, int(np.prod(shape)), p)).view(*shape)


# ---- LayerNorm(dropout(x) + residual) ----------------------------------------------------------------------------------
FAMILIES = ("normal", "offset", "tiny", "const", "spike", "cancel", "huge")
EPSES = (1e-5, 1e-12)
SEED = 0x2545F491
# forward: 4 rows per workgroup; backward: 16; the ordered second stage (one slice) unrolls by 16 past 8 partial rows
# and has a remainder: 129 -> 9 parts, 257 -> 17, 401 -> 26; the atomic one (8 slices of ceil(parts / 8)): 129 -> per 2,
# slices 5..7 empty, 1025 -> 65 parts, per 9, 2049 -> 129, per 17, 4113 -> 258, per 33
ROWS = (1, 3, 4, 5, 15, 16, 17, 63, 65, 129, 257, 401, 1025, 2049, 4113)
MAX_ROWS = max(ROWS)
GY_MAX = 8
K_IN = 20
LN_GRID = [(f, 0.0) for f in FAMILIES] + [(f, p) for f in ("normal", "offset") for p in (0.1, 0.5)]


def parts(rows):
    """partial rows the backward's first stage writes: one per workgroup of 16 rows"""
    return (rows + 15) // 16


@functools.lru_cache(maxsize=None)
def ln_case(family, away=False):
    """-> dict x, r, gy [MAX_ROWS, 256], gamma, beta [256], fp32; a test takes the first `rows` rows (the element index,
    and with it the mask, does not depend on the row count).  away: |x| >= 0.5 (normal family), so that a kept element
    changes the sum and `sum_out - r == 0` tells the dropped set.  gy is integer-valued in [-8, 8]."""
    g = torch.Generator().manual_seed(4200 + FAMILIES.index(family))
    R = MAX_ROWS
    gamma, beta = AC.scale_shift(C, g)
    a, b = torch.randn(R, C, generator=g), torch.randn(R, C, generator=g)
    if family == "normal":
        x, r = a, b
        if away:
            x = torch.where(x.abs() < 0.5, torch.where(x < 0, -0.5, 0.5), x)
    elif family == "offset":                     # mean 1000 +- 1: a one-pass variance loses every digit
        x, r = 1000.0 + a, 0.1 * b
    elif family == "tiny":                       # variance ~ 2e-6, below eps = 1e-5
        x, r = 1e-3 * a, 1e-3 * b
    elif family == "const":                      # x and r constant per row
        x, r = (3.0 * a[:, :1]).expand(R, C).contiguous(), (3.0 * b[:, :1]).expand(R, C).contiguous()
    elif family == "spike":                      # one 1e4 among 1e-2
        x, r = 1e-2 * a, 1e-2 * b
        x[torch.arange(R), torch.randint(0, C, (R,), generator=g)] = 1e4
    elif family == "cancel":                     # x ~ -r
        x = 100.0 * a
        r = -x + 1e-3 * b
    elif family == "huge":
        x, r = 1e15 * a, 1e15 * b
    else:
        raise KeyError(family)
    gy = torch.randint(-GY_MAX, GY_MAX + 1, (R, C), generator=g).float()
    assert MAX_ROWS * GY_MAX <= 2 ** 24
    return dict(x=x.float().contiguous(), r=r.float().contiguous(), gy=gy, gamma=gamma, beta=beta)


def eps32(eps):
    return float(np.float32(eps))


def ln_forward(x, r, gamma, beta, p, eps, seed):
    """fp64 -> dict S, mean, rstd, y, keep (bool, like x)"""
    kp = keep_t(seed, x.shape, p)
    S = x.double() * kp * scale64(p) + r.double()
    mean = S.mean(1)
    var = ((S - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / torch.sqrt(var + eps32(eps))
    y = (S - mean[:, None]) * rstd[:, None] * gamma.double() + beta.double()
    return dict(S=S, mean=mean, rstd=rstd, y=y, keep=kp, var=var)


def ln_fwd_bound(x, r, gamma, beta, p, eps, seed):
    """-> dict y, sum [rows, 256], mean, rstd [rows]: the absolute bounds of the module docstring"""
    f = ln_forward(x, r, gamma, beta, p, eps, seed)
    xs = (x.double() * f["keep"] * scale64(p)).abs()
    ds = 2 * E * (xs + r.double().abs()) + (2 * E * xs if p > 0 else 0.0)
    d = f["S"] - f["mean"][:, None]
    var, rstd = f["var"][:, None], f["rstd"][:, None]
    dm = ds.mean(1, keepdim=True) + 12 * E * f["S"].abs().mean(1, keepdim=True)
    dd = ds + dm + E * d.abs()
    dv = 2 * (d.abs() * dd).mean(1, keepdim=True) + 14 * E * var
    ve = var + eps32(eps)
    rho = 0.5 * (dv + E * ve) / ve + 2 * E
    hg = (d * rstd * gamma.double()).abs()
    by = gamma.double().abs() * rstd * (dd + d.abs() * rho) + 4 * E * hg + E * beta.double().abs()
    return dict(y=by, sum=ds, mean=dm[:, 0], rstd=(rho * rstd)[:, 0])


def _lanes(t):
    return np.ascontiguousarray(t.numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float32).reshape(-1, 64, 4)


def wave_sum32(v):
    """fp32 [rows, 64, 4] -> [rows]: the kernel's order, 3 in-lane additions then the xor butterfly 32 .. 1"""
    a = ((v[..., 0] + v[..., 1]) + v[..., 2]) + v[..., 3]
    lane = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        a = a + a[:, lane ^ m]
    assert a.dtype == np.float32
    return a[:, 0]


def _keep_scale32(seed, shape, p):
    return np.where(keep(seed, int(np.prod(shape)), p), scale32(p), np.float32(0)).astype(np.float32).reshape(shape)


def ln_forward32(x, r, gamma, beta, p, eps, seed):
    """the kernel's fp32 evaluation in its own order (every operation rounds on its own) -> dict of fp32 tensors"""
    xv, rv = _lanes(x), _lanes(r)
    s = xv * _keep_scale32(seed, xv.shape, p) + rv
    inv = np.float32(1.0 / C)
    mean = wave_sum32(s) * inv
    d = s - mean[:, None, None]
    var = wave_sum32(d * d) * inv
    rstd = np.float32(1) / np.sqrt(var + np.float32(eps))
    y = d * rstd[:, None, None] * _lanes(gamma) + _lanes(beta)
    t = lambda a, *shape: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).view(*shape)
    rows = xv.shape[0]
    return dict(S=t(s, rows, C), mean=t(mean, rows), rstd=t(rstd, rows), y=t(y, rows, C))


def ln_given(f):
    """the backward's fp32 inputs: the fp64 forward, rounded"""
    return f["S"].float(), f["mean"].float(), f["rstd"].float()


def ln_backward(gy, s, mean, rstd, gamma, kp, p):
    """fp64 from the given s, mean, rstd (any dtype) -> dict gres, gx, bound_res, bound_x [rows, 256] and the per-row
    terms gh = gy * h of dgamma"""
    s, mean, rstd = s.double(), mean.double()[:, None], rstd.double()[:, None]
    h = (s - mean) * rstd
    t = gy.double() * gamma.double()
    c1, c2 = t.mean(1, keepdim=True), (t * h).mean(1, keepdim=True)
    gres = rstd * (t - c1 - h * c2)
    mag = rstd.abs() * (t.abs() + t.abs().mean(1, keepdim=True) + h.abs() * (t * h).abs().mean(1, keepdim=True))
    ks = kp * scale64(p)
    return dict(gres=gres, gx=gres * ks, bound_res=K_IN * E * mag, bound_x=(K_IN + 3) * E * mag * ks, gh=gy.double() * h)


def affine_grads(b, gy, rows):
    """-> dgamma, its bound, dbeta (the exact integer sum) over the first `rows` rows"""
    gh = b["gh"][:rows]
    return gh.sum(0), (rows + 3) * E * gh.abs().sum(0), gy[:rows].double().sum(0)


def ln_backward32(gy, s, mean, rstd, gamma, p, seed):
    """the kernel's fp32 evaluation, wave sums in its order; dgamma / dbeta as sequential fp32 sums over the rows (the
    bound holds for any order) -> dict of fp32 tensors"""
    gv, sv, g = _lanes(gy), _lanes(s), _lanes(gamma)
    m, rs = mean.numpy().astype(np.float32)[:, None, None], rstd.numpy().astype(np.float32)[:, None, None]
    inv = np.float32(1.0 / C)
    h = (sv - m) * rs
    t = gv * g
    c1 = (wave_sum32(t) * inv)[:, None, None]
    c2 = (wave_sum32(t * h) * inv)[:, None, None]
    gres = rs * (t - c1 - h * c2)
    gx = gres * _keep_scale32(seed, gres.shape, p)
    rows = gv.shape[0]
    acc = lambda a: np.add.accumulate(a.reshape(rows, C), axis=0, dtype=np.float32)[-1]
    tt = lambda a, *shape: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).view(*shape)
    return dict(gres=tt(gres, rows, C), gx=tt(gx, rows, C), dgamma=tt(acc(gv * h), C), dbeta=tt(acc(gv), C))


def worst(got, ref, bnd):
    """(every element within its bound, the largest error / bound over the elements with a positive bound)"""
    err = (got.double() - ref).abs()
    ok = bool((err <= bnd).all())
    pos = bnd > 0
    return ok, (float((err[pos] / bnd[pos]).max()) if bool(pos.any()) else 0.0)


# ---- dropout(relu(x)) --------------------------------------------------------------------------------------------------
RELU_CAP = 4 * 256 * 16384                       # elements one pass of the capped grid covers
RELU_SIZES = (4, 8, 1020, 1024, 1028, RELU_CAP + 4, RELU_CAP - 4 * 256)
RELU_PS = (0.0, 0.1, 0.5)
DENORMAL = 1e-40
PLANTED = (0.0, -0.0, DENORMAL, math.inf, -math.inf, math.nan)
PLANTED_N = 1024


@functools.lru_cache(maxsize=4)
def relu_case(n):
    g = torch.Generator().manual_seed(77 + n % 1009)
    return dict(x=torch.randn(n, generator=g), gy=torch.randn(n, generator=g))


@functools.lru_cache(maxsize=4)
def relu_keep_scale(seed, n, p):
    return torch.from_numpy(_keep_scale32(seed, (n,), p))


def relu_drop(x, seed, p):
    """fp32, the kernel's statement"""
    return torch.where(x > 0, x, torch.zeros_like(x)) * relu_keep_scale(seed, x.numel(), p).view(x.shape)


def relu_drop_bwd(gy, y, p):
    sc = float(np.float32(1) / (np.float32(1) - np.float32(p)))
    return torch.where(y > 0, gy * torch.tensor(sc, dtype=torch.float32), torch.zeros_like(gy))


def same_bits_or_nan(a, b):
    """same_bits, except that any NaN equals any NaN (the sign and payload of inf * 0 are the hardware's choice)"""
    eq = (a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))
    return a.shape == b.shape and bool(eq.all())


def relu_planted(seed, p):
    """relu_case(1024) with every value of PLANTED at the first kept and at the first dropped positions (p > 0), in x and,
    shifted by one value, in gy -> (x, gy, kept positions, dropped positions)"""
    c = relu_case(PLANTED_N)
    x, gy = c["x"].clone(), c["gy"].clone()
    kp = keep(seed, PLANTED_N, p)
    kept, dropped = np.flatnonzero(kp)[:len(PLANTED)], np.flatnonzero(~kp)[:len(PLANTED)]
    vals = torch.tensor(PLANTED)
    for pos in (kept, dropped):
        x[torch.from_numpy(pos)] = vals[:len(pos)]
        gy[torch.from_numpy(pos)] = vals.roll(1)[:len(pos)]
    return x, gy, kept, dropped


# ---- column sums -------------------------------------------------------------------------------------------------------
COLSUM_MAX = 8
COLSUM_COLS = (4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096)


def rstep(cols):
    """rows one pass of a 1024-thread workgroup covers without unrolling"""
    return 4096 // cols


def _colsum_shapes():
    small = []
    for cols in COLSUM_COLS:
        rs = rstep(cols)
        for rows in sorted({1, rs - 1, rs, 4 * rs + 1}):
            small.append((rows, cols))
    # past the cap of 256 workgroups: each workgroup owns more than one unrolled pass (4 * rstep rows) and a remainder
    capped = [(256 * 4 * rstep(cols) + 5, cols) for cols in (4096, 256, 4)]
    return small, capped


COLSUM_SMALL, COLSUM_CAPPED = _colsum_shapes()
COLSUM_REAL = ((300, 256), (7, 16), (257, 4096), (300, 4))


def colsum_int(rows, cols):
    """integer-valued fp32 [rows, cols] in [-8, 8], a function of (row, column)"""
    r = torch.arange(rows, dtype=torch.int64)[:, None]
    c = torch.arange(cols, dtype=torch.int64)[None, :]
    return ((r * 7 + c * 13 + (r * c) % 5 + (r // 16) * 3 + (c // 4) * 5) % (2 * COLSUM_MAX + 1) - COLSUM_MAX).float()


def colsum_real(rows, cols):
    return torch.randn(rows, cols, generator=torch.Generator().manual_seed(rows * 4099 + cols))


def colsum_bound(x):
    return x.shape[0] * E * x.double().abs().sum(0)
