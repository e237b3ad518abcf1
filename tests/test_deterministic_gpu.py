"""GPU: the deterministic mode (vidar_amd/deterministic.py, csrc/det_acc.h).  With the mode on, the gradient scatters
are a function of the multiset of their contributions: permuting the work, changing the item order or the kernel variant,
or calling again gives the same bits -- and the results still agree with the oracles at the tolerances of the ops' own
test files (named at each check).  The repeated-call checks are statistical; the permutation and variant checks are the
ones fp32 atomics cannot pass.  Shapes: the smallest that still collide heavily.

Every test prints the figures it asserts on (pytest -s)."""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import msda as M
from oracle import head as H
from oracle import chamfer as C
from oracle import latent_render as LR

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def mode_on():
    from vidar_amd import deterministic
    with deterministic.use(True):
        yield
    assert deterministic.sync() is False            # the library switch is off again for the tests that follow


def bits_equal(a, b):
    """torch.equal on the bit patterns (NaN == NaN, -0 != +0)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def report(name, got, ref):
    err = float((got.detach().cpu().double() - ref.double()).abs().max())
    print(f"{name}: max|err| {err:.3e} of max|ref| {float(ref.abs().max()):.3e}")


# ---------------------------------------------------------------------------------------------
# MSDA grad_value
# ---------------------------------------------------------------------------------------------
SHAPES = [(12, 20), (6, 10)]
B, HEADS, CH, NQ, P = 2, 8, 32, 600, 4
NAN_AT = (0, 5, 3, 1, 2, 0)          # one location is NaN: the sample contributes nothing
MSDA_H = math.ceil(math.log2(B * NQ * HEADS * len(SHAPES) * P * 4 * CH))   # contributions of the call: 4 corners x 32 channels


@functools.lru_cache(maxsize=None)
def msda_case():
    value, sh, loc, w = M.make_case(0, B, SHAPES, NQ, H=HEADS, P=P, spread=0.02)
    assert float(loc.min()) < 0.0 and float(loc.max()) > 1.0       # zero padding is hit
    loc[NAN_AT] = float("nan")
    gout = torch.randn(B, NQ, HEADS * CH, generator=torch.Generator().manual_seed(1))
    return value, sh, loc, w, gout


def msda_reference(value, sh, loc, w, gout):
    """fp64 autograd of the gather oracle; a NaN location is a sample far outside (what it means to every kernel)"""
    v64 = value.double().requires_grad_(True)
    l64 = torch.nan_to_num(loc.double(), nan=-5.0)
    out = M.msda_gather(v64, sh, l64, w.double())
    return torch.autograd.grad((out * gout.double().view_as(out)).sum(), v64)[0]


@functools.lru_cache(maxsize=None)
def msda_ref_default():
    return msda_reference(*msda_case())


def msda_bwd(value, sh, loc, w, gout, binned=None):
    from vidar_amd.plugin.modules import multi_scale_deformable_attn_function as F
    lsi = M.level_start_index(SHAPES).cuda()
    return F._msda_backward(value.cuda(), sh.cuda(), lsi, loc.cuda(), w.cuda(), gout.cuda().contiguous(), binned=binned)


def test_msda_permuting_the_queries_gives_the_same_grad_value():
    value, sh, loc, w, gout = msda_case()
    perm = torch.randperm(NQ, generator=torch.Generator().manual_seed(2))
    a = msda_bwd(value, sh, loc, w, gout)[0]
    b = msda_bwd(value, sh, loc[:, perm].contiguous(), w[:, perm].contiguous(), gout[:, perm].contiguous())[0]
    assert torch.equal(a, b)
    assert float(a.abs().max()) > 0


def test_msda_item_order_and_repeated_calls_give_the_same_grad_value():
    from vidar_amd._lib import lib
    case = msda_case()
    outs = []
    for order in (0, 1):
        prev = lib().vidar_msda_set_item_order(order)
        try:
            outs.append(msda_bwd(*case)[0])
        finally:
            lib().vidar_msda_set_item_order(prev)
    outs += [msda_bwd(*case)[0] for _ in range(3)]
    outs.append(msda_bwd(*case, binned=True)[0])      # the mode picks the plain scatter whatever the caller asks for
    for o in outs[1:]:
        assert torch.equal(outs[0], o)


def test_msda_gathered_gradients_are_the_default_mode_s_bits():
    """grad_sampling_loc / grad_attn_weight are gathers: bit-identical to the default mode (which takes the same kernel
    form at this size: B Nq H L P < BINNED_MIN_SAMPLES)"""
    from vidar_amd import deterministic
    from vidar_amd.plugin.modules import multi_scale_deformable_attn_function as F
    assert B * NQ * HEADS * len(SHAPES) * P < F.BINNED_MIN_SAMPLES
    case = msda_case()
    _, gl, gw = msda_bwd(*case)
    with deterministic.use(False):
        gv0, gl0, gw0 = msda_bwd(*case)
    assert bits_equal(gl, gl0) and bits_equal(gw, gw0)


def test_msda_grad_value_matches_the_fp64_oracle():
    """tolerance of tests/test_msda_gpu.py for grad_value: rtol 2e-4, atol 2e-5 * max(1, max|ref|)"""
    gv = msda_bwd(*msda_case())[0]
    ref = msda_ref_default()
    report("msda grad_value", gv, ref)
    torch.testing.assert_close(gv.cpu().double(), ref, rtol=2e-4, atol=2e-5 * max(1.0, float(ref.abs().max())))


def msda_max_contribution(loc, w, g):
    """M of the call: the largest |corner weight * attention weight * grad_out| the kernel adds (fp64)"""
    gmax = g.view(B, NQ, HEADS, CH).abs().amax(-1).double()                     # [B, Nq, H]
    m = 0.0
    for l, (hl, wl) in enumerate(SHAPES):
        x = loc[:, :, :, l, :, 0].double() * wl - 0.5
        y = loc[:, :, :, l, :, 1].double() * hl - 0.5
        x0, y0 = x.floor(), y.floor()
        lw, lh = x - x0, y - y0
        inside = (y > -1) & (x > -1) & (y < hl) & (x < wl)                      # NaN: outside
        for dy, wy in ((0, 1 - lh), (1, lh)):
            for dx, wx in ((0, 1 - lw), (1, lw)):
                ok = inside & (y0 + dy >= 0) & (y0 + dy < hl) & (x0 + dx >= 0) & (x0 + dx < wl)
                c = torch.where(ok, wy * wx, torch.zeros_like(wx)) * w[:, :, :, l].double() * gmax[..., None]
                m = max(m, float(c.max()))
    return m


def test_msda_error_bound_with_six_decades_of_grad_out():
    """grad_out scaled per query by 10^U(-3, 3): |err| <= M 2^(2h - 62) + 2^-23 |ref| per address, the bound of
    det_acc.h with M = the largest contribution of the call and h from its contribution count"""
    value, sh, loc, w, gout = msda_case()
    scale = 10.0 ** (torch.rand(B, NQ, 1, generator=torch.Generator().manual_seed(3)) * 6 - 3)
    g = (gout * scale).contiguous()
    gv = msda_bwd(value, sh, loc, w, g)[0].cpu().double()
    ref = msda_reference(value, sh, loc, w, g)
    Mx = msda_max_contribution(loc, w, g)
    bound = Mx * 2.0 ** (2 * MSDA_H - 62) + 2.0 ** -23 * ref.abs()
    err = (gv - ref).abs()
    print(f"h {MSDA_H} M {Mx:.3e} max err {float(err.max()):.3e} quantisation term {Mx * 2.0 ** (2 * MSDA_H - 62):.3e} "
          f"worst err/bound {float((err / bound).max()):.3e}")
    assert bool((err <= bound).all())


def test_msda_zero_grad_out_gives_exact_zeros():
    value, sh, loc, w, gout = msda_case()
    gv = msda_bwd(value, sh, loc, w, torch.zeros_like(gout))[0]
    assert bits_equal(gv, torch.zeros_like(gv))


def test_msda_one_inf_makes_the_whole_grad_value_nan():
    """the mode's contract (the default mode poisons the touched addresses only); the call itself succeeds"""
    from vidar_amd import deterministic
    value, sh, loc, w, gout = msda_case()
    g = gout.clone()
    g[1, 17, 40] = float("inf")
    gv = msda_bwd(value, sh, loc, w, g)[0]           # check() inside raises on a bad return code
    torch.cuda.synchronize()
    assert bool(torch.isnan(gv).all())
    with deterministic.use(False):
        gv0 = msda_bwd(value, sh, loc, w, g)[0]
    assert 0 < int((~torch.isfinite(gv0)).sum()) < gv0.numel()


@pytest.mark.parametrize("merge", [0, 1])
def test_msda_fused_entry_point(merge):
    """vidar_msda_fused_bwd_f32, Qn = 2: permuted queries and repeated calls give the same grad_value, which matches the
    fp64 oracle at the tolerance of tests/test_msda_gpu.py's fused tests (rtol 3e-4, atol 3e-5 * max(1, max|ref|))"""
    from vidar_amd._lib import lib, check, ptr, stream_of
    from vidar_amd.plugin.modules import multi_scale_deformable_attn_function as F
    bs, Qn = 1, 2
    value, sh, loc, w, gout = msda_case()                      # B = bs * Qn batch rows
    assert B == bs * Qn
    gout_m = gout[:bs].contiguous() if merge else gout
    lsi = M.level_start_index(SHAPES).cuda()
    Nv = value.shape[1]
    L = len(SHAPES)

    def call(loc_, w_, g_):
        v, l, ww, g = value.cuda(), loc_.cuda().contiguous(), w_.cuda().contiguous(), g_.cuda().contiguous()
        gv = torch.empty_like(v); g_off = torch.empty(l.numel(), device="cuda"); g_logit = torch.empty(ww.numel(), device="cuda")
        ws, ws_ptr, nbytes = F._bwd_workspace(v, B, Nv, HEADS, NQ, L, P, None)
        check(lib().vidar_msda_fused_bwd_f32(ptr(v), ptr(sh.cuda()), ptr(lsi), ptr(l), ptr(ww), ptr(g), ptr(gv), ptr(g_off),
                                             ptr(g_logit), bs, Qn, Nv, HEADS, CH, NQ, L, P, merge, ws_ptr, nbytes,
                                             stream_of(v)), "fused backward")
        return gv
    a = call(loc, w, gout_m)
    perm = torch.randperm(NQ, generator=torch.Generator().manual_seed(4))
    assert torch.equal(a, call(loc[:, perm], w[:, perm], gout_m[:, perm]))
    for _ in range(2):
        assert torch.equal(a, call(loc, w, gout_m))
    g_eff = gout_m.repeat_interleave(Qn, 0) / Qn if merge else gout     # every queue entry reads its element's line / Qn
    ref = msda_reference(value, sh, loc, w, g_eff)
    report(f"fused merge={merge} grad_value", a, ref)
    torch.testing.assert_close(a.cpu().double(), ref, rtol=3e-4, atol=3e-5 * max(1.0, float(ref.abs().max())))


# ---------------------------------------------------------------------------------------------
# ray-march: 3 000 rays from one origin on a 24 x 24 x 16 volume
# ---------------------------------------------------------------------------------------------
RZ, RY, RX, RAYS = 16, 24, 24, 3000
RAY_OPTIONS = {"K512": (512, 0.125), "K37": (37, 1.0)}
MIN_GAP = 1e-4           # tests/test_ray_options_gpu.py: no hard sample may flip within fp32 logit error


@functools.lru_cache(maxsize=None)
def ray_case():
    g = torch.Generator().manual_seed(11)
    sigma = torch.randn(1, RZ, RY, RX, generator=g)
    origin = torch.tensor([[11.7, 12.4, 7.6]])
    pts = torch.rand(RAYS, 3, generator=g) * torch.tensor([RX + 8.0, RY + 8.0, RZ + 4.0]) - torch.tensor([4.0, 4.0, 2.0])
    tindex = torch.zeros(RAYS)
    tindex[::97] = -1.0                                       # padded rays
    wts = torch.rand(RAYS, generator=g) + 0.5
    return sigma, origin, pts, tindex, wts


@functools.lru_cache(maxsize=None)
def ray_reference(opt):
    """oracle gradients of the three ops for one (K, step): computed once, shared by the tests"""
    K, step = RAY_OPTIONS[opt]
    sigma, origin, pts, tindex, wts = ray_case()
    s2 = sigma.clone().requires_grad_(True)
    feat, length, keep = H.grid_features(s2, origin, pts, tindex, num=K, step=step)
    gen = torch.Generator().manual_seed(7)
    noise_d = -torch.empty(RAYS, K + 1).exponential_(generator=gen).log()
    noise_g = -torch.empty(RAYS, K).exponential_(generator=gen).log()
    for f_, n_ in ((feat.detach()[keep], noise_d[keep]), (feat.detach()[keep][:, 1:], noise_g[keep])):
        top = (f_ + n_).topk(2, dim=1).values
        assert float((top[:, 0] - top[:, 1]).min()) >= MIN_GAP
    ce = H.ce_per_ray(feat[keep])
    dd = H.gumbel_distance(feat[keep], length[keep], noise_d[keep])
    dg = H.gumbel_distance(feat[keep][:, 1:], length[keep][:, 1:], noise_g[keep])
    refs = [torch.autograd.grad((q * wts[keep]).sum(), s2, retain_graph=True)[0] for q in (ce, dd, dg)]
    assert RAYS // 3 < int(keep.sum()) < RAYS
    return keep, noise_d, noise_g, dict(zip(("ray_ce", "ray_dist", "ray_gumbel"), refs))


def ray_grad(op, opt, order=None):
    """gradient volume of `op` with the rays in `order` (a permutation; None = as they are), weights wts on kept rays"""
    from vidar_amd.plugin.dense_heads import ray_ops
    K, step = RAY_OPTIONS[opt]
    sigma, origin, pts, tindex, wts = ray_case()
    keep, noise_d, noise_g, _ = ray_reference(opt)
    w = (wts * keep).cuda()
    idx = torch.arange(RAYS) if order is None else order
    sg = sigma.cuda().requires_grad_(True)
    o, p, t = origin.cuda(), pts[idx].cuda(), tindex[idx].cuda()
    if op == "ray_ce":
        q = ray_ops.ray_ce(sg, o, p, t, step, K)[0]
    elif op == "ray_dist":
        q = ray_ops.ray_dist(sg, o, p, t, noise_d[idx].cuda(), step, K)[0]
    else:
        q = ray_ops.ray_gumbel(sg, o, p, t, noise_g[idx].cuda(), step, K)
    return torch.autograd.grad((q * w[idx.cuda()]).sum(), sg)[0]


@pytest.mark.parametrize("opt", list(RAY_OPTIONS))
@pytest.mark.parametrize("op", ["ray_ce", "ray_gumbel", "ray_dist"])
def test_ray_backward(op, opt):
    """permuted rays and three calls give the same gradient volume; K = 512 gives the same bits through the streamed
    kernels; against the oracle rtol 3e-4, atol 3e-5 * max|g_ref| (tests/test_ray_ops_gpu.py:103 /
    tests/test_ray_options_gpu.py:238 -- the form those files use where many rays add onto one voxel)"""
    from vidar_amd.plugin.dense_heads import ray_ops
    ref = ray_reference(opt)[3][op]
    a = ray_grad(op, opt)
    perm = torch.randperm(RAYS, generator=torch.Generator().manual_seed(5))
    assert torch.equal(a, ray_grad(op, opt, perm))
    for _ in range(2):
        assert torch.equal(a, ray_grad(op, opt))
    if RAY_OPTIONS[opt][0] == 512:
        with ray_ops.force_streamed():
            assert torch.equal(a, ray_grad(op, opt))
    report(f"{op} {opt} grad_sigma", a, ref)
    torch.testing.assert_close(a.cpu(), ref, rtol=3e-4, atol=3e-5 * float(ref.abs().max()))


# ---------------------------------------------------------------------------------------------
# LatentRendering, 24 x 24 BEV
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Z,A", [(16, 16), (4, 16), (1, 16), (32, 96)])
def test_latent_render_backwards(Z, A):
    """both stages: three calls give the same bits; against oracle/latent_render.py at the 3e-4 / 3e-5 * scale of
    tests/test_latent_render_groups_gpu.py.  The four cases reach the four lane widths of the mode's kernels: 16 and 4
    lanes per waypoint, (1, 16) one lane in stage 1 with J = 16, (32, 96) 64 lanes in both stages, two channel chunks and
    a bin that straddles the chunk boundary (STRADDLE of tests/test_latent_render_groups_gpu.py)"""
    from vidar_amd.plugin.modules.ray_operations.latent_rendering import latent_render_gather, latent_render_path_prob
    from test_latent_render_groups_gpu import oracle_stages, close
    bs, Hh, W, G, step, act, J = 1, 24, 24, 256, 0.5, "sigmoid", A // Z
    gen = torch.Generator().manual_seed(Z * 100 + A)
    occ = torch.randn(bs, Hh, W, Z, generator=gen, requires_grad=True)
    a = torch.randn(bs, Hh, W, A, generator=gen, requires_grad=True)
    go1 = torch.randn(bs, Hh, W, Z, generator=gen); go2 = torch.randn(bs, Hh, W, A, generator=gen)
    _, _, g_occ, g_a = oracle_stages(occ, a, go1, go2, Z, J, G, step, act)

    def grads():
        occ_d = occ.detach().cuda().requires_grad_(True); a_d = a.detach().cuda().requires_grad_(True)
        p = latent_render_path_prob(occ_d, G, step, act)
        f = latent_render_gather(p, a_d, G, step)
        return torch.autograd.grad((p * go1.cuda()).sum() + (f * go2.cuda()).sum(), [occ_d, a_d])
    first = grads()
    for _ in range(2):
        again = grads()
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    report(f"lr Z={Z} A={A} grad_occ", first[0], g_occ); report(f"lr Z={Z} A={A} grad_a", first[1], g_a)
    close(first[0], g_occ, 3e-4, 3e-5); close(first[1], g_a, 3e-4, 3e-5)


# ---------------------------------------------------------------------------------------------
# KNN grad_p2: P1 = 5 000 onto P2 = 50
# ---------------------------------------------------------------------------------------------
def test_knn_backward():
    """permuting the valid rows of p1 (with idx and grad_dist2) gives the same grad_p2 and the permuted grad_p1; against
    the oracle at tests/test_chamfer_gpu.py's tolerances (grad_p1 1e-6 / 1e-6, grad_p2 1e-5 / 1e-4)"""
    from vidar_amd.third_lib.chamferdist import _C
    from test_oracle_chamfer import clouds
    N, P1, P2 = 2, 5000, 50
    a, b = clouds(0, N, P1, P2, dup=True)
    l1 = np.array([P1, P1 - P1 // 3], np.int64); l2 = np.array([P2, P2 - P2 // 4], np.int64)
    t = lambda x: torch.from_numpy(x).cuda()
    idx, _ = _C.knn_points_idx(t(a), t(b), t(l1), t(l2), 1, -1)
    g = np.random.default_rng(1).standard_normal((N, P1, 1)).astype(np.float32)
    g1, g2 = _C.knn_points_backward(t(a), t(b), t(l1), t(l2), idx, t(g))
    for _ in range(2):
        h1, h2 = _C.knn_points_backward(t(a), t(b), t(l1), t(l2), idx, t(g))
        assert torch.equal(g1, h1) and torch.equal(g2, h2)
    rng = np.random.default_rng(2)
    perm = np.stack([np.concatenate([rng.permutation(int(l1[n])), np.arange(int(l1[n]), P1)]) for n in range(N)])
    take = lambda x: np.take_along_axis(x, perm[:, :, None], 1)
    p1, p2_ = _C.knn_points_backward(t(take(a)), t(b), t(l1), t(l2), t(take(idx.cpu().numpy())), t(take(g)))
    assert torch.equal(p2_, g2)
    assert torch.equal(p1, t(take(g1.cpu().numpy())))
    o1, o2 = C.knn_points_backward(a, b, l1, l2, idx.cpu().numpy(), g)
    report("knn grad_p2", g2, torch.from_numpy(o2))
    np.testing.assert_allclose(g1.cpu().numpy(), o1, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(g2.cpu().numpy(), o2, rtol=1e-5, atol=1e-4)


# ---------------------------------------------------------------------------------------------
# DCNv2 col2im
# ---------------------------------------------------------------------------------------------
def test_dcn_col2im():
    """N = 2, C = 16, 12 x 20, offsets ~ N(0, 1.5 px): the same grad_x under every vidar_dcn_set_variant, with and
    without the gather workspace, and on repeated calls; the whole op against oracle/dcn.py through
    tests/test_dcn_gpu.py's own check (2e-4, atol 2e-4 * max(1, max|ref|))"""
    from vidar_amd._lib import lib
    from vidar_amd.plugin.backbones import dcn_col2im
    from test_dcn_gpu import _fwd_bwd
    N, Cc, Hh, W = 2, 16, 12, 20
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, Cc, Hh, W, generator=g).cuda()
    off = (torch.randn(N, 18, Hh, W, generator=g) * 1.5).cuda()
    mask = torch.rand(N, 9, Hh, W, generator=g).cuda()
    gcols = torch.randn(N, Cc * 9, Hh * W, generator=g).cuda()
    outs = []
    for variant in (0, 1):
        prev = lib().vidar_dcn_set_variant(variant)
        try:
            for gather in (True, False):
                outs.append(dcn_col2im(gcols, x, off, mask, 3, 3, 1, 1, 1, Hh, W, gather=gather))
        finally:
            lib().vidar_dcn_set_variant(prev)
    outs += [dcn_col2im(gcols, x, off, mask, 3, 3, 1, 1, 1, Hh, W) for _ in range(2)]
    for o in outs[1:]:
        assert all(torch.equal(u, v) for u, v in zip(outs[0], o))
    assert float(outs[0][0].abs().max()) > 0
    _fwd_bwd(N, Cc, 8, Hh, W, 1)


# ---------------------------------------------------------------------------------------------
# LayerNorm affine gradients and the bias column sum: rows = 5 000, C = 256
# ---------------------------------------------------------------------------------------------
def test_layernorm_affine_gradients():
    """three calls give the same dgamma / dbeta; against torch's LayerNorm at tests/test_norm_fuse_gpu.py's tolerance
    (2e-4, atol 2e-5 * max(1, max|ref|)) and against the fp64 sum for dbeta"""
    from vidar_amd.plugin.bricks import drop_add_layernorm
    from test_norm_fuse_gpu import _setup
    x, r, norm, gy = _setup(5000)

    def grads():
        y = drop_add_layernorm(x, r, norm, 0.1, training=False)
        return torch.autograd.grad(y, [norm.weight, norm.bias], gy)
    first = grads()
    for _ in range(2):
        again = grads()
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    ref = torch.autograd.grad(norm(x + r), [norm.weight, norm.bias], gy)
    for u, v, nm in zip(first, ref, ["gamma", "beta"]):
        report(f"ln d{nm}", u, v.cpu())
        torch.testing.assert_close(u, v, rtol=2e-4, atol=2e-5 * max(1.0, float(v.abs().max())), msg=lambda m: nm + m)
    torch.testing.assert_close(first[1].double(), gy.double().sum(0), rtol=2e-4, atol=2e-5 * float(gy.double().sum(0).abs().max()))


def test_bias_column_sum():
    """gemm._colsum and the bias gradient of bricks.Linear under the mode: the same bits on every call, the fp64 column
    sums at tests/test_norm_fuse_gpu.py's colsum tolerance (1e-5, atol 2e-4 * max(1, sqrt(rows)))"""
    from vidar_amd import gemm
    from vidar_amd.plugin.bricks import Linear
    rows, cols = 5000, 256
    g2 = torch.randn(rows, cols, generator=torch.Generator().manual_seed(0)).cuda()
    outs = [gemm._colsum(g2) for _ in range(3)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    torch.testing.assert_close(outs[0].double(), g2.double().sum(0), rtol=1e-5, atol=2e-4 * max(1.0, rows ** 0.5))
    lin = Linear(64, cols).cuda()
    xin = torch.randn(rows, 64, generator=torch.Generator().manual_seed(1)).cuda()
    grads = []
    for _ in range(3):
        lin.zero_grad()
        (lin(xin) * g2).sum().backward()
        grads.append(lin.bias.grad.clone())
    assert torch.equal(grads[0], grads[1]) and torch.equal(grads[0], grads[2])
    torch.testing.assert_close(grads[0].double(), g2.double().sum(0), rtol=1e-5, atol=2e-4 * max(1.0, rows ** 0.5))


# ---------------------------------------------------------------------------------------------
# the mode off and the uncovered ops
# ---------------------------------------------------------------------------------------------
def _fused_outputs():
    from vidar_amd._lib import lib, check, ptr, stream_of
    from vidar_amd.plugin.modules import multi_scale_deformable_attn_function as F
    value, sh, loc, w, gout = (t.cuda() for t in msda_case())
    lsi = M.level_start_index(SHAPES).cuda()
    Nv, L = value.shape[1], len(SHAPES)
    gv = torch.empty_like(value); g_off = torch.empty(loc.numel(), device="cuda"); g_logit = torch.empty(w.numel(), device="cuda")
    ws, ws_ptr, nbytes = F._bwd_workspace(value, B, Nv, HEADS, NQ, L, P, None)
    check(lib().vidar_msda_fused_bwd_f32(ptr(value), ptr(sh), ptr(lsi), ptr(loc), ptr(w), ptr(gout), ptr(gv), ptr(g_off),
                                         ptr(g_logit), 1, 2, Nv, HEADS, CH, NQ, L, P, 0, ws_ptr, nbytes, stream_of(value)),
          "fused backward")
    return gv, g_off, g_logit


def _lr_outputs(Z, A):
    from vidar_amd.plugin.modules.ray_operations.latent_rendering import latent_render_gather, latent_render_path_prob
    gen = torch.Generator().manual_seed(Z * 100 + A)
    occ = torch.randn(1, 24, 24, Z, generator=gen).cuda().requires_grad_(True)
    a = torch.randn(1, 24, 24, A, generator=gen).cuda().requires_grad_(True)
    go1 = torch.randn(1, 24, 24, Z, generator=gen).cuda(); go2 = torch.randn(1, 24, 24, A, generator=gen).cuda()
    p = latent_render_path_prob(occ, 256, 0.5, "sigmoid")
    f = latent_render_gather(p, a, 256, 0.5)
    return torch.autograd.grad((p * go1).sum() + (f * go2).sum(), [occ, a])


def _knn_outputs():
    from vidar_amd.third_lib.chamferdist import _C
    from test_oracle_chamfer import clouds
    a, b = clouds(0, 2, 5000, 50, dup=True)
    t = lambda x: torch.from_numpy(x).cuda()
    l1 = t(np.array([5000, 3334], np.int64)); l2 = t(np.array([50, 38], np.int64))
    idx, _ = _C.knn_points_idx(t(a), t(b), l1, l2, 1, -1)
    g = t(np.random.default_rng(1).standard_normal((2, 5000, 1)).astype(np.float32))
    return _C.knn_points_backward(t(a), t(b), l1, l2, idx, g)


def _dcn_outputs(gather):
    from vidar_amd.plugin.backbones import dcn_col2im
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 16, 12, 20, generator=g).cuda(); off = (torch.randn(2, 18, 12, 20, generator=g) * 1.5).cuda()
    mask = torch.rand(2, 9, 12, 20, generator=g).cuda(); gcols = torch.randn(2, 144, 240, generator=g).cuda()
    return dcn_col2im(gcols, x, off, mask, 3, 3, 1, 1, 1, 12, 20, gather=gather)


def _ln_outputs():
    from vidar_amd.plugin.bricks import drop_add_layernorm
    from test_norm_fuse_gpu import _setup
    torch.manual_seed(0)                         # _setup draws gamma / beta from the global generator
    x, r, norm, gy = _setup(5000)
    y = drop_add_layernorm(x, r, norm, 0.1, training=False)
    return torch.autograd.grad(y, [norm.weight, norm.bias, x, r], gy)


def _colsum_outputs():
    from vidar_amd import gemm
    return (gemm._colsum(torch.randn(5000, 256, generator=torch.Generator().manual_seed(0)).cuda()),)


# op -> (outputs, number of leading SCATTERED outputs, rtol, atol factor of max(1, max|x|)): the tolerances the ops' own
# test files use between two summation orders or against their oracles; every other output is a gather
MODE_OFF = {
    "msda": (lambda: msda_bwd(*msda_case()), 1, 2e-4, 2e-5),
    "msda fused": (_fused_outputs, 1, 3e-4, 3e-5),
    **{f"{op} {opt}": (lambda op=op, opt=opt: (ray_grad(op, opt),), 1, 3e-4, 3e-5)
       for op in ("ray_ce", "ray_gumbel", "ray_dist") for opt in RAY_OPTIONS},
    "latent_render 16/16": (lambda: _lr_outputs(16, 16), 2, 3e-4, 3e-5),
    "latent_render 4/16": (lambda: _lr_outputs(4, 16), 2, 3e-4, 3e-5),
    "knn": (lambda: _knn_outputs()[::-1], 1, 1e-5, 1e-4),                       # (grad_p2, grad_p1)
    "dcn col2im gather": (lambda: _dcn_outputs(True), 1, 1e-4, 1e-5),
    "dcn col2im scatter": (lambda: _dcn_outputs(False), 1, 1e-4, 1e-5),
    "drop_add_ln": (_ln_outputs, 2, 2e-4, 2e-5),
    "colsum": (_colsum_outputs, 1, 1e-5, -2e-4 * 5000 ** 0.5),                  # negative: an absolute atol
}


@pytest.mark.parametrize("op", list(MODE_OFF))
def test_mode_off_against_mode_on(op):
    """every covered op with the mode off against the same call with the mode on: the gathered outputs (grad_loc,
    grad_w and the raw gradients, grad_p1, grad_offset, grad_mask, the LayerNorm input gradients) are the same bits in
    both modes -- the mode only replaces the scatter -- and the scattered outputs agree to summation order.  The default mode against the parent commit's library, both loaded in one process, is recorded in
    profiles/kbench_deterministic.md: it needs the parent's build, which a test cannot have."""
    from vidar_amd import deterministic
    from vidar_amd._lib import lib
    fn, scattered, rtol, atol = MODE_OFF[op]
    on = fn()
    with deterministic.use(False):
        assert lib().vidar_get_deterministic() == 0
        off = fn()
    assert lib().vidar_get_deterministic() == 1
    assert len(on) == len(off)
    for i, (a, b) in enumerate(zip(on, off)):
        if i < scattered:
            scale = max(1.0, float(b.abs().max()))
            print(f"{op}[{i}]: max|on - off| {float((a - b).abs().max()):.3e} of max|x| {scale:.3e}")
            torch.testing.assert_close(a, b, rtol=rtol, atol=atol * scale if atol > 0 else -atol)
        else:
            assert bits_equal(a, b), f"{op}: output {i} differs between the modes"


def test_mode_off_asks_for_the_default_workspaces():
    from vidar_amd import deterministic
    from vidar_amd._lib import lib
    from vidar_amd.plugin.modules import multi_scale_deformable_attn_function as F
    with deterministic.use(False):
        assert lib().vidar_ray_bwd_workspace_bytes(1, RZ, RY, RX) == 4 * 8 * RZ * RY * RX      # 8 private copies
        assert lib().vidar_latent_render_bwd_workspace_bytes(1, 24, 24, 16, 2) == 4 * 8 * 2 * 24 * 24 * 16
        v = torch.empty(1, device="cuda")
        assert F._bwd_workspace(v, B, 300, HEADS, NQ, 2, P, None)[0] is None                   # below BINNED_MIN_SAMPLES
        assert F._bwd_workspace(v, B, 300, HEADS, NQ, 2, P, True)[0] is not None


def test_uncovered_ops_raise_and_only_warn_under_warn_only():
    """dvxlr.get_grad_sigma on the GPU: RuntimeError naming the op under the mode; under warn_only one warning and the
    fp32-atomic result of the default mode (to summation order)"""
    import warnings
    from vidar_amd import deterministic
    from vidar_amd.synthetic import ray_set
    from vidar_amd.third_lib import dvxlr
    sigma, origin, points, tindex = (torch.from_numpy(a).cuda() for a in ray_set(seed=3, N=1, T=2, rays_per_frame=256, pad=3))
    pred, gt, dd, idx = dvxlr.render(sigma, origin, points, tindex)
    em = torch.rand_like(dd)
    with pytest.raises(RuntimeError, match="dvxlr.get_grad_sigma"):
        dvxlr.get_grad_sigma(em, idx, tindex, sigma)
    with deterministic.use(False):
        want = dvxlr.get_grad_sigma(em, idx, tindex, sigma)[0]
    deterministic._warned.discard("dvxlr.get_grad_sigma")
    with deterministic.use(True, warn_only=True):
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            got = dvxlr.get_grad_sigma(em, idx, tindex, sigma)[0]
            dvxlr.get_grad_sigma(em, idx, tindex, sigma)
        assert len([x for x in w if "dvxlr.get_grad_sigma" in str(x.message)]) == 1
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5 * max(1.0, float(want.abs().max())))
