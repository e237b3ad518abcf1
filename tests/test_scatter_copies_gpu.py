"""GPU: the private-copies shell of the seven scatter backwards (csrc/scatter_copies.h), called straight through the C
ABI with every kind of workspace a caller can hand in.

The backward entries add their atomics into 8 private copies of the gradient volume kept in the caller's workspace and
sum the copies afterwards; with no workspace, one that is too small or (latent render: float4 copy sum) misaligned they
add straight into the outputs.  The Python wrappers always pass a full workspace, so only this file runs the other half:
  full     a workspace of the advertised size        -> copies are used: the workspace's bytes change
  null     workspace = NULL (advertised byte count)  -> straight into the outputs
  short    the same buffer, one byte short           -> straight into the outputs: the workspace's bytes do not change
  offset4  latent render only: the right size, the pointer 4 bytes further -> as short
Which path ran is observed from a byte pattern written into the workspace before each call.  Outputs are pre-filled with
NaN, so every path must write all of them.

Shapes are the smallest that wrap the copy index (more than 8 workgroups of 4 rays / cells, workgroup 8 adds into copy 0
again).  Tolerances between the paths (only the order of the atomic adds differs) are those of the entry's own parity
test for the same gradient: ray entries rtol 3e-4 / atol 3e-5 x max|g| (tests/test_ray_options_gpu.py), latent render
rtol 3e-4 / atol 3e-5 x max(1, max|g|) (tests/test_latent_render_gpu.py); the dvxlr scatters get small integer values,
for which every partial sum is exact in fp32 whatever the order: torch.equal, and equal to numpy's scatter-add."""
import numpy as np
import pytest
import torch

from test_oracle_head import tensors, Fn, Z, Y, X

pytestmark = pytest.mark.gpu
PATTERN = 0xA5          # as a float 0xA5A5A5A5 = -2.87e-16: neither zero nor a sum any case produces
MODES = ("full", "null", "short")


def L():
    from vidar_amd._lib import lib
    return lib()


def P(t):
    from vidar_amd._lib import ptr
    return ptr(t)


def stream():
    return torch.cuda.current_stream().cuda_stream


def nan_like(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def run(call, shapes, nbytes, mode):
    """call(outputs, workspace pointer, workspace bytes) -> rc under workspace `mode`.
    -> (outputs on the host, True if the call wrote into the workspace)"""
    assert nbytes > 0
    ws = torch.full((nbytes + 16,), PATTERN, dtype=torch.uint8, device="cuda")
    wsp, wsn = {"full": (P(ws), nbytes), "null": (None, nbytes), "short": (P(ws), nbytes - 1),
                "offset4": (P(ws) + 4, nbytes)}[mode]
    outs = [nan_like(*s) for s in shapes]
    assert call(outs, wsp, wsn) == 0
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == PATTERN).all()), "bytes past the advertised size were written"
    return [o.cpu() for o in outs], not bool((ws == PATTERN).all())


def check_paths(call, shapes, nbytes, close, modes=MODES):
    got = {m: run(call, shapes, nbytes, m) for m in modes}
    assert got["full"][1], "a full workspace must be used (private copies)"
    for m in modes[1:]:
        assert not got[m][1], f"workspace '{m}' must be left alone (adds go straight into the outputs)"
    want = got["null"][0]
    for w in want:
        assert bool(torch.isfinite(w).all()) and float(w.abs().max()) > 0
    for m in modes:
        if m != "null":
            for g, w in zip(got[m][0], want):
                close(g, w)
    return want


# ---- ray entries: the 8 x 20 x 24 volume of tests/test_oracle_head.py, two frames ------------------------------------
def ray_close(g, w):
    torch.testing.assert_close(g, w, rtol=3e-4, atol=3e-5 * float(w.abs().max()))


def ray_inputs(name, K):
    """-> (sigma, origin, points, tindex, saved [R, *] of the forward, per-ray grad) on the GPU"""
    from vidar_amd.synthetic import dense_rays
    t, sigma = tensors()
    sigma, origin = sigma.contiguous().cuda(), t["origin_grids"][0].float().contiguous().cuda()
    gen = torch.Generator().manual_seed(K)
    if name == "gumbel":
        pts, ti = dense_rays(Fn, Z, Y, X)
    else:
        pts, ti = t["gt_grids"][0].float(), t["gt_tindex"][0].float()
    R = pts.shape[0]
    assert R >= 40 and int((ti == 0).sum()) > 0 and int((ti == 1).sum()) > 0
    pts, ti = pts.contiguous().cuda(), ti.contiguous().cuda()
    dims = (Fn, R, Z, Y, X, K, 1.0, stream())
    ent = -torch.empty(R, K + (name == "dist")).exponential_(generator=gen).log().cuda()
    if name == "ce":
        ce, lse, valid = nan_like(R), nan_like(R), nan_like(R)
        rc = L().vidar_ray_ce_fwd_f32(P(sigma), P(origin), P(pts), P(ti), P(ce), P(lse), P(valid), *dims)
        saved = lse
    elif name == "gumbel":
        dist, saved = nan_like(R), nan_like(R, 3)
        rc = L().vidar_ray_gumbel_fwd_f32(P(sigma), P(origin), P(pts), P(ti), P(ent), P(dist), P(saved), *dims)
    else:
        dist, gt_len, saved, valid = nan_like(R), nan_like(R), nan_like(R, 3), nan_like(R)
        rc = L().vidar_ray_dist_fwd_f32(P(sigma), P(origin), P(pts), P(ti), P(ent), P(dist), P(gt_len), P(saved), P(valid),
                                        *dims)
    assert rc == 0
    grad = (torch.rand(R, generator=gen) + 0.5).cuda()
    return sigma, origin, pts, ti, saved, grad


def ray_call(name, K, sigma, origin, pts, ti, saved, grad):
    fn = getattr(L(), f"vidar_ray_{name}_bwd_f32")
    R = pts.shape[0]
    return lambda outs, wsp, wsn: fn(P(sigma), P(origin), P(pts), P(ti), P(saved), P(grad), P(outs[0]), Fn, R, Z, Y, X,
                                     K, 1.0, wsp, wsn, stream())


@pytest.mark.parametrize("K", [512, 40], ids=["K512-register", "K40-streamed"])
@pytest.mark.parametrize("name", ["ce", "gumbel", "dist"])
def test_ray_backward_workspace_paths(name, K):
    nbytes = L().vidar_ray_bwd_workspace_bytes(Fn, Z, Y, X)
    assert nbytes == 8 * 4 * Fn * Z * Y * X
    check_paths(ray_call(name, K, *ray_inputs(name, K)), [(Fn, Z, Y, X)], nbytes, ray_close)


@pytest.mark.parametrize("name", ["ce", "gumbel", "dist"])
def test_ray_backward_without_rays_zeroes_the_output(name):
    sigma = tensors()[1].contiguous().cuda()
    origin = torch.zeros(Fn, 3, device="cuda")
    e = torch.empty(0, 3, device="cuda")
    call = ray_call(name, 512, sigma, origin, e, e[:, 0], e, e[:, 0])
    (g,), used = run(call, [(Fn, Z, Y, X)], L().vidar_ray_bwd_workspace_bytes(Fn, Z, Y, X), "full")
    assert used and float(g.abs().max()) == 0.0


# ---- latent render: bs = 2, 9 x 9 cells (81 cells, 4 per workgroup), 16 height bins, grid_step 1.0 -------------------
LR_BS, LR_H, LR_W, LR_Z, LR_G = 2, 9, 9, 16, 256
LR_STEP = float(np.float32(1.0 / (min(LR_H, LR_W) // 2)))
LR_DIMS = (LR_BS, LR_H, LR_W, LR_Z, LR_G, LR_STEP)
LR_MODES = MODES + ("offset4",)


def lr_close(g, w):
    torch.testing.assert_close(g, w, rtol=3e-4, atol=3e-5 * max(1.0, float(w.abs().max())))


def lr_inputs():
    gen = torch.Generator().manual_seed(9)
    occ, a, go1, go2 = (torch.randn(LR_BS, LR_H, LR_W, LR_Z, generator=gen).cuda() for _ in range(4))
    prob, feat, msum = nan_like(*occ.shape), nan_like(*occ.shape), nan_like(*occ.shape)
    assert L().vidar_latent_render_prob_fwd_f32(P(occ), P(prob), *LR_DIMS, 0, stream()) == 0
    assert L().vidar_latent_render_gather_fwd_f32(P(prob), P(a), P(feat), P(msum), *LR_DIMS, 1e-3, stream()) == 0
    return occ, a, go1, go2, prob, feat, msum


def lr_prob_call(occ, go1, dims=LR_DIMS):
    return lambda outs, wsp, wsn: L().vidar_latent_render_prob_bwd_f32(P(occ), P(go1), P(outs[0]), *dims, 0, wsp, wsn,
                                                                       stream())


def lr_gather_call(prob, a, feat, msum, go2, dims=LR_DIMS):
    return lambda outs, wsp, wsn: L().vidar_latent_render_gather_bwd_f32(
        P(prob), P(a), P(feat), P(msum), P(go2), P(outs[0]), P(outs[1]), *dims, 1e-3, wsp, wsn, stream())


def test_latent_render_prob_backward_workspace_paths():
    occ, a, go1, go2, prob, feat, msum = lr_inputs()
    nbytes = L().vidar_latent_render_bwd_workspace_bytes(LR_BS, LR_H, LR_W, LR_Z, 1)
    assert nbytes == 8 * 4 * occ.numel()
    check_paths(lr_prob_call(occ, go1), [occ.shape], nbytes, lr_close, LR_MODES)


def test_latent_render_gather_backward_workspace_paths():
    occ, a, go1, go2, prob, feat, msum = lr_inputs()
    nbytes = L().vidar_latent_render_bwd_workspace_bytes(LR_BS, LR_H, LR_W, LR_Z, 2)
    assert nbytes == 2 * 8 * 4 * occ.numel()
    check_paths(lr_gather_call(prob, a, feat, msum, go2), [occ.shape, occ.shape], nbytes, lr_close, LR_MODES)


def test_latent_render_backward_of_an_empty_batch_touches_nothing():
    occ, a, go1, go2, prob, feat, msum = lr_inputs()
    dims = (0,) + LR_DIMS[1:]
    for call, shapes, maps in ((lr_prob_call(occ, go1, dims), [occ.shape], 1),
                               (lr_gather_call(prob, a, feat, msum, go2, dims), [occ.shape, occ.shape], 2)):
        outs, used = run(call, shapes, L().vidar_latent_render_bwd_workspace_bytes(LR_BS, LR_H, LR_W, LR_Z, maps), "full")
        assert not used and all(bool(torch.isnan(o).all()) for o in outs)


# ---- dvxlr get_grad_sigma / _v2: N = 2, T = 2, a 4 x 6 x 5 volume, 40 rays of 5 samples --------------------------------
DV_N, DV_T, DV_Z, DV_Y, DV_X, DV_M, DV_L = 2, 2, 4, 6, 5, 40, 5
DV_VOL = (DV_N, DV_T, DV_Z, DV_Y, DV_X)


def dv_inputs(M=DV_M):
    """small integers everywhere: every partial sum is exact in fp32"""
    rng = np.random.default_rng(11)
    em = rng.integers(-3, 4, (DV_N, M, DV_L)).astype(np.float32)
    grp = rng.integers(-3, 4, (DV_N, M, DV_L)).astype(np.float32)
    indicator = rng.integers(-1, 2, (DV_N, M, DV_L)).astype(np.float32)
    idx = np.stack([rng.integers(0, s, (DV_N, M, DV_L)) for s in (DV_Z, DV_Y, DV_X)], -1).astype(np.float32)
    tindex = rng.integers(0, DV_T, (DV_N, M)).astype(np.float32)
    if M:
        tindex[0, [3, 17]] = -1.0
        tindex[1, [0, 33]] = np.nan
    return em, idx, tindex, indicator, grp


def dv_expected(em, idx, tindex, indicator, grp):
    g, g2 = np.zeros(DV_VOL, np.float32), np.zeros(DV_VOL, np.float32)
    for n in range(DV_N):
        for m in range(em.shape[1]):
            if not tindex[n, m] >= 0:
                continue
            z, y, x = idx[n, m].astype(np.int64).T
            np.add.at(g[n, int(tindex[n, m])], (z, y, x), em[n, m])
            np.add.at(g2[n, int(tindex[n, m])], (z, y, x), np.where(indicator[n, m] >= 0, grp[n, m], 0.0))
    return torch.from_numpy(g), torch.from_numpy(g2)


def dv_call(v2, arrays):
    em, idx, tindex, indicator, grp = (torch.from_numpy(a).cuda() for a in arrays)
    dims = (DV_N, em.shape[1], DV_L, DV_T, DV_Z, DV_Y, DV_X)
    if v2:
        return lambda outs, wsp, wsn: L().vidar_dvxlr2_get_grad_sigma_f32(
            P(em), P(idx), P(tindex), P(indicator), P(grp), P(outs[0]), P(outs[1]), *dims, wsp, wsn, stream())
    return lambda outs, wsp, wsn: L().vidar_dvxlr_get_grad_sigma_f32(P(em), P(idx), P(tindex), P(outs[0]), *dims, wsp, wsn,
                                                                     stream())


def dv_bytes(v2):
    nbytes = L().vidar_dvxlr_get_grad_sigma_workspace_bytes(*DV_VOL, 2 if v2 else 1)
    assert nbytes == (2 if v2 else 1) * 8 * 4 * int(np.prod(DV_VOL))
    return nbytes


def exact(g, w):
    assert torch.equal(g, w)


@pytest.mark.parametrize("v2", [False, True], ids=["get_grad_sigma", "get_grad_sigma_v2"])
def test_dvxlr_scatter_workspace_paths(v2):
    arrays = dv_inputs()
    want = check_paths(dv_call(v2, arrays), [DV_VOL] * (2 if v2 else 1), dv_bytes(v2), exact)
    for g, w in zip(want, dv_expected(*arrays)):
        assert torch.equal(g, w)


@pytest.mark.parametrize("v2", [False, True], ids=["get_grad_sigma", "get_grad_sigma_v2"])
def test_dvxlr_scatter_without_rays_zeroes_the_outputs(v2):
    outs, used = run(dv_call(v2, dv_inputs(M=0)), [DV_VOL] * (2 if v2 else 1), dv_bytes(v2), "full")
    assert used and all(float(o.abs().max()) == 0.0 for o in outs)
