"""GPU parity of LatentRendering at other height-bin / LoRA widths than the released 16 / 16: Z = pred_height bins,
A = Z * J LoRA channels, channel ch weighted by the path probability of bin ch // J.

(a) the module against golden vectors of the reference module (tests/golden/make_latent_render_groups_golden.py);
(b, c) both stages, forward and backward, against the torch-CPU oracle, which takes any Z as it is; the grouped stage 2
    is the oracle's gather once per j on the channels a.view(.., Z, J)[..., j] -- the reference's own grouping;
(d) Z = A = 16 through the autograd function equals the old entry points bit for bit;
(e) out-of-range Z / A are refused before anything is launched.
Tolerances are those of tests/test_latent_render_gpu.py (same term counts: <= 257-term fp32 tree products / sums against
the reference's sequential cumprod / sum): module forward rtol 1e-4 / atol 1e-5 * scale, module gradients 2e-4 / 2e-5 *
scale, stages 3e-4 / 3e-5 * scale, at every size."""
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import latent_render as LR
from latent_render_groups_cases import GOLDEN_CASES, build

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).parent / "golden"
BAD_ARG = -22


def close(a, b, rtol=1e-4, atol=1e-5):
    b = torch.as_tensor(b)
    scale = max(1.0, float(b.abs().max()))
    torch.testing.assert_close(a.detach().cpu(), b, rtol=rtol, atol=atol * scale)


@pytest.mark.parametrize("name", list(GOLDEN_CASES))
def test_module_matches_reference_golden(name):
    g = np.load(GOLD / f"latent_render_groups_{name}.npz")
    mod = build(name).cuda()
    keys = [k[2:] for k in g.files if k.startswith("p_")]
    mod.load_state_dict({k: torch.from_numpy(g["p_" + k]) for k in keys}, strict=True)
    embed = torch.from_numpy(g["embed"]).cuda().requires_grad_(True)
    out = mod(embed)
    close(out, g["out"])
    params = dict(mod.named_parameters())
    grads = torch.autograd.grad((out * torch.from_numpy(g["gout"]).cuda()).sum(), [embed, *[params[k] for k in keys]])
    close(grads[0], g["grad_embed"], rtol=2e-4, atol=2e-5)
    for gr, k in zip(grads[1:], keys):
        close(gr, g["g_" + k], rtol=2e-4, atol=2e-5)


def oracle_stages(occ, a, go1, go2, Z, J, G, step, act):
    """-> (path_prob, feat, grad_occ, grad_a) of the CPU oracle"""
    bs, H, W, _ = occ.shape
    p = LR.path_prob(occ, G, step, act)
    av = a.view(bs, H, W, Z, J)
    f = torch.stack([LR.gather(p, av[..., j], G, step) for j in range(J)], -1).reshape(bs, H, W, Z * J)
    r = torch.autograd.grad((p * go1).sum() + (f * go2).sum(), [occ, a])
    return p.detach(), f.detach(), r[0], r[1]


def check_stages(bs, H, W, Z, J, step, act, fwd=(3e-4, 3e-5), bwd=(3e-4, 3e-5)):
    from vidar_amd.plugin.modules.ray_operations.latent_rendering import latent_render_gather, latent_render_path_prob
    A = Z * J
    gen = torch.Generator().manual_seed(H * 100 + W + 7 * Z + J)
    occ = torch.randn(bs, H, W, Z, generator=gen, requires_grad=True)
    a = torch.randn(bs, H, W, A, generator=gen, requires_grad=True)
    go1 = torch.randn(bs, H, W, Z, generator=gen); go2 = torch.randn(bs, H, W, A, generator=gen)
    p_ref, f_ref, g_occ, g_a = oracle_stages(occ, a, go1, go2, Z, J, 256, step, act)
    occ_d = occ.detach().cuda().requires_grad_(True); a_d = a.detach().cuda().requires_grad_(True)
    p = latent_render_path_prob(occ_d, 256, step, act)
    f = latent_render_gather(p, a_d, 256, step)
    assert p.shape == (bs, H, W, Z) and f.shape == (bs, H, W, A)
    d = torch.autograd.grad((p * go1.cuda()).sum() + (f * go2.cuda()).sum(), [occ_d, a_d])
    for name, got, want, (rtol, atol) in (("path_prob", p, p_ref, fwd), ("feat", f, f_ref, fwd),
                                          ("grad_occ", d[0], g_occ, bwd), ("grad_a", d[1], g_a, bwd)):
        err = float((got.detach().cpu() - want).abs().max())
        print(f"Z={Z} J={J} {H}x{W} step={step} {act}: {name} max|err| {err:.3e} of max|ref| {float(want.abs().max()):.3e}")
    close(p, p_ref, *fwd); close(f, f_ref, *fwd)
    close(d[0], g_occ, *bwd); close(d[1], g_a, *bwd)


GROUPS = [(1, 1), (1, 16), (2, 128), (3, 4), (4, 4), (8, 4), (16, 2), (32, 1), (64, 1)]
# J divides neither 64 nor 4: (32, 3) -- A = 96, a bin straddles the backward's 64-channel chunk boundary and adds its sum
# in two parts; (5, 13) -- A = 65, no multiple of 4 and above 64: the scalar forward with its chunk loop
STRADDLE = [(32, 3), (5, 13)]
# every (Z, J) at 2 x 2 (a single workgroup, every ray inside one cell of the centre) and at 7 x 7 (odd, 13 workgroups:
# the private-copy index wraps), both steps between them; 33 x 47 (non-square, 388 workgroups) where the oracle's
# [bs, channels, Q, 257] intermediates stay small: up to 16 bins and 32 channels
STAGE_CASES = ([(2, 2, z, j, 1.0, "sigmoid") for z, j in GROUPS + STRADDLE] +
               [(7, 7, z, j, 0.5, "sigmoid") for z, j in STRADDLE] +
               [(7, 7, z, j, (0.5, 1.0)[i % 2], ("exp", "sigmoid")[i % 2]) for i, (z, j) in enumerate(GROUPS)] +
               [(33, 47, z, j, (1.0, 0.5)[i % 2], "sigmoid") for i, (z, j) in enumerate(GROUPS) if z <= 16 and z * j <= 32])


@pytest.mark.parametrize("H,W,Z,J,step,act", STAGE_CASES)
def test_stages_match_oracle(H, W, Z, J, step, act):
    check_stages(2, H, W, Z, J, step, act)


def test_stages_match_oracle_50x50_four_bins_of_four():
    """the private copies at the centre cells, grad_prob summed over the 4 channels of a bin"""
    check_stages(1, 50, 50, 4, 4, 1.0, "sigmoid")


def test_stages_match_oracle_200x200_one_bin():
    """the full grid with one bin and one channel"""
    check_stages(1, 200, 200, 1, 1, 0.5, "sigmoid")


def test_16_16_through_the_function_is_the_old_entry_bit_for_bit():
    """guards the dispatch of A == Z to the entries without `grouped`.  The backward adds with atomics, whose order
    between waves is free: each probe has a gradient in ONE cell per sample, so that a single wave adds non-zero terms
    (the others add exact zeros) and the sums do not depend on the order of the waves."""
    from vidar_amd._lib import lib, ptr, stream_of, workspace
    from vidar_amd.plugin.modules.ray_operations.latent_rendering import _step, latent_render_gather
    bs, H, W, Z, G = 2, 9, 13, 16, 256
    gen = torch.Generator().manual_seed(3)
    prob = torch.rand(bs, H, W, Z, generator=gen).cuda().requires_grad_(True)
    a = torch.randn(bs, H, W, Z, generator=gen).cuda().requires_grad_(True)
    feat = latent_render_gather(prob, a, G, 1.0)
    L, s, step = lib(), stream_of(prob), _step(1.0, H, W)
    f0, m0 = torch.empty_like(prob), torch.empty_like(prob)
    assert L.vidar_latent_render_gather_fwd_f32(ptr(prob), ptr(a), ptr(f0), ptr(m0), bs, H, W, Z, G, step, 1e-3, s) == 0
    assert torch.equal(feat.detach(), f0)
    for i, j in ((0, 0), (4, 6), (8, 3)):                       # a corner, the centre, the last row
        go = torch.zeros(bs, H, W, Z, device="cuda")
        go[:, i, j] = torch.randn(bs, Z, generator=gen).cuda()
        gp, ga = torch.autograd.grad(feat, [prob, a], go, retain_graph=True)
        gp0, ga0 = torch.empty_like(prob), torch.empty_like(a)
        ws, wsp, wsn = workspace(L.vidar_latent_render_bwd_workspace_bytes, bs, H, W, Z, 2, like=prob)
        assert L.vidar_latent_render_gather_bwd_f32(ptr(prob), ptr(a), ptr(f0), ptr(m0), ptr(go), ptr(gp0), ptr(ga0), bs, H,
                                                    W, Z, G, step, 1e-3, wsp, wsn, s) == 0
        torch.cuda.synchronize()
        assert float(gp0.abs().max()) > 0 and float(ga0.abs().max()) > 0
        assert torch.equal(gp, gp0) and torch.equal(ga, ga0)


def test_out_of_range_channel_counts_are_refused_before_any_launch():
    from vidar_amd._lib import lib, ptr
    L, s = lib(), torch.cuda.current_stream().cuda_stream
    bs, H, W, G = 1, 3, 3, 8
    buf = [torch.full((bs * H * W * 512,), float("nan"), device="cuda") for _ in range(7)]
    p = [ptr(b) for b in buf]
    for Z in (0, 65):
        assert L.vidar_latent_render_prob_fwd_f32(p[0], p[1], bs, H, W, Z, G, 0.5, 0, s) == BAD_ARG
        assert L.vidar_latent_render_prob_bwd_f32(p[0], p[1], p[2], bs, H, W, Z, G, 0.5, 0, None, 0, s) == BAD_ARG
    for Z, A in ((3, 16), (4, 2), (2, 258), (64, 320)):          # A % Z != 0, A < Z, A > 256 (twice)
        assert L.vidar_latent_render_gather_grouped_fwd_f32(p[0], p[1], p[2], p[3], bs, H, W, Z, A, G, 0.5, 1e-3, s) == BAD_ARG
        assert L.vidar_latent_render_gather_grouped_bwd_f32(*p, bs, H, W, Z, A, G, 0.5, 1e-3, None, 0, s) == BAD_ARG
    assert L.vidar_latent_render_gather_fwd_f32(p[0], p[1], p[2], p[3], bs, H, W, 65, G, 0.5, 1e-3, s) == BAD_ARG
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(b).all()) for b in buf), "a refused call wrote to its arguments"
