"""GPU: measured evidence of a sweep (vidar_sweep_evidence_f32, csrc/ray_march.hip sweep_evidence_body).

1. parity: the six marches of tests/sweep_evidence_cases.py, both outputs, both modes, against the fp64 restatement; per
   march and output the max abs error over the voxels is held to 4 x the fp32 restatement's own error (recomputed here; the
   deterministic mode adds its own bound, det_bound with R (K + 1) 8 contributions); finite, >= 0;
2. all rays skipped, and R == 0, give exact zeros;
3. a ray with L == 0 and a ray with a NaN end point add nothing;
4. the deterministic mode: equal bits over two runs and over a permutation of the rays;
5. bad arguments are errors.
Shapes: 130 rays in a 2 x 4 x 10 x 96 volume (ray_stats_cases.py).

On an MI355X the kernel's own error was between 0.28 and 1.14 times the yardstick's: hit 1.00 at every march in both
modes (1.67e-6, the rounding of the end point's own weights), free 0.29 .. 1.14 in the default mode and 0.28 .. 1.14 in the
deterministic one over two runs; the test prints both figures."""
import math

import pytest
import torch

import ray_stats_cases as RC
import sweep_evidence_cases as SE

pytestmark = pytest.mark.gpu
NAMES = ("hit", "free")
_DEVICE = {}


def device_run(K, step, det):
    """(hit, free) of ray_ops.sweep_evidence on a march in the default (det False) or deterministic mode, on the CPU; once"""
    from vidar_amd import deterministic
    from vidar_amd.plugin.dense_heads import ray_ops
    key = (K, step, det)
    if key not in _DEVICE:
        c = SE.case(K, step)
        with deterministic.use(det):
            out = ray_ops.sweep_evidence(c.origin.cuda(), c.pts.cuda(), c.tindex.cuda(), SE.SHAPE, step, K)
        _DEVICE[key] = tuple(t.cpu() for t in out)
    return _DEVICE[key]


def det_bound(K, want, M=1.0):
    """the deterministic mode's own error per voxel (det_acc.h): M 2^(2h - 62) + 2^-23 |want|, h from the call's
    contribution bound R (K + 1) 8; no contribution exceeds M = 1 (a weight times a_k <= 1)"""
    h = math.ceil(math.log2(RC.R * (K + 1) * 8))
    return M * 2.0 ** (2 * h - 62) + 2.0 ** -23 * want.abs()


@pytest.mark.parametrize("K,step", SE.MARCHES, ids=SE.MARCH_IDS)
def test_parity_with_the_fp64_restatement(K, step):
    c = SE.case(K, step)
    yard = c.yardstick()
    print(f"returns beyond K * step: {c.beyond}")
    failures = []
    for det in (False, True):
        got = device_run(K, step, det)
        for name, g, want, y in zip(NAMES, got, c.want64, yard):
            assert g.shape == SE.SHAPE and g.dtype == torch.float32
            assert bool(torch.isfinite(g).all()) and float(g.min()) >= 0.0
            err = (g.double() - want).abs()
            print(f"  {'deterministic' if det else 'default':13s} {name:4s} device error {float(err.max()):.2e}   "
                  f"fp32 restatement error {y:.2e}   ratio {float(err.max()) / y if y else math.inf:.2f}   "
                  f"largest value {float(want.max()):.1f}")
            allowed = 4 * y + (det_bound(K, want) if det else 0.0)
            if not bool((err <= allowed).all()):
                failures.append((det, name, float(err.max()), y))
    assert not failures, failures


def test_skipped_rays_and_no_rays_give_exact_zeros():
    from vidar_amd import deterministic
    from vidar_amd.plugin.dense_heads import ray_ops
    c = SE.case(65, 0.25)
    origin, pts = c.origin.cuda(), c.pts.cuda()
    skipped = torch.where(torch.arange(RC.R) % 2 == 0, torch.tensor(-1.0), torch.tensor(float(RC.F_))).cuda()
    skipped[3] = float("nan")
    for det in (False, True):
        with deterministic.use(det):
            for K, step in ((65, 0.25), (512, 1.0)):
                for out in (ray_ops.sweep_evidence(origin, pts, skipped, SE.SHAPE, step, K),
                            ray_ops.sweep_evidence(origin, pts[:0], skipped[:0], SE.SHAPE, step, K)):
                    for g in out:
                        assert g.shape == SE.SHAPE and float(g.abs().max()) == 0.0


def test_zero_length_and_nan_end_points_add_nothing():
    from vidar_amd import deterministic
    from vidar_amd.plugin.dense_heads import ray_ops
    c = SE.case(64, 0.5)
    origin, tindex = c.origin.cuda(), c.tindex.cuda()
    marched = [r for r in range(RC.R) if r not in RC.SKIPPED]
    zero, nan, one, inf = marched[0], marched[1], marched[2], marched[3]
    pts = c.pts.clone()
    pts[zero] = c.origin[int(c.tindex[zero])]                        # L == 0
    pts[nan, 1] = float("nan")
    pts[one] = float("nan")
    pts[inf, 0] = float("inf")
    dead = torch.tensor([zero, nan, one, inf])
    keep = torch.ones(RC.R, dtype=torch.bool)
    keep[dead] = False
    for det in (False, True):
        with deterministic.use(det):
            got = ray_ops.sweep_evidence(origin, pts.cuda(), tindex, SE.SHAPE, 0.5, 64)
            only = ray_ops.sweep_evidence(origin, pts[dead].cuda(), tindex[dead.cuda()], SE.SHAPE, 0.5, 64)
            want = ray_ops.sweep_evidence(origin, c.pts[keep].cuda(), tindex[keep.cuda()], SE.SHAPE, 0.5, 64)
        for g, o, w in zip(got, only, want):
            assert bool(torch.isfinite(g).all()) and float(o.abs().max()) == 0.0
            if det:
                assert torch.equal(g, w)                              # the same multiset of contributions: equal bits
            assert float(w.max()) > 0.0


@pytest.mark.parametrize("K,step", [(512, 0.2), (1026, 0.125)], ids=["K512", "K1026"])
def test_deterministic_mode_gives_equal_bits(K, step):
    from vidar_amd import deterministic
    from vidar_amd.plugin.dense_heads import ray_ops
    c = SE.case(K, step)
    first = device_run(K, step, True)
    origin, pts, tindex = c.origin.cuda(), c.pts.cuda(), c.tindex.cuda()
    perm = torch.randperm(RC.R, generator=torch.Generator().manual_seed(5)).cuda()
    with deterministic.use(True):
        again = ray_ops.sweep_evidence(origin, pts, tindex, SE.SHAPE, step, K)
        shuffled = ray_ops.sweep_evidence(origin, pts[perm].contiguous(), tindex[perm].contiguous(), SE.SHAPE, step, K)
    for a, b, f in zip(again, shuffled, first):
        assert torch.equal(a.cpu(), f) and torch.equal(b.cpu(), f)
    yard = c.yardstick()
    for name, d, f, want, y in zip(NAMES, device_run(K, step, False), first, c.want64, yard):
        gap = (d.double() - f.double()).abs()
        print(f"  {name:4s} default against deterministic: max gap {float(gap.max()):.2e}, allowed at least {4 * y:.2e}")
        assert bool((gap <= 4 * y + det_bound(K, want)).all())


def test_bad_arguments_are_errors():
    from vidar_amd import deterministic
    from vidar_amd._lib import BAD_ARG, lib, ptr, stream_of
    from vidar_amd.plugin.dense_heads import ray_ops
    c = SE.case(37, 1.0)
    origin, pts, tindex = c.origin.cuda(), c.pts.cuda(), c.tindex.cuda()
    for K in (0, ray_ops.max_k() + 1):
        with pytest.raises(ValueError):
            ray_ops.sweep_evidence(origin, pts, tindex, SE.SHAPE, 1.0, K)
    with pytest.raises(ValueError):
        ray_ops.sweep_evidence(origin, pts, tindex, (RC.F_, 0, RC.Y, RC.X))
    with pytest.raises(ValueError):
        ray_ops.sweep_evidence(origin[:1], pts, tindex, SE.SHAPE)     # one origin, two frames
    with pytest.raises(ValueError):
        ray_ops.sweep_evidence(origin, pts, tindex[:-1], SE.SHAPE)
    with pytest.raises(RuntimeError):
        ray_ops.sweep_evidence(c.origin, c.pts, c.tindex, SE.SHAPE)   # no CPU path
    n = math.prod(SE.SHAPE)
    hit, free = torch.full(SE.SHAPE, 7.0, device="cuda"), torch.full(SE.SHAPE, 7.0, device="cuda")
    with deterministic.use(True):
        deterministic.sync()
        need = ray_ops.occupancy_workspace_bytes(*SE.SHAPE)
        assert need == 8 * (2 * n + 2)
        small = torch.empty(need - 8, dtype=torch.uint8, device="cuda")
        for wsp, wsn in ((None, 0), (ptr(small), need - 8)):
            rc = lib().vidar_sweep_evidence_f32(ptr(origin), ptr(pts), ptr(tindex), ptr(hit), ptr(free), RC.F_, RC.R,
                                                *SE.SHAPE[1:], 37, 1.0, wsp, wsn, stream_of(origin))
            assert rc == BAD_ARG
    torch.cuda.synchronize()
    assert float(hit.min()) == 7.0 and float(free.min()) == 7.0       # nothing was launched, nothing zeroed
