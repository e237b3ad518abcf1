"""Shared inputs and the plain restatement of tests/test_sca_gather_{cases_cpu,gpu}.py: the visible-query plan
(vidar_sca_plan_f32) and the two row gathers built on its tables (vidar_sca_rows_f32 / vidar_sca_combine_f32) of
csrc/bev_prep.hip.  torch + numpy only, no GPU, no kernel of the product.

The plan.  F = 2 frames, B = 2 batch items, N = 3 cameras, D = 4 anchors per pillar.  In batch item 0 of either frame one
camera sees nothing (every depth is -50), one sees every query (constant depth 10, u and v in [0.1, 0.9]) and one is
mixed; batch item 1 has other matrices, cameras that see and do not see in other places, so a list taken from the wrong
item differs.  The mixed cameras are of two kinds: `flat` keeps the depth in [14, 26] and lets u, v run past both image
borders; `pinhole` is a real camera at the origin, so its depth crosses the threshold.

project64(): u, v, cz of every anchor in fp64.  anchors(): drawn in [0, 1] and REDRAWN while one of them is, in any
(frame, item, camera), within 1e-3 of the depth threshold, or within 1e-3 * max(1, 1 / cz) of an image border.  Why the
scaling: the fp32 depth is a four-term sum of magnitudes below ~110, off by at most 4 * 2^-24 * 110 < 3e-5 =: e, so u and
v (quotients by cz) are off by about |u| e / cz relative to a border they sit near; 1e-3 / cz is 33 times that for any
cz >= 1e-3, and 1e-3 is 33 times it from cz = 1 on.  Outside these margins the kernel's strict fp32 comparisons MUST
agree with fp64, so every table is compared exactly and no anchor is excluded.
tables(): from the fp64 mask, the tables as include/vidar_hip.h states them.

The gathers.  Hand-built tables (not a plan's): Q = 37 queries of which five are visible to no camera; camera 0 sees the
other 32, camera 1 half of them, camera 2 three, two of which camera 1 sees too (three-term sums, where the order of
the additions shows in the bits); the visible queries sit in their camera's list in SHUFFLED order (slot !=
rank), `idx` of the slots past the list points at the unseen queries, whose source rows are NaN.  rows32() / combine32()
restate the kernels in sequential fp32 (bev_prep.hip is built without contraction: the device must give these bits);
combine64() and its bound  N * 2^-24 * sum|terms| / count  (N - 1 additions and one division, each rounding once relative
to at most the sum of magnitudes) hold combine32 and the device to fp64.
"""
import functools

import numpy as np
import torch

EPS = 2.0 ** -24
GUARD = 64

# ---- the plan ----------------------------------------------------------------------------------------------------------
NF, NB, NCAM, ND = 2, 2, 3, 4
PLAN_Q = [1, 63, 64, 1023, 1024, 1025, 2500]               # one, exactly one and several 1024-query chunks of the compaction
PC_RANGE = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
IMG_H, IMG_W = 480.0, 800.0
Z_EPS = float(np.float32(1e-5))
MARGIN = 1e-3
MAX_REDRAWS = 20


def cam_nothing():
    return [[0, 0, 0, 1.0], [0, 0, 0, 1.0], [0, 0, 0, -50.0], [0, 0, 0, 1.0]]


def cam_everything():
    kx, ky = 10 * IMG_W * 0.8 / 102.4, 10 * IMG_H * 0.8 / 102.4
    return [[kx, 0, 0, 10 * IMG_W * 0.5], [0, ky, 0, 10 * IMG_H * 0.5], [0, 0, 0, 10.0], [0, 0, 0, 1.0]]


def cam_flat(fx, fy, tilt):
    """depth 20 + tilt * x;  u = 0.5 + fx y / (cz W),  v = 0.5 + fy z / (cz H)"""
    return [[0.5 * IMG_W * tilt, fx, 0, 0.5 * IMG_W * 20], [0.5 * IMG_H * tilt, 0, fy, 0.5 * IMG_H * 20],
            [tilt, 0, 0, 20.0], [0, 0, 0, 1.0]]


def cam_pinhole(yaw, f=400.0):
    """at the origin, looking along (cos yaw, sin yaw, 0), z up"""
    c, s = np.cos(yaw), np.sin(yaw)
    fwd, left = np.array([c, s, 0.0]), np.array([-s, c, 0.0])
    r0 = -f * left + 0.5 * IMG_W * fwd
    r1 = np.array([0.0, 0.0, -f]) + 0.5 * IMG_H * fwd
    return [[*r0, 0.0], [*r1, 0.0], [*fwd, 0.0], [0, 0, 0, 1.0]]


def lidar2img():
    """[F, B, N, 4, 4] fp32"""
    m = [[[cam_nothing(), cam_everything(), cam_flat(312.0, 1500.0, 0.1)],
          [cam_everything(), cam_pinhole(0.3), cam_nothing()]],
         [[cam_pinhole(1.0), cam_nothing(), cam_everything()],
          [cam_flat(-250.0, 1200.0, -0.08), cam_flat(312.0, 1500.0, 0.1), cam_pinhole(2.5)]]]
    return torch.tensor(np.asarray(m, dtype=np.float64), dtype=torch.float32)


def project64(ref_3d, l2i):
    """ref_3d [D, Q, 3], l2i [F, B, N, 4, 4] -> u, v, cz [F, N, B, Q, D] float64 (the layout of ref_cam / bev_mask)"""
    lo = torch.tensor(PC_RANGE[:3], dtype=torch.float64)
    span = torch.tensor(PC_RANGE[3:], dtype=torch.float64) - lo
    pts = ref_3d.double() * span + lo
    m = l2i.double()
    cam = torch.einsum("fbnij,dqj->fnbqdi", m[..., :3, :3], pts) + m[..., :3, 3].permute(0, 2, 1, 3)[:, :, :, None, None]
    cz = cam[..., 2]
    den = cz.clamp(min=Z_EPS)
    return cam[..., 0] / den / IMG_W, cam[..., 1] / den / IMG_H, cz


def border_distance(u, v):
    return torch.stack((u.abs(), (u - 1).abs(), v.abs(), (v - 1).abs())).min(0).values


def too_close(u, v, cz):
    """[F, N, B, Q, D] bool: the redraw rule of anchors()"""
    scale = torch.where(cz > Z_EPS, (1.0 / cz.clamp(min=Z_EPS)).clamp(min=1.0), torch.ones_like(cz))
    return ((cz - Z_EPS).abs() < MARGIN) | (border_distance(u, v) < MARGIN * scale)


@functools.lru_cache(maxsize=None)
def anchors(Q, seed=11):
    """-> (ref_3d [D, Q, 3] fp32 in [0, 1], number of redraw rounds)"""
    g = torch.Generator().manual_seed(seed + Q)
    ref = torch.rand(ND, Q, 3, generator=g)
    l2i = lidar2img()
    for rounds in range(MAX_REDRAWS + 1):
        bad = too_close(*project64(ref, l2i)).any(0).any(0).any(0).t()             # [D, Q]
        if not bool(bad.any()):
            return ref, rounds
        ref[bad] = torch.rand(int(bad.sum()), 3, generator=g)
    raise AssertionError(f"anchors(Q={Q}) still has {int(bad.sum())} borderline anchors after {MAX_REDRAWS} redraws")


def mask64(u, v, cz):
    return (cz > Z_EPS) & (v > 0) & (v < 1) & (u < 1) & (u > 0)


def tables(mask):
    """mask [F, N, B, Q, D] bool -> dict count [F, B, Q] f32, lens [F, N] i32, idx [F, N, Q] i64, valid [F, N, Q] u8,
    slot_of [F, N, Q] i32, as include/vidar_hip.h states them"""
    Fr, N, B, Q, _ = mask.shape
    vis = mask.any(-1)                                                              # [F, N, B, Q]
    count = vis.sum(1).clamp(min=1).float()
    lens = torch.zeros(Fr, N, dtype=torch.int32)
    idx = torch.zeros(Fr, N, Q, dtype=torch.int64)
    valid = torch.zeros(Fr, N, Q, dtype=torch.uint8)
    slot_of = torch.full((Fr, N, Q), -1, dtype=torch.int32)
    for f in range(Fr):
        for n in range(N):
            seen = torch.nonzero(vis[f, n, 0]).view(-1)                             # batch item 0, ascending
            k = seen.numel()
            lens[f, n] = k
            idx[f, n] = torch.cat((seen, torch.arange(k, Q)))                       # filler: the slot number itself
            valid[f, n, :k] = 1
            slot_of[f, n, seen] = torch.arange(k, dtype=torch.int32)
    return dict(count=count, lens=lens, idx=idx, valid=valid, slot_of=slot_of)


@functools.lru_cache(maxsize=None)
def plan_case(Q):
    ref, _ = anchors(Q)
    l2i = lidar2img()
    u, v, cz = project64(ref, l2i)
    mask = mask64(u, v, cz)
    return dict(ref_3d=ref, l2i=l2i, u=u, v=v, cz=cz, mask=mask, **tables(mask))


# ---- the gathers -------------------------------------------------------------------------------------------------------
GN, GQ = 3, 37
GATHER_CASES = [(B, C, S, cnt) for B in (1, 2) for C in (4, 256, 260) for S in (0, 5, 37) for cnt in (False, True)]


def gather_id(c):
    return f"B{c[0]}-C{c[1]}-S{c[2]}-{'count' if c[3] else 'nocount'}"


@functools.lru_cache(maxsize=None)
def gather_tables():
    """-> dict idx [N, Q] i64, valid [N, Q] u8, slot_of [N, Q] i32, lens (list), dead [Q] bool, count [2, Q] f32 in {1, 2, 3}"""
    g = torch.Generator().manual_seed(23)
    dead = torch.arange(GQ) % 7 == 3                                                 # 3, 10, 17, 24, 31: no camera sees them
    live = torch.nonzero(~dead).view(-1)
    some = live[torch.randperm(live.numel(), generator=g)]
    half = live.numel() // 2
    seen = [live, some[:half], some[half - 2:half + 1]]             # two queries are seen by all three cameras
    unseen = torch.nonzero(dead).view(-1)
    idx = torch.zeros(GN, GQ, dtype=torch.int64)
    valid = torch.zeros(GN, GQ, dtype=torch.uint8)
    slot_of = torch.full((GN, GQ), -1, dtype=torch.int32)
    for n, q in enumerate(seen):
        q = q[torch.randperm(q.numel(), generator=g)]
        k = q.numel()
        idx[n, :k] = q
        idx[n, k:] = unseen[torch.arange(GQ - k) % unseen.numel()]
        valid[n, :k] = 1
        slot_of[n, q] = torch.arange(k, dtype=torch.int32)
    count = torch.randint(1, 4, (2, GQ), generator=g).float()
    return dict(idx=idx, valid=valid, slot_of=slot_of, lens=[int(q.numel()) for q in seen], dead=dead, count=count)


@functools.lru_cache(maxsize=None)
def gather_inputs(B, C, S):
    """x [B, Q, C] (rows' source), y [B, N, S, C] (combine's source), finite; and the same with NaN where the kernels
    must not read: x_nan at the unseen queries, y_nan at the slots past each camera's list"""
    t = gather_tables()
    g = torch.Generator().manual_seed(1000 * B + 10 * C + S)
    x, y = torch.randn(B, GQ, C, generator=g), torch.randn(B, GN, S, C, generator=g)
    x_nan, y_nan = x.clone(), y.clone()
    x_nan[:, t["dead"]] = float("nan")
    for n, k in enumerate(t["lens"]):
        y_nan[:, n, k:] = float("nan")
    return dict(x=x, y=y, x_nan=x_nan, y_nan=y_nan)


def rows32(src, idx, valid, count, S):
    """src [B, Q, C] -> [B, N, S, C]: valid ? src[b, idx] (/ count[b, idx]) : 0, in src's dtype"""
    sel = idx[:, :S]
    out = src[:, sel]
    if count is not None:
        out = out / count.to(src.dtype)[:, sel][..., None]
    return torch.where(valid[:, :S].bool()[None, :, :, None], out, torch.zeros_like(out))


def combine32(src, slot_of, count, S):
    """src [B, N, S, C] -> [B, Q, C]: cameras added in the order 0, 1, 2 onto 0, then one division; in src's dtype"""
    B, N, _, C = src.shape
    acc = torch.zeros(B, slot_of.shape[1], C, dtype=src.dtype)
    for n in range(N):
        s = slot_of[n].long()
        ok = (s >= 0) & (s < S)
        if bool(ok.any()):
            acc[:, ok] = acc[:, ok] + src[:, n, s[ok]]
    return acc / count.to(src.dtype)[..., None] if count is not None else acc


def combine_bound(src, slot_of, count, S):
    """N * 2^-24 * sum |terms| (/ count)"""
    return src.shape[1] * EPS * combine32(src.double().abs(), slot_of, count.double() if count is not None else None, S)


def adjoint_terms(x, y, idx, valid, count, S):
    """sum over the pairs the two gathers connect of |x| |y| / count, fp64: the magnitude both inner products round against"""
    return float((rows32(x.double().abs(), idx, valid, count.double() if count is not None else None, S)
                  * y.double().abs()).sum())
