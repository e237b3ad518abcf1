"""GPU: the kernels of csrc/bev_prep.hip through the C ABI against the restatement of tests/sca_gather_cases.py (pinned
to the module's torch formulation by tests/test_sca_gather_cases_cpu.py).

1. vidar_sca_plan_f32 on synthetic cameras at Q = 1 .. 2500 (one, exactly one, several 1024-query chunks of the
   compaction): bev_mask, count, lens, idx (list AND filler), valid and slot_of EXACTLY as fp64 gives them -- every
   anchor is kept clear of the borders and of the depth threshold by construction, none is excluded; ref_cam to fp32
   rounding on the anchors at least 1 deep;
2. vidar_sca_rows_f32: the bits of src[b, idx] / count[b, idx] in fp32, exactly 0 on the slots past a camera's list --
   whose idx points at NaN rows, so a kernel that multiplied by the flag would show;
3. vidar_sca_combine_f32: the bits of the sequential fp32 sum over the cameras 0, 1, 2 and one division, and within
   N * 2^-24 * sum|terms| of fp64; slots >= S, -1 and the NaN rows past a camera's list add nothing;
4. <rows(x), y> == <x, combine(y)> in fp64, to the roundings of the two;
5. outputs are windows of NaN-filled buffers whose 64-float guards survive; B = 0, and S = 0 for rows, write nothing and
   return 0 (combine at S = 0 has outputs, the empty sums: it writes its zeros, which SpatialCrossAttention relies on
   when no camera sees anything); bad arguments return VIDAR_ERR_BAD_ARG and write nothing."""
import ctypes
import math

import pytest
import torch

import sca_gather_cases as SC

pytestmark = pytest.mark.gpu
G = SC.GUARD


def abi():
    from vidar_amd._lib import lib, ptr, stream_of, BAD_ARG
    return lib(), ptr, stream_of, BAD_ARG


def window(shape):
    n = math.prod(shape)
    buf = torch.full((G + n + G,), math.nan, device="cuda")
    return buf, buf[G:G + n]


def guards_intact(buf, n):
    return bool(torch.isnan(buf[:G]).all()) and bool(torch.isnan(buf[G + n:]).all())


# ---- 1. the plan -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", SC.PLAN_Q)
def test_plan_tables_are_exactly_the_fp64_tables(Q):
    L, ptr, stream_of, _ = abi()
    c = SC.plan_case(Q)
    assert float((c["cz"] - SC.Z_EPS).abs().min()) >= SC.MARGIN          # the margins, on the fp64 values: no anchor is
    assert float(SC.border_distance(c["u"], c["v"]).min()) >= SC.MARGIN  # borderline, none is left out below
    Fr, B, N, D = SC.NF, SC.NB, SC.NCAM, SC.ND
    dev = "cuda"
    ref_3d, l2i = c["ref_3d"].cuda(), c["l2i"].cuda()
    ref_cam = torch.full((Fr, N, B, Q, D, 2), math.nan, device=dev)
    mask = torch.full((Fr, N, B, Q, D), 7, device=dev, dtype=torch.uint8)
    count = torch.full((Fr, B, Q), math.nan, device=dev)
    idx = torch.full((Fr, N, Q), -5, device=dev, dtype=torch.int64)
    valid = torch.full((Fr, N, Q), 7, device=dev, dtype=torch.uint8)
    lens = torch.full((Fr, N), -5, device=dev, dtype=torch.int32)
    slot_of = torch.full((Fr, N, Q), -5, device=dev, dtype=torch.int32)
    rng = (ctypes.c_float * 6)(*SC.PC_RANGE)
    rc = L.vidar_sca_plan_f32(ptr(ref_3d), ptr(l2i), ptr(ref_cam), ptr(mask), ptr(count), ptr(idx), ptr(valid),
                              ptr(lens), ptr(slot_of), rng, SC.IMG_H, SC.IMG_W, Fr, B, N, Q, D, stream_of(ref_3d))
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.equal(mask.cpu(), c["mask"].to(torch.uint8))
    assert torch.equal(count.cpu(), c["count"])
    assert torch.equal(lens.cpu(), c["lens"])
    assert torch.equal(valid.cpu(), c["valid"])
    assert torch.equal(idx.cpu(), c["idx"])                              # the lists ascending, then the slot numbers
    assert torch.equal(slot_of.cpu(), c["slot_of"])
    # the same, said as the contract says it
    idx_h, inv = idx.cpu(), slot_of.cpu().long()
    vis0 = c["mask"].any(-1)[:, :, 0]
    assert torch.equal(inv >= 0, vis0)
    for f in range(Fr):
        for n in range(N):
            seen = inv[f, n] >= 0
            k = int(seen.sum())
            assert torch.equal(idx_h[f, n][inv[f, n][seen]], torch.nonzero(seen).view(-1))
            assert torch.equal(idx_h[f, n, k:], torch.arange(k, Q))     # the filler: distinct and in range
    far = c["cz"] >= 1.0
    assert int(far.sum()) > 0
    torch.testing.assert_close(ref_cam.cpu().double()[far], torch.stack((c["u"], c["v"]), -1)[far], rtol=2e-4, atol=1e-5)


# ---- 2 - 4. the gathers ------------------------------------------------------------------------------------------------
_DEVICE = {}


def device_gathers(case):
    """rows and combine of the device on the NaN-planted and on the finite inputs of a case, on the CPU; run once"""
    if case in _DEVICE:
        return _DEVICE[case]
    L, ptr, stream_of, _ = abi()
    B, C, S, with_count = case
    t, d = SC.gather_tables(), SC.gather_inputs(B, C, S)
    idx, valid, slot_of = t["idx"].cuda(), t["valid"].cuda(), t["slot_of"].cuda()
    count = t["count"][:B].cuda().contiguous() if with_count else None
    out = {}
    for tag in ("", "_nan"):
        x = d["x" + tag].cuda()
        # combine's source ends in a NaN guard of its own: a slot >= S of the last camera would read it
        ybuf, y = window((B, SC.GN, S, C))
        y.copy_(d["y" + tag].reshape(-1))
        rbuf, rows = window((B, SC.GN, S, C))
        cbuf, comb = window((B, SC.GQ, C))
        st = stream_of(x)
        assert L.vidar_sca_rows_f32(ptr(x), ptr(idx), ptr(valid), ptr(count), ptr(rows), B, SC.GN, S, SC.GQ, SC.GQ, C, st) == 0
        assert L.vidar_sca_combine_f32(ptr(y), ptr(slot_of), ptr(count), ptr(comb), B, SC.GN, S, SC.GQ, C, st) == 0
        torch.cuda.synchronize()
        assert guards_intact(rbuf, rows.numel()) and guards_intact(cbuf, comb.numel())
        if S == 0:                              # no slots: rows has nothing to write; combine's sums are empty, so zeros
            assert bool(torch.isnan(rbuf).all()) and float(comb.abs().max()) == 0.0
        out["rows" + tag] = rows.cpu().view(B, SC.GN, S, C)
        out["combine" + tag] = comb.cpu().view(B, SC.GQ, C)
    _DEVICE[case] = out
    return out


def host_tables(case):
    t = SC.gather_tables()
    return t["idx"], t["valid"], t["slot_of"], (t["count"][:case[0]] if case[3] else None)


@pytest.mark.parametrize("case", SC.GATHER_CASES, ids=SC.gather_id)
def test_rows_bits(case):
    B, C, S, _ = case
    idx, valid, _, count = host_tables(case)
    d, got = SC.gather_inputs(B, C, S), device_gathers(case)
    want = SC.rows32(d["x_nan"], idx, valid, count, S)
    assert bool(torch.isfinite(want).all())
    assert torch.equal(got["rows_nan"], want) and torch.equal(got["rows"], want)
    pad = ~valid[:, :S].bool()
    if S:
        assert float(got["rows_nan"][:, pad].abs().max()) == 0.0 and int(pad.sum()) > 0


@pytest.mark.parametrize("case", SC.GATHER_CASES, ids=SC.gather_id)
def test_combine_bits_and_fp64_bound(case):
    B, C, S, _ = case
    _, _, slot_of, count = host_tables(case)
    d, got = SC.gather_inputs(B, C, S), device_gathers(case)
    want = SC.combine32(d["y"], slot_of, count, S)
    assert torch.equal(got["combine_nan"], want) and torch.equal(got["combine"], want)
    ref = SC.combine32(d["y"].double(), slot_of, count.double() if count is not None else None, S)
    assert bool(((got["combine"].double() - ref).abs() <= SC.combine_bound(d["y"], slot_of, count, S)).all())
    unseen = (slot_of < 0) | (slot_of >= S)
    assert float(got["combine"][:, unseen.all(0)].abs().max()) == 0.0 and int(unseen.all(0).sum()) >= 5


@pytest.mark.parametrize("case", SC.GATHER_CASES, ids=SC.gather_id)
def test_rows_and_combine_are_adjoint(case):
    B, C, S, _ = case
    idx, valid, _, count = host_tables(case)
    d, got = SC.gather_inputs(B, C, S), device_gathers(case)
    lhs = float((got["rows"].double() * d["y"].double()).sum())
    rhs = float((d["x"].double() * got["combine"].double()).sum())
    # rows rounds once (the division), combine N times; both against sum |x| |y| / count over the connected pairs
    tol = (1 + SC.GN) * SC.EPS * SC.adjoint_terms(d["x"], d["y"], idx, valid, count, S)
    print(f"<rows x, y> = {lhs:.9e}   <x, combine y> = {rhs:.9e}   difference {abs(lhs - rhs):.2e}   bound {tol:.2e}")
    assert abs(lhs - rhs) <= tol
    assert (S == 0) == (lhs == 0.0 and rhs == 0.0)


# ---- 5. empty problems and bad arguments -------------------------------------------------------------------------------
def test_empty_and_bad_arguments_write_nothing():
    L, ptr, stream_of, BAD_ARG = abi()
    t = SC.gather_tables()
    B, C, S, Q, N = 2, 8, 5, SC.GQ, SC.GN
    idx, valid, slot_of, count = t["idx"].cuda(), t["valid"].cuda(), t["slot_of"].cuda(), t["count"].cuda()
    x, y = torch.randn(B, Q, C, device="cuda"), torch.randn(B, N, S, C, device="cuda")
    rbuf, rows = window((B, N, S, C))
    cbuf, comb = window((B, Q, C))
    st = stream_of(x)

    def call_rows(B=B, N=N, S=S, stride=Q, Q=Q, C=C):
        return L.vidar_sca_rows_f32(ptr(x), ptr(idx), ptr(valid), ptr(count), ptr(rows), B, N, S, stride, Q, C, st)

    def call_combine(B=B, N=N, S=S, Q=Q, C=C):
        return L.vidar_sca_combine_f32(ptr(y), ptr(slot_of), ptr(count), ptr(comb), B, N, S, Q, C, st)
    assert call_rows(B=0) == 0 and call_rows(S=0) == 0 and call_combine(B=0) == 0
    for bad in (dict(C=6), dict(C=0), dict(N=0), dict(N=-1), dict(Q=0), dict(Q=-3), dict(B=-1), dict(S=-1)):
        assert call_rows(**bad) == BAD_ARG, bad
        assert call_combine(**bad) == BAD_ARG, bad
    assert call_rows(stride=S - 1) == BAD_ARG
    torch.cuda.synchronize()
    assert bool(torch.isnan(rbuf).all()) and bool(torch.isnan(cbuf).all())
