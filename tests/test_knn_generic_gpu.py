"""GPU: the generic (D, K) nearest-neighbour kernels (csrc/knn_generic.hip) against the reference's OWN knn_cpu.cpp
build (oracle/_ref): indices and distances bit for bit for every D, every K bucket edge and every split of p2, with ties,
ragged lengths and empty inputs; the backward's grad_p1 bit for bit and grad_p2 inside the fp32 any-order summation
bound; the routing of the wrapper (kernel range, the torch program outside it, the A/B switch, the deterministic mode)."""
import ctypes

import numpy as np
import pytest
import torch

from test_knn_generic_cpu import _clouds

pytestmark = pytest.mark.gpu

DS = [1, 2, 3, 5, 8]
KS = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32]
N, P1, P2 = 2, 301, 157
CHUNKS = [0, 1, 3, 157]


def dev(*ts):
    return tuple(t.cuda() for t in ts)


def ragged(l1, l2, case):
    """one full cloud and one shorter than most K; `empty`: no valid point in cloud 1, no valid row in batch 0"""
    l1, l2 = l1.clone(), l2.clone()
    l2[0] = P2
    l2[1] = 3
    if case == "empty":
        l2[1] = 0
        l1[0] = 0
    return l1, l2


@pytest.mark.parametrize("ties", [False, True], ids=["gaussian", "lattice"])
@pytest.mark.parametrize("D", DS)
def test_forward_equals_the_reference_build_for_every_split(D, ties, ref_modules):
    from vidar_amd.third_lib.chamferdist import _C
    ref = ref_modules("ref_chamferdist_C")
    a, b, l1, l2 = _clouds(31 * D + int(ties), N, P1, P2, D, ties)
    ga, gb = dev(a, b)
    for K in KS:
        if (D, K) == (3, 1):
            continue                                             # the K = 1, D = 3 kernel: tests/test_chamfer_gpu.py
        for case in ("short", "empty"):
            m1, m2 = ragged(l1, l2, case)
            ri, rd = ref.knn_points_idx(a, b, m1, m2, K, -1)
            g1, g2 = dev(m1, m2)
            outs = [_C.knn_points_idx(ga, gb, g1, g2, K, -1, chunks=c) for c in CHUNKS]
            for c, (oi, od) in zip(CHUNKS, outs):
                assert oi.dtype == torch.int64 and od.dtype == torch.float32 and oi.shape == od.shape == (N, P1, K)
                assert torch.equal(oi.cpu(), ri), (D, K, case, c)
                assert torch.equal(od.cpu(), rd), (D, K, case, c)
                assert torch.equal(oi, outs[0][0]) and torch.equal(od, outs[0][1]), (D, K, case, c)


def query(n, p1, p2, d, k, chunks):
    from vidar_amd._lib import lib
    nbytes, used = ctypes.c_int64(0), ctypes.c_int64(0)
    rc = lib().vidar_knn_workspace_bytes(n, p1, p2, d, k, chunks, ctypes.addressof(nbytes), ctypes.addressof(used))
    return rc, nbytes.value, used.value


def test_a_small_p1_splits_a_large_p2(ref_modules):
    from vidar_amd.third_lib.chamferdist import _C
    ref = ref_modules("ref_chamferdist_C")
    a, b, l1, l2 = _clouds(11, 1, 5, 5000, 3, False)
    l1[0] = 5; l2[0] = 4321
    rc, nbytes, used = query(1, 5, 5000, 3, 4, 0)
    assert rc == 0 and used > 1 and nbytes == 8 * 5 * used * 4
    oi, od = _C.knn_points_idx(*dev(a, b, l1, l2), 4, -1)
    ri, rd = ref.knn_points_idx(a, b, l1, l2, 4, -1)
    assert torch.equal(oi.cpu(), ri) and torch.equal(od.cpu(), rd)


def test_ties_across_a_chunk_boundary():
    from vidar_amd.third_lib.chamferdist import _C
    a, _, _, _ = _clouds(5, 1, 70, 64, 3, False)
    b = torch.full((1, 64, 3), 0.25)
    full = lambda n: torch.tensor([n])
    oi, od = _C.knn_points_idx(*dev(a, b, full(70), full(64)), 8, -1, chunks=4)
    assert torch.equal(oi.cpu(), torch.arange(8).expand(1, 70, 8))
    assert torch.equal(od[..., :1].expand(-1, -1, 8), od)


def test_short_and_empty_inputs_give_zeros():
    from vidar_amd.third_lib.chamferdist import _C
    a, b, l1, l2 = _clouds(2, 2, 40, 3, 3, False)
    l1[:] = 40; l2[:] = 3
    oi, od = _C.knn_points_idx(*dev(a, b, l1, l2), 8, -1)        # K > P2
    assert oi.shape == (2, 40, 8) and not oi[..., 3:].any() and not od[..., 3:].any()
    assert torch.equal(oi[..., :3].sort(-1).values.cpu(), torch.arange(3).expand(2, 40, 3)) and bool((od[..., :3] > 0).all())
    oi, od = _C.knn_points_idx(*dev(a, b, l1, torch.zeros(2, dtype=torch.int64)), 8, -1)   # lengths2 = 0
    assert oi.shape == (2, 40, 8) and not oi.any() and not od.any()
    g1, g2 = _C.knn_points_backward(*dev(a, b, l1, torch.zeros(2, dtype=torch.int64)), oi, torch.ones_like(od))
    assert g1.shape == (2, 40, 3) and g2.shape == (2, 3, 3) and not g1.any() and not g2.any()
    e = torch.zeros(2, 0, 3)
    oi, od = _C.knn_points_idx(*dev(e, b, torch.zeros(2, dtype=torch.int64), l2), 8, -1)   # P1 = 0
    assert oi.shape == (2, 0, 8) and od.shape == (2, 0, 8) and oi.dtype == torch.int64
    g1, g2 = _C.knn_points_backward(*dev(e, b, torch.zeros(2, dtype=torch.int64), l2), oi, od)
    assert g1.shape == (2, 0, 3) and g2.shape == (2, 3, 3) and not g2.any()
    oi, od = _C.knn_points_idx(*dev(a, e, l1, torch.zeros(2, dtype=torch.int64)), 8, -1)   # P2 = 0
    assert oi.shape == (2, 40, 8) and not oi.any() and not od.any()
    torch.cuda.synchronize()


def test_the_call_overwrites_every_output_element(ref_modules):
    """idx = -7 and dist2 = NaN before the call, through the raw ABI: rows past lengths1 and slots past lengths2 are
    the call's to zero"""
    from vidar_amd._lib import lib, ptr, stream_of
    ref = ref_modules("ref_chamferdist_C")
    K, D = 9, 5
    a, b, l1, l2 = _clouds(77, N, P1, P2, D, True)
    l1, l2 = ragged(l1, l2, "short")
    ri, rd = ref.knn_points_idx(a, b, l1, l2, K, -1)
    ga, gb, g1, g2 = dev(a, b, l1, l2)
    idx = torch.full((N, P1, K), -7, dtype=torch.int64, device="cuda")
    dist = torch.full((N, P1, K), float("nan"), device="cuda")
    rc, nbytes, used = query(N, P1, P2, D, K, 3)
    assert rc == 0 and used == 3
    ws = torch.full((nbytes // 8,), 0x0badbadbadbadbad, dtype=torch.int64, device="cuda")
    rc = lib().vidar_knn_fwd_f32(ptr(ga), ptr(gb), ptr(g1), ptr(g2), ptr(idx), ptr(dist), ptr(ws), nbytes,
                                 N, P1, P2, D, K, 3, stream_of(ga))
    assert rc == 0
    assert torch.equal(idx.cpu(), ri) and torch.equal(dist.cpu(), rd)
    # a workspace one byte short is refused, not overrun
    assert lib().vidar_knn_fwd_f32(ptr(ga), ptr(gb), ptr(g1), ptr(g2), ptr(idx), ptr(dist), ptr(ws), nbytes - 1,
                                   N, P1, P2, D, K, 3, stream_of(ga)) == -22


def p2_sums(a, b, l1, l2, idx, g):
    """per element of grad_p2: the fp64 sum S of the fp32 contributions -c, sum |c| and their count, from `idx`"""
    n_, p1_, d_ = a.shape
    K = idx.shape[2]
    a, b, idx, g = a.numpy(), b.numpy(), idx.numpy(), g.numpy()
    S = np.zeros(b.shape, np.float64); A = np.zeros(b.shape, np.float64); C = np.zeros(b.shape, np.int64)
    for n in range(n_):
        kk = min(K, int(l2[n]))
        rows = int(l1[n])
        j = idx[n, :rows, :kk]                                                   # [rows, kk]
        g2 = np.float32(2.0) * g[n, :rows, :kk]                                  # fp32, as the kernel
        c = g2[..., None] * (a[n, :rows, None, :] - b[n][j])                     # [rows, kk, D] fp32, each op rounded
        assert c.dtype == np.float32
        jj = np.broadcast_to(j[..., None], c.shape)
        dd = np.broadcast_to(np.arange(d_), c.shape)
        np.add.at(S[n], (jj, dd), -c.astype(np.float64))
        np.add.at(A[n], (jj, dd), np.abs(c).astype(np.float64))
        np.add.at(C[n], (jj, dd), 1)
    return S, A, C


@pytest.mark.parametrize("D,K", [(3, 2), (3, 9), (8, 4), (1, 32), (2, 1)])
def test_backward(D, K, ref_modules):
    """grad_p1: a per-row sum in the order k = 0, 1, .., bit-equal to the reference build.  grad_p2: fp32 atomics in any
    order; against the fp64 sum S of the same fp32 contributions, |out - S| <= n_a * 2^-23 * sum |c| (n_a contributions
    at that address): the any-order fp32 summation bound (n - 1) * 2^-24 * sum |c| with a factor 2 of slack"""
    from vidar_amd.third_lib.chamferdist import _C
    ref = ref_modules("ref_chamferdist_C")
    a, b, l1, l2 = _clouds(13 * D + K, N, P1, P2, D, True)       # a lattice: many rows share their neighbours
    l1, l2 = ragged(l1, l2, "short")
    ri, _ = ref.knn_points_idx(a, b, l1, l2, K, -1)
    g = torch.from_numpy(np.random.default_rng(D + K).standard_normal((N, P1, K)).astype(np.float32))
    r1, _ = ref.knn_points_backward(a, b, l1, l2, ri, g)
    o1, o2 = _C.knn_points_backward(*dev(a, b, l1, l2, ri, g))
    assert o1.shape == a.shape and o2.shape == b.shape
    assert torch.equal(o1.cpu(), r1)
    S, A, C = p2_sums(a, b, l1, l2, ri, g)
    err = np.abs(o2.cpu().numpy().astype(np.float64) - S)
    bound = C * 2.0 ** -23 * A
    print(f"D={D} K={K}: max contributions per address {C.max()}, max |out - S| {err.max():.3e}, "
          f"max err / bound {np.max(err[C > 0] / np.maximum(bound[C > 0], 1e-300)):.3f}")
    assert C.max() > 1
    assert (err <= bound).all()


def test_autograd_through_knn_points():
    from vidar_amd.third_lib.chamferdist import _C, knn_points
    a, b, l1, l2 = _clouds(3, N, P1, P2, 3, False)
    l1, l2 = ragged(l1, l2, "short")
    ga, gb, g1, g2 = dev(a, b, l1, l2)
    ga.requires_grad_(); gb.requires_grad_()
    out = knn_points(ga, gb, g1, g2, K=5, return_nn=True)
    assert out.knn.shape == (N, P1, 5, 3)
    out.dists.sum().backward()
    oi, od = _C.knn_points_idx(ga.detach(), gb.detach(), g1, g2, 5, -1)
    assert torch.equal(out.idx, oi) and torch.equal(out.dists.detach(), od)
    w1, w2 = _C.knn_points_backward(ga.detach(), gb.detach(), g1, g2, oi, torch.ones_like(od))
    assert torch.equal(ga.grad, w1)
    torch.testing.assert_close(gb.grad, w2, rtol=1e-5, atol=1e-5)                # two launches of fp32 atomics


@pytest.mark.parametrize("D,K", [(9, 2), (3, 40)])
def test_outside_the_kernel_range_the_torch_program_answers(D, K, ref_modules, monkeypatch):
    from vidar_amd.third_lib.chamferdist import _C
    ref = ref_modules("ref_chamferdist_C")
    assert query(N, P1, P2, D, K, 0)[:2] == (-22, -1)
    calls = []
    program = _C._generic_knn_idx
    monkeypatch.setattr(_C, "_generic_knn_idx", lambda *x: calls.append(1) or program(*x))
    a, b, l1, l2 = _clouds(D + K, N, P1, P2, D, True)
    oi, od = _C.knn_points_idx(*dev(a, b, l1, l2), K, -1)
    ri, rd = ref.knn_points_idx(a, b, l1, l2, K, -1)
    assert calls and torch.equal(oi.cpu(), ri) and torch.equal(od.cpu(), rd)


def test_the_switch_to_the_torch_program(monkeypatch):
    from vidar_amd.third_lib.chamferdist import _C
    a, b, l1, l2 = _clouds(21, N, P1, P2, 5, True)
    args = dev(a, b, l1, l2)
    ki, kd = _C.knn_points_idx(*args, 6, -1)
    g = torch.ones_like(kd)
    k1, k2 = _C.knn_points_backward(*args, ki, g)
    calls = []
    program = _C._generic_knn_idx
    monkeypatch.setattr(_C, "_generic_knn_idx", lambda *x: calls.append(1) or program(*x))
    assert not calls
    monkeypatch.setenv("VIDAR_KNN_GENERIC", "torch")
    ti, td = _C.knn_points_idx(*args, 6, -1)
    assert calls and torch.equal(ti, ki) and torch.equal(td, kd)
    t1, t2 = _C.knn_points_backward(*args, ki, g)
    torch.testing.assert_close(t1, k1, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(t2, k2, rtol=1e-5, atol=1e-4)


def test_the_deterministic_mode_still_refuses_the_generic_backward():
    from vidar_amd import deterministic
    from vidar_amd.third_lib.chamferdist import _C
    a, b, l1, l2 = _clouds(1, 1, 20, 10, 3, False)
    args = dev(a, b, l1, l2)
    oi, od = _C.knn_points_idx(*args, 2, -1)
    with deterministic.use(True):
        with pytest.raises(RuntimeError, match="knn generic backward"):
            _C.knn_points_backward(*args, oi, torch.ones_like(od))
    g1, g2 = _C.knn_points_backward(*args, oi, torch.ones_like(od))
    assert g1.shape == a.shape and g2.shape == b.shape
