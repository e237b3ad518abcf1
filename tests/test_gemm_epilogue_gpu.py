"""The pipelined epilogue of csrc/gemm_mfma.hip (last_step_piped: a full fp32 tile runs its last k-step accumulator-major
with the scale / shift / residual / ReLU and the stores between the MFMAs) against fp64 products and, bit for bit,
against the wave-specialised kernels, which keep the plain epilogue().

All calls go through G.gemm_raw with the convolution's operand pair (A K-major, B MN-major) plus K-major / K-major.
Tolerances are those of tests/test_gemm_gpu.py: normwise 2e-6 (fp32: K <= 256 products of |x| <= 1) and 6e-5 (bf16x3)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from vidar_amd import gemm as G  # noqa: E402
from vidar_amd._lib import lib  # noqa: E402

DEV = "cuda"
TOL = {G.F32: 2e-6, G.BF16X3: 6e-5}
KINDS = ("full", "scale", "shift", "residual")


def rnd(*shape, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1).to(DEV)


def normwise(c, ref):
    return float((c.double() - ref).abs().max() / ref.abs().max())


def operands(M, N, K, b_layout, batch=1):
    a = rnd(M, K, seed=M + K)                                             # shared by the batch (a weight matrix)
    b = rnd(batch, K, N, seed=N + K) if b_layout == 1 else rnd(batch, N, K, seed=N + K)
    acc = torch.einsum("mk,bkn->bmn", a.double(), (b if b_layout == 1 else b.transpose(1, 2)).double())
    return a, b, acc


def call(a, b, b_layout, M, N, K, batch, vec_axis, kind, precision, vecs):
    """one product into a window of a NaN-filled buffer -> (window, whole buffer, fp64 reference)"""
    scale, shift, res_big = vecs
    use_scale, use_shift, use_res = kind in ("full", "scale"), kind in ("full", "shift"), kind in ("full", "residual")
    relu = kind == "full"
    ldc, ldr = N + 5, N + 9                                                # ldc != ldr != N
    big = torch.full((batch, M + 3, ldc), float("nan"), device=DEV)
    C = big[:, :M, :N]
    res = res_big[:, :M, :N]
    G.gemm_raw(a, a.stride(0), G.K_MAJOR, b, b.stride(1), b_layout, C, ldc, M, N, K, batch=batch, sA=0, sB=b.stride(0),
               sC=big.stride(0), scale=scale[vec_axis] if use_scale else None, shift=shift[vec_axis] if use_shift else None,
               vec_axis=vec_axis, residual=res if use_res else None, ldr=ldr if use_res else 0,
               sR=res_big.stride(0) if use_res else 0, relu=relu, precision=precision)
    return C, big


def reference(acc, vec_axis, kind, vecs):
    scale, shift, res_big = vecs
    M, N = acc.shape[1:]
    bc = (lambda v: v.double()[None, None, :]) if vec_axis == 0 else (lambda v: v.double()[None, :, None])
    y = acc
    if kind in ("full", "scale"):
        y = y * bc(scale[vec_axis])
    if kind in ("full", "shift"):
        y = y + bc(shift[vec_axis])
    if kind in ("full", "residual"):
        y = y + res_big[:, :M, :N].double()
    return torch.relu(y) if kind == "full" else y


def make_vecs(M, N, batch):
    """(scale by axis, shift by axis, the residual as a window of a NaN-filled buffer with its own leading dimension)"""
    scale = {0: rnd(N, seed=5) + 1.5, 1: rnd(M, seed=6) + 1.5}
    shift = {0: rnd(N, seed=7), 1: rnd(M, seed=8)}
    res_big = torch.full((batch, M + 2, N + 9), float("nan"), device=DEV)
    res_big[:, :M, :N] = rnd(batch, M, N, seed=9)
    return scale, shift, res_big


def with_variant(variant, fn):
    prev = lib().vidar_gemm_set_variant(variant)
    try:
        return fn()
    finally:
        lib().vidar_gemm_set_variant(prev)


@pytest.mark.parametrize("K", [32, 33, 45, 64, 256])
@pytest.mark.parametrize("M,N", [(128, 128), (130, 70), (257, 129), (64, 1)])
def test_edge_shapes(M, N, K):
    """the single-k-step tile, the k tail, ragged M, cut column tiles, a residual that must not be read past its window:
    finite, nothing written outside the window, within tolerance, and bit-identical to variant 2"""
    vecs = make_vecs(M, N, 1)
    for b_layout in ((G.MN_MAJOR, G.K_MAJOR) if (M, N) == (130, 70) or (M, N, K) == (128, 128, 64) else (G.MN_MAJOR,)):
        a, b, acc = operands(M, N, K, b_layout)
        for precision in (G.F32, G.BF16X3):
            for vec_axis in (0, 1):
                for kind in KINDS:
                    run = lambda: call(a, b, b_layout, M, N, K, 1, vec_axis, kind, precision, vecs)
                    C, big = run()
                    what = (M, N, K, b_layout, precision, vec_axis, kind)
                    assert torch.isfinite(C).all(), what
                    assert torch.isnan(big[:, M:]).all() and torch.isnan(big[:, :, N:]).all(), ("wrote outside the window", what)
                    err = normwise(C, reference(acc, vec_axis, kind, vecs))
                    assert err <= TOL[precision], (err, what)
                    C2, _ = with_variant(2, run)
                    assert torch.equal(C, C2), ("variant 2 differs", what)


@pytest.mark.parametrize("K", [32, 64])
def test_persistent_walk(K):
    """every workgroup runs at least two tiles (grid = 3 workgroups per CU): the next tile's prefetch meets the pipelined
    epilogue, and the scale / shift table alternates between its two buffers"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    batch, M = 4, 256
    N = 128 * math.ceil(2 * 3 * cus / 8) + 70
    a, b, acc = operands(M, N, K, G.MN_MAJOR, batch)
    vecs = make_vecs(M, N, batch)
    for precision in (G.F32, G.BF16X3):
        run = lambda: call(a, b, G.MN_MAJOR, M, N, K, batch, 1, "full", precision, vecs)
        C, big = run()
        assert torch.isfinite(C).all()
        assert torch.isnan(big[:, M:]).all() and torch.isnan(big[:, :, N:]).all(), "wrote outside the window"
        err = normwise(C, reference(acc, 1, "full", vecs))
        assert err <= TOL[precision], err
        assert float((C == 0).float().mean()) > 0.2 and float(C.min()) >= 0.0          # the ReLU was applied
        C2, _ = with_variant(2, run)
        assert torch.equal(C, C2), "variant 2 differs"


@pytest.mark.parametrize("precision", [G.F32, G.BF16X3])
def test_unchanged_paths(precision):
    """a split-K weight gradient with the bias gradient riding along (slabs + a_rowsum) and a product without an
    epilogue, MN-major A and K-major A"""
    M, N, K = 4097, 130, 33
    g2, x2 = rnd(M, N, seed=7), rnd(M, K, seed=8)
    gw, gb = G.linear_grad_weight(g2, x2, precision, with_bias=True)
    assert normwise(gw, g2.double().t() @ x2.double()) <= (3e-6 if precision == G.F32 else 1e-4) * (M ** 0.5)
    assert float((gb.double() - g2.double().sum(0)).abs().max() / g2.double().sum(0).abs().max()) <= 2e-5
    w, x = rnd(256, 96, seed=9), rnd(2, 96, 1450, seed=10)
    y = G.conv_forward(w, x, precision=precision)                         # full and cut tiles, no epilogue
    assert normwise(y, torch.einsum("oc,bcp->bop", w.double(), x.double())) <= TOL[precision]
    assert torch.equal(y, with_variant(2, lambda: G.conv_forward(w, x, precision=precision)))
    gy = rnd(2, 256, 1450, seed=11)
    gx = G.conv_grad_input(w, gy, precision)
    assert normwise(gx, torch.einsum("oc,bop->bcp", w.double(), gy.double())) <= TOL[precision]
