"""CPU: the restatement of tests/affine_act_cases.py held to torch's own operators, so that the GPU test compares the
kernels of csrc/affine_act.hip with something that is itself pinned: forward() to F.batch_norm (eval) + residual +
F.relu in fp64, backward() to autograd's bits in fp32, stem64() to F.max_pool2d, and bound() / stem_bound() hold for
torch's fp32 evaluation of the same expression (a bound a correct fp32 evaluation could miss would be no bound)."""
import math

import pytest
import torch
import torch.nn.functional as F

import affine_act_cases as AC

SMALL = AC.TINY + [AC.ALIGN_SHAPE, (1, 2, 16387)]


def frozen_bn(C, seed):
    g = torch.Generator().manual_seed(seed)
    gamma = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5) * torch.where(torch.arange(C) % 2 == 0, -1.0, 1.0)
    beta, mean = torch.randn(C, generator=g, dtype=torch.float64), torch.randn(C, generator=g, dtype=torch.float64)
    var = torch.rand(C, generator=g, dtype=torch.float64) * 1.5 + 0.5
    return gamma, beta, mean, var


@pytest.mark.parametrize("shape", SMALL, ids=AC.shape_id)
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("res", [False, True])
def test_forward_is_eval_batch_norm_residual_relu(shape, relu, res):
    c = AC.case(*shape)
    gamma, beta, mean, var = frozen_bn(shape[1], 3)
    eps = 1e-5
    s = gamma / torch.sqrt(var + eps)
    b = beta - mean * s
    x, r = c["x"].double(), (c["r"].double() if res else None)
    want = F.batch_norm(x, mean, var, gamma, beta, False, 0.0, eps)
    if res:
        want = want + r
    if relu:
        want = F.relu(want)
    got = AC.forward(x, s, b, r, relu)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("shape", SMALL + [AC.PLANTED_SHAPE], ids=AC.shape_id)
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("res", [False, True])
def test_bound_holds_for_torchs_fp32_evaluation(shape, relu, res):
    c = AC.planted() if shape == AC.PLANTED_SHAPE else AC.case(*shape)
    x, s, b, r = c["x"], c["s"], c["b"], (c["r"] if res else None)
    assert bool((s > 0).any()) and bool((s < 0).any()) and float(s.abs().min()) >= 0.5
    y = x * s.view(1, -1, 1) + b.view(1, -1, 1)
    if res:
        y = y + r
    if relu:
        y = torch.where(y > 0, y, torch.zeros_like(y))
    assert y.dtype == torch.float32
    assert AC.within(y, AC.forward(x, s, b, r, relu), AC.bound(x, s, b, r))


@pytest.mark.parametrize("relu", [0, 1])
def test_planted_values_and_the_nan_rule(relu):
    c = AC.planted()
    ref = AC.forward(c["x"], c["s"], c["b"], None, relu)
    assert float(ref[0, 0, 0]) == 0.0                                    # 1 * 1 - 1
    assert float(ref[0, 0, 1]) == (0.0 if relu else -1.0)                # -0.0 * 1 - 1
    assert float(ref[0, 0, 3]) == math.inf and float(ref[0, 0, 4]) == (0.0 if relu else -math.inf)
    nan = ref[0, :, 5]
    assert bool((nan == 0).all()) if relu else bool(torch.isnan(nan).all())
    assert bool(torch.isfinite(ref[0, :, 6:]).all())
    bnd = AC.bound(c["x"], c["s"], c["b"], None)
    assert not bool(torch.isfinite(bnd[0, :, 3:6]).any()) and bool(torch.isfinite(bnd[0, :, :3]).all())
    wrong = ref.clone()
    wrong[0, 1, 5] = 1.0                                                 # `within` asks for the exact value there
    assert AC.within(ref, ref, bnd) and not AC.within(wrong, ref, bnd)


@pytest.mark.parametrize("shape", SMALL, ids=AC.shape_id)
@pytest.mark.parametrize("relu", [0, 1])
def test_backward_is_autograds_bits(shape, relu):
    c = AC.case(*shape)
    x, r = c["x"].clone().requires_grad_(), c["r"].clone().requires_grad_()
    s = c["s"].view(1, -1, 1)
    y = x * s + c["b"].view(1, -1, 1) + r
    if relu:
        y = F.relu(y)
    gx, gr = torch.autograd.grad(y, [x, r], c["gy"])
    y_in = y.detach() if relu else torch.full_like(y, math.nan)         # without ReLU the output is not looked at
    mine = AC.backward(c["gy"], y_in, c["s"], relu)
    assert AC.same_bits(mine[0], gx) and AC.same_bits(mine[1], gr)
    if relu:
        assert 0 < int((y == 0).sum()) < y.numel()


@pytest.mark.parametrize("shape", AC.STEM_SHAPES[:-1], ids=AC.shape_id)
def test_stem_is_max_pool_of_the_forward(shape):
    c = AC.stem_case(*shape)
    x, s, b = c["x"], c["s"], c["b"]
    N, C, H, W = shape
    ref = AC.stem64(x, s, b)
    assert ref.shape == (N, C, (H - 1) // 2 + 1, W // 2) and bool(torch.isfinite(ref).all())
    act = torch.nan_to_num(x.double() * s.double().view(1, -1, 1, 1) + b.double().view(1, -1, 1, 1), nan=0.0)
    torch.testing.assert_close(ref, F.max_pool2d(F.relu(act), 3, 2, 1), rtol=0, atol=0)
    y32 = AC.pool(AC.forward(x, s, b, None, True).float())              # a correct fp32 evaluation is inside the bound
    assert AC.within(y32, ref, AC.stem_bound(x, s, b))
    flat, out = x.view(N * C, H, W), ref.view(N * C, *ref.shape[2:])
    assert math.isnan(float(flat[0, 0, 0])) and bool((s < 0).any())
    if N * C >= 2:
        assert float(out[1].abs().max()) == 0.0                          # the all-negative plane: 0, not -inf
    if W >= 8:
        p, t = (N * C - 1 if N * C >= 3 else 0), W // 4 - 1
        a = torch.relu(flat[p].double() * s[p % C].double() + b[p % C].double()).nan_to_num(0.0)
        row, col = H // 2, 4 * t - 1
        assert float(a[row, col]) == float(a.max()) > 50.0
        assert float(out[p, row // 2, 2 * t]) == float(a.max())          # read through p[-1] by the thread of column t


def test_stem_bound_sees_a_wrong_halo():
    """dropping the left halo column from the pooling changes the planted plane by far more than the bound"""
    shape = (1, 2, 3, 8)
    c = AC.stem_case(*shape)
    x, s, b = c["x"], c["s"], c["b"]
    blind = x.clone()
    blind[0, 0, 1, 3] = 0.0
    assert not AC.within(AC.stem64(blind, s, b), AC.stem64(x, s, b), AC.stem_bound(x, s, b))
