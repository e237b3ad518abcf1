"""CPU: the restatements of tests/norm_fuse_cases.py pinned on their own, so that tests/test_norm_fuse_direct_gpu.py
compares the kernels of csrc/norm_fuse.hip with something that is itself held: the fp64 LayerNorm tail to
F.layer_norm and its autograd in fp64, the bounds to an fp32 evaluation in the kernel's own order on every family and
eps (a bound a correct fp32 evaluation could miss would be no bound), the keep rule to its rate and its independence
inside a float4, and the integer-exactness conditions to every listed shape."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import norm_fuse_cases as NC

CPU_ROWS = 401
FAMILY_EPS = [(f, p, eps) for f, p in NC.LN_GRID for eps in NC.EPSES]
FAMILY_EPS_IDS = [f"{f}-p{p}-eps{eps}" for f, p, eps in FAMILY_EPS]


def sliced(family, p, rows=CPU_ROWS):
    c = NC.ln_case(family, away=p > 0)
    return {k: (v[:rows] if v.dim() == 2 else v) for k, v in c.items()}


@pytest.mark.parametrize("family,p,eps", FAMILY_EPS, ids=FAMILY_EPS_IDS)
def test_fp64_forward_and_backward_are_torchs_layer_norm(family, p, eps):
    c = sliced(family, p, 65)
    f = NC.ln_forward(c["x"], c["r"], c["gamma"], c["beta"], p, eps, NC.SEED)
    kp, sc = f["keep"], NC.scale64(p)
    x, r = c["x"].double().requires_grad_(), c["r"].double().requires_grad_()
    gamma, beta = c["gamma"].double().requires_grad_(), c["beta"].double().requires_grad_()
    y = F.layer_norm(x * kp * sc + r, (NC.C,), gamma, beta, NC.eps32(eps))
    torch.testing.assert_close(f["y"], y.detach(), rtol=1e-9, atol=1e-9 * float(c["beta"].abs().max()))
    gx, gr, gg, gb = torch.autograd.grad(y, [x, r, gamma, beta], c["gy"].double())
    b = NC.ln_backward(c["gy"], f["S"], f["mean"], f["rstd"], c["gamma"], kp, p)
    dgamma, _, dbeta = NC.affine_grads(b, c["gy"], 65)
    # absolute part: 1e-9 of the natural size of each gradient (a constant row has h = 0 up to fp64 noise times rstd)
    per_row = 1e-9 * float(f["rstd"].max()) * NC.GY_MAX * 2 * sc
    summed = 1e-9 * 65 * NC.GY_MAX * 20
    for mine, ref, atol in ((b["gres"], gr, per_row), (b["gx"], gx, per_row), (dgamma, gg, summed), (dbeta, gb, summed)):
        torch.testing.assert_close(mine, ref, rtol=1e-7, atol=atol)
    assert bool((b["gx"][~kp] == 0).all())
    if p > 0:
        assert 0 < int(kp.sum()) < kp.numel()


@pytest.mark.parametrize("family,p,eps", FAMILY_EPS, ids=FAMILY_EPS_IDS)
def test_kernel_order_fp32_evaluation_is_inside_every_bound(family, p, eps):
    c = sliced(family, p)
    args = (c["x"], c["r"], c["gamma"], c["beta"], p, eps, NC.SEED)
    f, bnd, f32 = NC.ln_forward(*args), NC.ln_fwd_bound(*args), NC.ln_forward32(*args)
    for name, key in (("y", "y"), ("sum", "S"), ("mean", "mean"), ("rstd", "rstd")):
        ok, ratio = NC.worst(f32[key], f[key], bnd[name])
        print(f"margin fwd {name} {ratio:.3f}")
        assert ok, (name, ratio)
    if family == "const":
        assert NC.same_bits(f32["y"], c["beta"].expand(CPU_ROWS, NC.C).contiguous())
        want = np.float32(1) / np.sqrt(np.float32(eps))
        assert bool((f32["rstd"] == float(want)).all())
    s, mean, rstd = NC.ln_given(f)
    b = NC.ln_backward(c["gy"], s, mean, rstd, c["gamma"], f["keep"], p)
    b32 = NC.ln_backward32(c["gy"], s, mean, rstd, c["gamma"], p, NC.SEED)
    dgamma, dgamma_bound, dbeta = NC.affine_grads(b, c["gy"], CPU_ROWS)
    for name, got, ref, bd in (("gres", b32["gres"], b["gres"], b["bound_res"]), ("gx", b32["gx"], b["gx"], b["bound_x"]),
                               ("dgamma", b32["dgamma"], dgamma, dgamma_bound)):
        ok, ratio = NC.worst(got, ref, bd)
        print(f"margin bwd {name} {ratio:.3f}")
        assert ok, (name, ratio)
    assert torch.equal(b32["dbeta"].double(), dbeta)
    assert bool((b32["gx"][~f["keep"]] == 0).all())


def test_a_sequential_row_sum_is_outside_the_bound():
    """the constants count the kernel's tree: the bound is tight enough to tell a 256-term chain from it"""
    c = sliced("spike", 0.0, 40)
    args = (c["x"], c["r"], c["gamma"], c["beta"], 0.0, 1e-5, NC.SEED)
    f, bnd = NC.ln_forward(*args), NC.ln_fwd_bound(*args)
    s = (c["x"] + c["r"]).numpy()
    mean = np.add.accumulate(s, axis=1, dtype=np.float32)[:, -1] * np.float32(1 / 256)
    d = s - mean[:, None]
    var = np.add.accumulate(d * d, axis=1, dtype=np.float32)[:, -1] * np.float32(1 / 256)
    y = d * (np.float32(1) / np.sqrt(var + np.float32(1e-5)))[:, None] * c["gamma"].numpy() + c["beta"].numpy()
    ok, ratio = NC.worst(torch.from_numpy(y), f["y"], bnd["y"])
    print(f"sequential / bound {ratio:.2f}")
    assert not ok and ratio > 1.5        # the tree's own worst ratio on this family is 0.64


@pytest.mark.parametrize("wrong", ["one_pass", "divisor_255", "eps_outside"])
def test_forward_bound_sees_a_wrong_variance(wrong):
    """what the GPU test is for: three classic mistakes leave the bound on the family built for them"""
    family, eps = {"one_pass": ("offset", 1e-5), "divisor_255": ("normal", 1e-5), "eps_outside": ("tiny", 1e-5)}[wrong]
    c = sliced(family, 0.0, 17)
    args = (c["x"], c["r"], c["gamma"], c["beta"], 0.0, eps, NC.SEED)
    f, bnd = NC.ln_forward(*args), NC.ln_fwd_bound(*args)
    S = (c["x"] + c["r"]).double()
    mean = S.mean(1, keepdim=True)
    var = ((S - mean) ** 2).mean(1, keepdim=True)
    if wrong == "one_pass":
        S32 = c["x"] + c["r"]
        var = ((S32 * S32).mean(1, keepdim=True) - S32.mean(1, keepdim=True) ** 2).double()
        rstd = 1 / torch.sqrt(var.clamp_min(0) + eps)
    elif wrong == "divisor_255":
        rstd = 1 / torch.sqrt(var * 256 / 255 + eps)
    else:
        rstd = 1 / (torch.sqrt(var) + eps)
    y = (S - mean) * rstd * c["gamma"].double() + c["beta"].double()
    assert not NC.worst(y, f["y"], bnd["y"])[0]


def test_integer_exactness_conditions_hold_for_every_listed_shape():
    assert max(NC.ROWS) * NC.GY_MAX <= 2 ** 24
    gy = NC.ln_case("normal")["gy"]
    assert bool((gy == gy.round()).all()) and float(gy.abs().max()) == NC.GY_MAX
    # four row counts per width; rstep - 1 == 1 at 2048 columns and 0 at 4096 (rows = 0: zeros), where rstep == 1 too
    assert len(NC.COLSUM_SMALL) == 4 * len(NC.COLSUM_COLS) - 2 and (0, 4096) in NC.COLSUM_SMALL
    for rows, cols in NC.COLSUM_SMALL + NC.COLSUM_CAPPED:
        assert rows * NC.COLSUM_MAX <= 2 ** 24 and rows * cols * 4 <= 18 * 2 ** 20
    for rows, cols in NC.COLSUM_CAPPED:
        per_pass = 4 * NC.rstep(cols)
        assert -(-rows // per_pass) > 256 and rows == 256 * per_pass + 5
    for rows, cols in NC.COLSUM_REAL:
        assert rows <= 300
    for rows, cols in [(64, 16), (33, 256), (5, 4096)]:
        x = NC.colsum_int(rows, cols)
        assert bool((x == x.round()).all()) and float(x.abs().max()) <= NC.COLSUM_MAX
        total = x.double().sum(0)
        assert bool((x.abs().sum(1) > 0).all())                       # no row could be dropped unseen
        assert not torch.equal(total[:-1], total[1:]) and not torch.equal(x[:-1], x[1:])
        assert not torch.equal(total, x[:-1].double().sum(0))          # a dropped row, a doubled row
        assert not torch.equal(total, total + x[0].double())
    assert [NC.parts(r) for r in (129, 257, 401, 1025, 2049, 4113)] == [9, 17, 26, 65, 129, 258]
    assert NC.RELU_SIZES[-2] // 4 > 256 * 16384 and NC.RELU_SIZES[-1] // 4 // 256 + 1 == 16384


@pytest.mark.parametrize("seed", [NC.SEED, 12345])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_rate_and_independence_inside_a_float4(p, seed):
    n = 2 ** 20
    kp = NC.keep(seed, n, p)
    q = 1.0 - float(np.float32(p))
    assert abs(int(kp.sum()) - n * q) <= 5 * math.sqrt(n * q * (1 - q))
    groups = kp.reshape(-1, 4)
    mixed = int((groups.any(1) & ~groups.all(1)).sum())                # a float4 whose four positions do not agree
    m = 1.0 - q ** 4 - (1 - q) ** 4
    assert abs(mixed - len(groups) * m) <= 5 * math.sqrt(len(groups) * m * (1 - m))
    for a in range(4):
        for b in range(a + 1, 4):                                      # no two positions share one decision
            agree = float((groups[:, a] == groups[:, b]).mean())
            assert abs(agree - (q * q + (1 - q) ** 2)) < 0.01
    assert np.array_equal(NC.keep(seed, 64, p, start=100), kp[100:164])
    assert not np.array_equal(NC.keep(seed + 2, n, p), kp)


def test_p_zero_keeps_everything_and_the_scale_is_fp32():
    assert NC.keep(NC.SEED, 4096, 0.0).all()
    assert float(NC.scale32(0.0)) == 1.0 and float(NC.scale32(0.5)) == 2.0
    assert float(NC.scale32(0.1)) == float(np.float32(1) / np.float32(0.9))
    assert NC.keep(5, 8, 0.5, start=2 ** 32).shape == (8,)             # the 64-bit term is stated (and not tested)


def test_relu_drop_restatement_and_its_planted_values():
    p, seed = 0.5, NC.SEED
    x, gy, kept, dropped = NC.relu_planted(seed, p)
    assert len(kept) == len(dropped) == len(NC.PLANTED)
    y = NC.relu_drop(x, seed, p)
    zero, nzero, den, inf, ninf, nan = range(6)
    for pos in (kept, dropped):
        assert float(y[pos[zero]]) == 0 and float(y[pos[nzero]]) == 0 and not math.copysign(1, float(y[pos[nzero]])) < 0
        assert float(y[pos[ninf]]) == 0 and float(y[pos[nan]]) == 0     # NaN under the ReLU is 0
    assert float(y[kept[den]]) == float(np.float32(NC.DENORMAL) * np.float32(2)) > 0 and float(y[dropped[den]]) == 0
    assert float(y[kept[inf]]) == math.inf and math.isnan(float(y[dropped[inf]]))
    gx = NC.relu_drop_bwd(gy, y, p)
    assert float(gx[dropped[inf]]) == 0 and float(gx[dropped[den]]) == 0
    assert float(gx[kept[den]]) == 2 * float(gy[kept[den]])
    clean = NC.relu_case(1024)["x"]
    ref = F.relu(clean) * torch.from_numpy(NC.keep(seed, 1024, p)) * 2.0
    assert NC.same_bits(NC.relu_drop(clean, seed, p), ref)
    assert NC.same_bits(NC.relu_drop(clean, seed, 0.0), F.relu(clean))
