"""GPU: the five entries of csrc/norm_fuse.hip through the C ABI against the restatements of tests/norm_fuse_cases.py
(pinned by tests/test_norm_fuse_cases_cpu.py; the bounds are derived there).

1. LN forward: y, sum_out, mean_out, rstd_out within the elementwise bound of the fp64 reference on every row family
   x eps x row count at p = 0, and with the restated mask at p in {0.1, 0.5}; constant rows give beta bit for bit and
   rstd = fl(1 / fl(sqrt(eps))); the kept set EQUALS the restated one (sum_out - residual == 0 exactly where dropped);
2. LN backward from given fp32 sum / mean / rstd (the rounded fp64 forward, not the kernel's): grad_x, grad_residual and
   dgamma within their bounds, dbeta equal to the integer sum, grad_x zero at the restated dropped set; in the default
   mode and in the deterministic one, where three calls give the same bits; grad_gamma / grad_beta start as NaN;
3. relu_drop forward and backward bit for bit at the sizes around one float4, one workgroup and the grid cap, in place
   too, and on planted 0 / -0 / denormal / +-inf / NaN at kept and at dropped positions;
4. colsum exact on integer-valued matrices at every width x the row counts around one pass, past the 256-workgroup cap,
   and within the any-order bound on real ones; `out` starts as NaN;
5. every output is a window of a NaN-filled buffer whose 64 floats on each side are still NaN afterwards -- also after a
   workspace of exactly vidar_drop_add_ln_bwd_workspace_bytes(rows);
6. empty problems write nothing (or the zeros the header promises); a NaN p, p outside [0, 1), C != 256, negative sizes,
   n % 4 != 0, a NULL operand and a float4 operand 4 bytes off a 16-byte boundary are VIDAR_ERR_BAD_ARG and write
   nothing -- the entries return on these before any launch, and the offset pointers stay inside their buffers;
7. the autograd Functions clone a contiguous view that starts one float into its storage: same bits as an aligned copy."""
import math

import numpy as np
import pytest
import torch

import norm_fuse_cases as NC

pytestmark = pytest.mark.gpu
G = NC.GUARD
C = NC.C


def abi():
    from vidar_amd._lib import lib, ptr, stream_of, BAD_ARG
    return lib(), ptr, stream_of, BAD_ARG


def window(n):
    """(buffer, window): `n` floats inside a NaN-filled buffer, G floats of guard on each side, 16-byte aligned"""
    buf = torch.full((G + n + G,), math.nan, device="cuda")
    win = buf[G:G + n]
    assert n == 0 or win.data_ptr() % 16 == 0
    return buf, win


def guards_intact(buf, win):
    return bool(torch.isnan(buf[:G]).all()) and bool(torch.isnan(buf[G + win.numel():]).all())


def dev(t):
    out = t.contiguous().cuda()
    assert out.data_ptr() % 16 == 0
    return out


class Margins(dict):
    def see(self, name, got, ref, bnd, where):
        ok, ratio = NC.worst(got, ref, bnd)
        self[name] = max(self.get(name, 0.0), ratio)
        assert ok, f"{name} at {where}: error / bound = {ratio:.3f}"

    def show(self, what):
        print(what, " ".join(f"margin:{k}={v:.3f}" for k, v in self.items()))


# ---- LayerNorm(dropout(x) + residual) ----------------------------------------------------------------------------------
LN_IDS = [f"{f}-p{p}" for f, p in NC.LN_GRID]


def ln_fwd(x, r, gamma, beta, rows, p, eps, seed):
    """device tensors in -> (y, sum, mean, rstd) on the CPU; asserts the return code and the guards"""
    L, ptr, stream_of, _ = abi()
    outs = [window(rows * C), window(rows * C), window(rows), window(rows)]
    rc = L.vidar_drop_add_ln_fwd_f32(ptr(x), ptr(r), ptr(gamma), ptr(beta), *(ptr(w) for _, w in outs), rows, C, p, eps,
                                     seed, stream_of(x))
    torch.cuda.synchronize()
    assert rc == 0, f"vidar_drop_add_ln_fwd_f32 returned {rc}"
    assert all(guards_intact(b, w) for b, w in outs)
    y, s, mean, rstd = (w.cpu() for _, w in outs)
    return y.view(rows, C), s.view(rows, C), mean, rstd


@pytest.mark.parametrize("eps", NC.EPSES)
@pytest.mark.parametrize("family,p", NC.LN_GRID, ids=LN_IDS)
def test_ln_forward_within_the_derived_bound(family, p, eps):
    c = NC.ln_case(family, away=p > 0)
    args = (c["x"], c["r"], c["gamma"], c["beta"], p, eps, NC.SEED)
    f, bnd = NC.ln_forward(*args), NC.ln_fwd_bound(*args)
    x, r, gamma, beta = (dev(c[k]) for k in ("x", "r", "gamma", "beta"))
    m = Margins()
    for rows in NC.ROWS:
        got = dict(zip(("y", "S", "mean", "rstd"), ln_fwd(x[:rows], r[:rows], gamma, beta, rows, p, eps, NC.SEED)))
        for name, key in (("y", "y"), ("sum", "S"), ("mean", "mean"), ("rstd", "rstd")):
            m.see(name, got[key], f[key][:rows], bnd[name][:rows], f"rows={rows}")
        if family == "const":                    # 256 equal values sum exactly: d = 0
            assert NC.same_bits(got["y"], c["beta"].expand(rows, C).contiguous())
            assert bool((got["rstd"] == float(np.float32(1) / np.sqrt(np.float32(eps)))).all())
        if p > 0:                                # the kept set is the restated one
            dropped = ~f["keep"][:rows]
            assert torch.equal((got["S"] - c["r"][:rows]) == 0, dropped), f"mask at rows={rows}"
            assert rows * C < 1000 or 0 < int(dropped.sum()) < rows * C
    m.show(f"ln_fwd {family} p={p} eps={eps}")


def ln_bwd(gy, s, mean, rstd, gamma, rows, p, seed):
    """device tensors in -> (grad_x, grad_residual, dgamma, dbeta) on the CPU; asserts the return code and the guards"""
    L, ptr, stream_of, _ = abi()
    nbytes = L.vidar_drop_add_ln_bwd_workspace_bytes(rows)
    assert nbytes == NC.parts(rows) * 2 * C * 4
    outs = [window(rows * C), window(rows * C), window(C), window(C), window(nbytes // 4)]       # all NaN before the call
    rc = L.vidar_drop_add_ln_bwd_f32(ptr(gy), ptr(s), ptr(gamma), ptr(mean), ptr(rstd), *(ptr(w) for _, w in outs),
                                     rows, C, p, seed, stream_of(gy))
    torch.cuda.synchronize()
    assert rc == 0, f"vidar_drop_add_ln_bwd_f32 returned {rc}"
    assert all(guards_intact(b, w) for b, w in outs)
    gx, gres, dgamma, dbeta = (w.cpu() for _, w in outs[:4])
    return gx.view(rows, C), gres.view(rows, C), dgamma, dbeta


@pytest.mark.parametrize("mode", [False, True], ids=["default", "deterministic"])
@pytest.mark.parametrize("eps", NC.EPSES)
@pytest.mark.parametrize("family,p", NC.LN_GRID, ids=LN_IDS)
def test_ln_backward_within_the_derived_bounds(family, p, eps, mode):
    from vidar_amd import deterministic
    abi()
    c = NC.ln_case(family, away=p > 0)
    f = NC.ln_forward(c["x"], c["r"], c["gamma"], c["beta"], p, eps, NC.SEED)
    s, mean, rstd = NC.ln_given(f)
    b = NC.ln_backward(c["gy"], s, mean, rstd, c["gamma"], f["keep"], p)
    gy_d, s_d, mean_d, rstd_d, gamma_d = (dev(t) for t in (c["gy"], s, mean, rstd, c["gamma"]))
    m = Margins()
    with deterministic.use(mode):
        for rows in NC.ROWS:
            call = lambda: ln_bwd(gy_d[:rows], s_d[:rows], mean_d[:rows], rstd_d[:rows], gamma_d, rows, p, NC.SEED)
            gx, gres, dgamma, dbeta = call()
            where = f"rows={rows}"
            m.see("grad_residual", gres, b["gres"][:rows], b["bound_res"][:rows], where)
            m.see("grad_x", gx, b["gx"][:rows], b["bound_x"][:rows], where)
            want_dgamma, dgamma_bound, want_dbeta = NC.affine_grads(b, c["gy"], rows)
            m.see("dgamma", dgamma, want_dgamma, dgamma_bound, where)
            assert torch.equal(dbeta.double(), want_dbeta), f"dbeta at {where}"
            assert bool((gx[~f["keep"][:rows]] == 0).all()), f"grad_x at the dropped set, {where}"
            if mode:
                for _ in range(2):
                    assert all(NC.same_bits(u, v) for u, v in zip(call(), (gx, gres, dgamma, dbeta))), where
    m.show(f"ln_bwd {family} p={p} eps={eps} mode={mode}")


def test_ln_with_no_rows():
    L, ptr, stream_of, _ = abi()
    c = NC.ln_case("normal")
    x, gamma, beta = dev(c["x"][:4]), dev(c["gamma"]), dev(c["beta"])
    outs = [window(4 * C), window(4 * C), window(4), window(4)]
    assert L.vidar_drop_add_ln_fwd_f32(ptr(x), ptr(x), ptr(gamma), ptr(beta), *(ptr(w) for _, w in outs), 0, C, 0.1, 1e-5,
                                       1, stream_of(x)) == 0
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(b).all()) for b, _ in outs)               # the forward writes nothing
    assert L.vidar_drop_add_ln_bwd_workspace_bytes(0) == 0
    gx, gr, dg, db = window(4 * C), window(4 * C), window(C), window(C)
    assert L.vidar_drop_add_ln_bwd_f32(ptr(x), ptr(x), ptr(gamma), ptr(outs[2][1]), ptr(outs[3][1]), ptr(gx[1]), ptr(gr[1]),
                                       ptr(dg[1]), ptr(db[1]), None, 0, C, 0.1, 1, stream_of(x)) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(gx[0]).all()) and bool(torch.isnan(gr[0]).all())
    for buf, win in (dg, db):                                             # the backward zeroes the affine gradients
        assert bool((win == 0).all()) and guards_intact(buf, win)


# ---- dropout(relu(x)) --------------------------------------------------------------------------------------------------
def relu_fwd(x_host, p, seed, in_place):
    L, ptr, stream_of, _ = abi()
    n = x_host.numel()
    buf, y = window(n)
    if in_place:
        y.copy_(x_host)
        x = y
    else:
        x = dev(x_host)
    rc = L.vidar_relu_drop_fwd_f32(ptr(x), ptr(y), n, p, seed, stream_of(y))
    torch.cuda.synchronize()
    assert rc == 0 and guards_intact(buf, y)
    return y.cpu()


def relu_bwd(gy_host, y_host, p, in_place):
    L, ptr, stream_of, _ = abi()
    n = gy_host.numel()
    buf, gx = window(n)
    if in_place:
        gx.copy_(gy_host)
        gy = gx
    else:
        gy = dev(gy_host)
    y = dev(y_host)
    rc = L.vidar_relu_drop_bwd_f32(ptr(gy), ptr(y), ptr(gx), n, p, stream_of(y))
    torch.cuda.synchronize()
    assert rc == 0 and guards_intact(buf, gx)
    return gx.cpu()


@pytest.mark.parametrize("p", NC.RELU_PS)
@pytest.mark.parametrize("n", NC.RELU_SIZES)
def test_relu_drop_bits(n, p):
    c = NC.relu_case(n)
    want_y = NC.relu_drop(c["x"], NC.SEED, p)
    want_gx = NC.relu_drop_bwd(c["gy"], want_y, p)
    for in_place in (False, True):
        assert NC.same_bits(relu_fwd(c["x"], p, NC.SEED, in_place), want_y), f"forward, in_place={in_place}"
        assert NC.same_bits(relu_bwd(c["gy"], want_y, p, in_place), want_gx), f"backward, in_place={in_place}"
    if p > 0 and n >= 1020:
        assert 0 < int((want_y > 0).sum()) < int((c["x"] > 0).sum())        # some positive elements dropped, some kept


@pytest.mark.parametrize("p", NC.RELU_PS)
def test_relu_drop_planted_values(p):
    x, gy, kept, dropped = NC.relu_planted(NC.SEED, p)
    want_y = NC.relu_drop(x, NC.SEED, p)
    y = relu_fwd(x, p, NC.SEED, False)
    assert NC.same_bits_or_nan(y, want_y)
    zero, nzero, den, inf, ninf, nan = range(6)
    sc = float(NC.scale32(p))
    assert float(y[kept[nan]]) == 0 and float(y[kept[inf]]) == math.inf and float(y[kept[ninf]]) == 0
    assert float(y[kept[den]]) == float(np.float32(NC.DENORMAL) * np.float32(sc)) > 0
    assert math.copysign(1, float(y[kept[nzero]])) > 0
    if p > 0:
        assert math.isnan(float(y[dropped[inf]])) and float(y[dropped[nan]]) == 0 and float(y[dropped[den]]) == 0
    want_gx = NC.relu_drop_bwd(gy, want_y, p)
    assert NC.same_bits_or_nan(relu_bwd(gy, want_y, p, False), want_gx)


# ---- column sums -------------------------------------------------------------------------------------------------------
def colsum(x_host):
    L, ptr, stream_of, _ = abi()
    rows, cols = x_host.shape
    x = dev(x_host) if rows else torch.empty(4, device="cuda")
    buf, out = window(cols)                                               # NaN before the call
    rc = L.vidar_colsum_f32(ptr(x), ptr(out), rows, cols, stream_of(out))
    torch.cuda.synchronize()
    assert rc == 0 and guards_intact(buf, out)
    return out.cpu()


@pytest.mark.parametrize("cols", NC.COLSUM_COLS)
def test_colsum_exact_on_integers_around_one_pass(cols):
    for rows, _ in (s for s in NC.COLSUM_SMALL if s[1] == cols):
        x = NC.colsum_int(rows, cols)
        assert torch.equal(colsum(x).double(), x.double().sum(0)), f"rows={rows}"


@pytest.mark.parametrize("rows,cols", NC.COLSUM_CAPPED)
def test_colsum_exact_on_integers_past_the_workgroup_cap(rows, cols):
    x = NC.colsum_int(rows, cols)
    assert torch.equal(colsum(x).double(), x.double().sum(0))


@pytest.mark.parametrize("rows,cols", NC.COLSUM_REAL)
def test_colsum_real_values_within_the_any_order_bound(rows, cols):
    x = NC.colsum_real(rows, cols)
    ok, ratio = NC.worst(colsum(x), x.double().sum(0), NC.colsum_bound(x))
    print(f"colsum {rows}x{cols} margin:colsum={ratio:.3f}")
    assert ok, ratio


def test_colsum_empty_and_refusals():
    L, ptr, stream_of, BAD_ARG = abi()
    assert bool((colsum(torch.empty(0, 128)) == 0).all())
    x = dev(NC.colsum_int(8, 8192))
    buf, out = window(8192)
    for cols in (12, 0, 8192):                                            # 3 groups, none, more than one workgroup row
        assert L.vidar_colsum_f32(ptr(x), ptr(out), 8, cols, stream_of(x)) == BAD_ARG
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())


# ---- arguments the entries refuse --------------------------------------------------------------------------------------
def slack(n):
    """a device tensor of n floats with 4 more behind it: the pointer 4 bytes on stays inside the allocation"""
    return torch.full((n + 4,), math.nan, device="cuda")[:n]


def entries(rows=5, n=1024):
    """name -> (function, [(pointer name, tensor, read or written as float4)], the valid scalar arguments)"""
    L, _, stream_of, _ = abi()
    big, row, vec = rows * C, rows, C
    st = stream_of(torch.empty(1, device="cuda"))
    ws = L.vidar_drop_add_ln_bwd_workspace_bytes(rows) // 4
    t = lambda size, v: (slack(size), v)
    return {
        "ln_fwd": (L.vidar_drop_add_ln_fwd_f32,
                   dict(x=t(big, 1), residual=t(big, 1), gamma=t(vec, 1), beta=t(vec, 1), y=t(big, 1), sum_out=t(big, 1),
                        mean_out=t(row, 0), rstd_out=t(row, 0)),
                   dict(rows=rows, C=C, p=0.1, eps=1e-5, seed=1, stream=st)),
        "ln_bwd": (L.vidar_drop_add_ln_bwd_f32,
                   dict(grad_y=t(big, 1), sum_in=t(big, 1), gamma=t(vec, 1), mean_in=t(row, 0), rstd_in=t(row, 0),
                        grad_x=t(big, 1), grad_residual=t(big, 1), grad_gamma=t(vec, 0), grad_beta=t(vec, 0),
                        workspace=t(ws, 1)),
                   dict(rows=rows, C=C, p=0.1, seed=1, stream=st)),
        "relu_fwd": (L.vidar_relu_drop_fwd_f32, dict(x=t(n, 1), y=t(n, 1)), dict(n=n, p=0.1, seed=1, stream=st)),
        "relu_bwd": (L.vidar_relu_drop_bwd_f32, dict(grad_y=t(n, 1), y=t(n, 1), grad_x=t(n, 1)),
                     dict(n=n, p=0.1, stream=st)),
        "colsum": (L.vidar_colsum_f32, dict(x=t(rows * 64, 1), out=t(64, 0)), dict(rows=rows, cols=64, stream=st)),
    }


BAD_SCALARS = {
    "ln_fwd": [dict(p=math.nan), dict(p=1.0), dict(p=-0.1), dict(C=128), dict(C=0), dict(rows=-1)],
    "ln_bwd": [dict(p=math.nan), dict(p=1.0), dict(p=-0.1), dict(C=128), dict(C=0), dict(rows=-1)],
    "relu_fwd": [dict(p=math.nan), dict(p=1.0), dict(p=-0.1), dict(n=-4), dict(n=1022)],
    "relu_bwd": [dict(p=math.nan), dict(p=1.0), dict(p=-0.1), dict(n=-4), dict(n=1022)],
    "colsum": [dict(rows=-1), dict(cols=12), dict(cols=0), dict(cols=-64), dict(cols=8192)],
}


@pytest.mark.parametrize("entry", list(BAD_SCALARS))
def test_bad_arguments_are_refused_and_write_nothing(entry):
    _, _, _, BAD_ARG = abi()
    fn, ptrs, scalars = entries()[entry]
    where = {k: t.data_ptr() for k, (t, _) in ptrs.items()}
    call = lambda ps, sc: fn(*ps.values(), *sc.values())
    for bad in BAD_SCALARS[entry]:
        assert call(where, {**scalars, **bad}) == BAD_ARG, bad
    for name, (_, is_vec) in ptrs.items():
        # the entry returns on either before it launches anything (csrc/norm_fuse.hip: `given`, `vec`)
        assert call({**where, name: None}, scalars) == BAD_ARG, f"{name} = NULL"
        if is_vec:
            assert call({**where, name: where[name] + 4}, scalars) == BAD_ARG, f"{name} 4 bytes off"
    torch.cuda.synchronize()
    for name, (t, _) in ptrs.items():
        assert bool(torch.isnan(t).all()), f"{name} was written"


# ---- the autograd Functions --------------------------------------------------------------------------------------------
def off_by_one(t):
    """`t` as a contiguous device view that starts one float into its storage"""
    buf = torch.empty(t.numel() + 1, device="cuda")
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() % 16 == 4
    return out


def test_functions_clone_a_view_off_the_16_byte_boundary():
    from vidar_amd import deterministic
    from vidar_amd.plugin import bricks
    c = NC.ln_case("normal")
    rows = 37
    norm = torch.nn.LayerNorm(C).cuda()
    with torch.no_grad():
        norm.weight.copy_(c["gamma"]); norm.bias.copy_(c["beta"])
    results = []
    with deterministic.use(True):                                          # dgamma / dbeta in a fixed order
        for place in (off_by_one, dev):
            x, r = (place(c[k][:rows]).detach().requires_grad_() for k in ("x", "r"))
            gy = place(c["gy"][:rows])
            torch.manual_seed(11)
            y = bricks.drop_add_layernorm(x, r, norm, 0.3, training=True)
            grads = torch.autograd.grad(y, [x, r, norm.weight, norm.bias], gy)
            h = place(c["x"][:rows]).detach().requires_grad_()
            z = bricks._ReluDropout.apply(h, 0.3, 12345)
            gh, = torch.autograd.grad(z, h, gy)
            results.append([t.detach().cpu() for t in (y, *grads, z, gh)])
    assert all(NC.same_bits(u, v) for u, v in zip(*results))
    assert 0 < int((results[0][5] == 0).sum()) < rows * C
