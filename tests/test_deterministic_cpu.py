"""CPU: the deterministic mode without a GPU -- the fixed-point arithmetic of vidar_amd/csrc/det_acc.h compiled for
the host (tests/det_acc_host.cpp), the Python switch (vidar_amd/deterministic.py), the coverage table, and the
uncovered ops, which must raise before they touch the GPU."""
import os
import subprocess
import sys
import warnings
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("det_acc_host") / "det_acc_host"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'vidar_amd' / 'csrc'}",
                    str(ROOT / "tests" / "det_acc_host.cpp"), "-o", str(exe)], check=True)
    return exe


@pytest.fixture(scope="module")
def host_output(host_exe):
    r = subprocess.run([str(host_exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@pytest.mark.parametrize("check", ["permutation", "error bound", "overflow", "edge cases", "identity"])
def test_host_arithmetic(host_output, check):
    """1e5 contributions over 12 decades give the same bits under 20 permutations and lie within N delta / 2 + one fp32
    rounding of the exact sum; 2^31 contributions of +-M do not overflow; M == 0 -> exact zeros, M inf / NaN -> NaN"""
    assert f"{check} ok" in host_output.splitlines(), host_output


@pytest.mark.parametrize("n,vals", [(1000, [0.1, -2.5e-3, 7.75, 3.0e-7, -7.9999995, 1.0e-3]),
                                    (1 << 31, [3.0e38, -1.5e38, 2.5e-3]),
                                    (7, [1.0e-40, 3.0e-41, -2.0e-45]),          # a denormal M
                                    (2, [0.5, 0.5])])                           # M a power of two
def test_header_against_exact_rationals(host_exe, n, vals):
    """the header's own h, delta, accumulator and result for one address (tests/det_acc_host.cpp `small`) against the
    documented formulas evaluated with fractions.Fraction: E with 2^E >= M (and <= 2 M for a normal M),
    delta = 2^(E - (62 - h)), q = round-half-even(v / delta), out = fp32(acc * delta), |acc delta - exact| <= N delta / 2"""
    import math
    import struct
    from fractions import Fraction
    f32 = [struct.unpack("f", struct.pack("f", v))[0] for v in vals]
    r = subprocess.run([str(host_exe), "small", str(n), *[repr(v) for v in f32]], capture_output=True, text=True, check=True)
    words = r.stdout.split()
    got = {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}
    h = math.ceil(math.log2(n))
    M = Fraction(max(abs(v) for v in f32))
    delta = Fraction(2) ** got["delta_exp"]
    E = got["delta_exp"] + 62 - h
    assert got["h"] == h
    assert Fraction(2) ** E >= M and (Fraction(2) ** E <= 2 * M or M < Fraction(2) ** -126)
    acc = sum(round(Fraction(v) / delta) for v in f32)           # round(): half to even, like llrint
    assert got["acc"] == acc and abs(acc) <= 2 ** 62
    exact = sum(Fraction(v) for v in f32)
    assert abs(acc * delta - exact) <= len(f32) * delta / 2
    assert len(f32) * delta / 2 <= M * Fraction(2) ** (2 * h - 62) or M < Fraction(2) ** -126
    out = struct.unpack("f", struct.pack("I", got["out"]))[0]
    assert out == struct.unpack("f", struct.pack("f", float(acc * delta)))[0]      # one rounding to fp32


@pytest.fixture
def det():
    from vidar_amd import deterministic as d
    saved = (d._mode, d._warn_only, set(d._warned))
    torch_saved = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled())
    yield d
    d._mode, d._warn_only = saved[:2]
    d._warned.clear(); d._warned.update(saved[2])
    torch.use_deterministic_algorithms(torch_saved[0], warn_only=torch_saved[1])


def test_set_use_and_following_torch(det):
    det.set(None)
    torch.use_deterministic_algorithms(False)
    assert det.enabled() is False
    torch.use_deterministic_algorithms(True)
    assert det.enabled() is True and det.warn_only() is False
    torch.use_deterministic_algorithms(True, warn_only=True)
    assert det.enabled() is True and det.warn_only() is True
    det.set(False)                                   # an explicit setting wins over torch, in both directions
    assert det.enabled() is False
    torch.use_deterministic_algorithms(False)
    det.set(True)
    assert det.enabled() is True and det.warn_only() is False
    with det.use(False):
        assert det.enabled() is False
        with det.use(True, warn_only=True):
            assert det.enabled() is True and det.warn_only() is True
        assert det.enabled() is False
    assert det.enabled() is True
    with det.use(None):
        assert det.enabled() is False                # torch's flag is off
    assert det.set(None) is True and det.enabled() is False
    with pytest.raises(TypeError):
        det.set("yes")


@pytest.mark.parametrize("value,want", [("1", "True"), ("0", "False"), (None, "None")])
def test_environment_start_value(value, want):
    env = {k: v for k, v in os.environ.items() if k != "VIDAR_DETERMINISTIC"}
    if value is not None:
        env["VIDAR_DETERMINISTIC"] = value
    code = "from vidar_amd import deterministic as d; print(d._mode, d.enabled())"
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, check=True)
    assert out.stdout.split() == [want, "True" if value == "1" else "False"]


def test_environment_rejects_other_values():
    env = dict(os.environ, VIDAR_DETERMINISTIC="yes")
    r = subprocess.run([sys.executable, "-c", "import vidar_amd.deterministic"], env=env, cwd=ROOT, capture_output=True)
    assert r.returncode != 0 and b"VIDAR_DETERMINISTIC" in r.stderr


def test_library_switch_returns_the_previous_value(det):
    from vidar_amd._lib import lib
    L = lib()
    was = L.vidar_set_deterministic(1)
    try:
        assert L.vidar_get_deterministic() == 1
        assert L.vidar_set_deterministic(0) == 1 and L.vidar_get_deterministic() == 0
        assert L.vidar_set_deterministic(7) == 0 and L.vidar_get_deterministic() == 1      # any non-zero value is "on"
        with det.use(False):
            assert det.sync() is False and L.vidar_get_deterministic() == 0
        with det.use(True):
            assert det.sync() is True and L.vidar_get_deterministic() == 1
    finally:
        L.vidar_set_deterministic(was)


def test_workspace_queries_follow_the_switch():
    """host-only arithmetic: in the mode 8 B per output element + one 8-byte slot per output for its max word"""
    import ctypes
    from vidar_amd._lib import lib
    L = lib()
    off = (L.vidar_msda_bwd_workspace_bytes(2, 300, 8, 600, 2, 4), L.vidar_ray_bwd_workspace_bytes(2, 16, 24, 24),
           L.vidar_latent_render_bwd_workspace_bytes(1, 24, 24, 16, 2))
    n = ctypes.c_int64(-1)
    assert L.vidar_knn1_d3_bwd_workspace_bytes(2, 50, ctypes.addressof(n)) == 0 and n.value == 0
    was = L.vidar_set_deterministic(1)
    try:
        assert L.vidar_msda_bwd_workspace_bytes(2, 300, 8, 600, 2, 4) == 8 * (2 * 300 * 8 * 32 + 1)
        assert L.vidar_ray_bwd_workspace_bytes(2, 16, 24, 24) == 8 * (2 * 16 * 24 * 24 + 1)
        assert L.vidar_latent_render_bwd_workspace_bytes(1, 24, 24, 16, 1) == 8 * (24 * 24 * 16 + 1)
        assert L.vidar_latent_render_bwd_workspace_bytes(1, 24, 24, 16, 2) == 8 * (2 * 24 * 24 * 16 + 2)
        assert L.vidar_knn1_d3_bwd_workspace_bytes(2, 50, ctypes.addressof(n)) == 0 and n.value == 8 * (2 * 50 * 3 + 1)
        assert L.vidar_dcn_col2im_det_workspace_bytes(2, 16, 12, 20, ctypes.addressof(n)) == 0
        assert n.value == 8 * (2 * 16 * 12 * 20 + 1)
    finally:
        L.vidar_set_deterministic(was)
    assert off == (L.vidar_msda_bwd_workspace_bytes(2, 300, 8, 600, 2, 4), L.vidar_ray_bwd_workspace_bytes(2, 16, 24, 24),
                   L.vidar_latent_render_bwd_workspace_bytes(1, 24, 24, 16, 2))


def test_coverage_table(det):
    rows = det.coverage()
    assert all(len(r) == 3 and all(isinstance(x, str) and x for x in r) for r in rows)
    status = {op: s for op, s, _ in rows}
    assert set(status.values()) == {"fixed-point", "fixed-order", "already deterministic", "not covered"}
    for op in ("msda backward", "ray_ce backward", "ray_gumbel backward", "ray_dist backward", "latent_render backward",
               "knn1_d3 backward", "dcn col2im"):
        assert status[op] == "fixed-point", op
    for op in ("drop_add_ln backward", "bias gradient"):
        assert status[op] == "fixed-order", op
    for op in UNCOVERED:
        assert status[op] == "not covered", op
    # the README prints the table as it is
    assert det.coverage_table() in (ROOT / "README.md").read_text()


def _dvxlr(): from vidar_amd.third_lib import dvxlr; return dvxlr.get_grad_sigma(*[torch.zeros(1)] * 4)
def _dvxlr2(): from vidar_amd.third_lib import dvxlr_v2; return dvxlr_v2.get_grad_sigma_v2(*[torch.zeros(1)] * 6)
def _dvr(): from vidar_amd.third_lib import dvr; return dvr.render(*[torch.zeros(1)] * 4, "l1")
def _dcnv3(): from vidar_amd.third_lib import dcnv3; return dcnv3.dcnv3_backward(*[torch.zeros(1)] * 3, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1.0, torch.zeros(1), 64)


def _knn_generic():
    from vidar_amd.third_lib.chamferdist import _C
    p = torch.zeros(1, 4, 2)
    return _C.knn_points_backward(p, p, torch.zeros(1), torch.zeros(1), torch.zeros(1, 4, 1), torch.zeros(1, 4, 1))


UNCOVERED = {"dvxlr.get_grad_sigma": _dvxlr, "dvxlr_v2.get_grad_sigma": _dvxlr2, "dvr.render": _dvr,
             "dcnv3 backward": _dcnv3, "knn generic backward": _knn_generic}


@pytest.mark.parametrize("op", list(UNCOVERED))
def test_uncovered_ops_raise_before_any_gpu_call(det, op):
    """under the mode the wrapper raises RuntimeError naming the op -- with CPU arguments, on a machine without a GPU:
    nothing was checked, allocated or launched before; with warn_only it warns once and goes on (to the argument check
    that refuses the CPU tensors, which does not name the mode)"""
    with det.use(True):
        with pytest.raises(RuntimeError, match="does not have a deterministic implementation") as e:
            UNCOVERED[op]()
        assert op in str(e.value)
    det._warned.discard(op)
    with det.use(True, warn_only=True):
        for expect_warning in (True, False):                    # once per op
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                with pytest.raises(Exception) as e:
                    UNCOVERED[op]()
                assert "deterministic implementation" not in str(e.value)
            named = [x for x in w if op in str(x.message)]
            assert bool(named) == expect_warning, [str(x.message) for x in w]
        assert op in det.warned()
    with det.use(None):
        torch.use_deterministic_algorithms(True)               # following torch's flag
        with pytest.raises(RuntimeError, match="does not have a deterministic implementation"):
            UNCOVERED[op]()
        torch.use_deterministic_algorithms(True, warn_only=True)
        with pytest.raises(Exception) as e:
            UNCOVERED[op]()
        assert "deterministic implementation" not in str(e.value)
