"""GPU: the reference's own dvr / dvxlr / dvxlr_v2 DEVICE kernels (oracle/_ref/ref_*_hip.so: the reference .cu files
compiled by hipcc for gfx950 under the three-row token table of oracle/build_ref.py) against

  1. oracle/dvr_oracle.c, the restatement every other dvr test compares with, and
  2. the product kernels (vidar_amd.third_lib.{dvr,dvxlr,dvxlr_v2}) under each launch variant.

Index lists, `indicator` and occupancy: bit-exact, NaN equal to NaN.  pred / gt_dist / dd / ray_pred: rtol 2e-5 and
atol 2e-6 * max(1, |ref|_max), the bounds of tests/test_fullsize_parity_gpu.py::_close (device exp / sqrt need not
be glibc's); every comparison prints how many elements differ at all and by how much at the worst.
get_grad_sigma(_v2) adds with float atomics in any order: rtol 1e-4, atol 1e-5 * max(1, |ref|_max) against the fp64
accumulation of the same (index, value) lists, as tests/test_dvr_gpu.py::test_dvxlr_get_grad_sigma.

dvr.render's grad_sigma: dvr.cu:622 is a plain `+=` from one thread per ray, which the reference's own comment calls
racy; on a device it loses updates wherever two rays share a voxel, so there it is no reference.  It is compared
only on `noshare` (dvr_device_sets.noshare_case: rays of `two_frames` thinned until no two share a voxel, asserted
on the CPU and again here); on every other set only dvr.render's per-ray outputs are compared with the device
reference, and its grad_sigma stays pinned to the host build (tests/test_oracle_dvr.py, tests/test_dvr_gpu.py).

The reference kernels check no argument.  Every set comes from tests/dvr_device_sets.py, and the CPU suite has run
each through the host build of the same kernel bodies first (tests/test_ref_device_build_cpu.py).  The libraries are
loaded with build_ref.load: a missing one is a failure, not a skip."""
import ctypes

import numpy as np
import pytest
import torch

import dvr_device_sets as S
from oracle import build_ref
from oracle import dvr as O
from test_fullsize_parity_gpu import VARIANTS, _restore, _set_variant

pytestmark = pytest.mark.gpu
HIP_INVALID_CONFIGURATION = 9                    # what a launch of zero blocks (no rays) answers


def _hip_runtime():
    """the HIP runtime this process already uses (the reference checks none of its launches: the test does)."""
    with open("/proc/self/maps") as maps:
        for line in maps:
            if "libamdhip64.so" in line:
                return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime loaded")


def _ref_call(fn, *args, rays=1):
    """the reference launches on the null stream and then synchronises the device itself"""
    torch.cuda.synchronize()
    out = fn(*args)
    err = _hip_runtime().hipGetLastError()
    assert err == 0 or (rays == 0 and err == HIP_INVALID_CONFIGURATION), f"reference launch failed: hipError {err}"
    return out


def _dev(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(tag, got, want):
    """bitwise equality (NaN == NaN), on the device"""
    got, want = _dev(got), _dev(want)
    assert got.shape == want.shape and got.dtype == want.dtype, tag
    bad = ~((got == want) | (got.isnan() & want.isnan()))
    n = int(bad.sum())
    print(f"[refdev] {tag}: {n} of {got.numel()} elements differ (bit-exact expected)")
    assert n == 0, f"{tag}: {n} elements differ; first at {bad.nonzero()[0].tolist()}"


def _floats(tag, got, want, rtol=2e-5, atol_rel=2e-6):
    got, want = _dev(got), _dev(want)
    assert got.shape == want.shape and got.dtype == want.dtype, tag
    nan = want.isnan()
    assert torch.equal(got.isnan(), nan), f"{tag}: NaN in other places"
    g, w = got.masked_fill(nan, 0), want.masked_fill(nan, 0)
    fin = w[w.isfinite()]
    scale = max(1.0, float(fin.abs().max())) if fin.numel() else 1.0
    ne = g != w                                   # infinities must be equal ones
    diff = (g - w).abs()
    worst = float(diff[ne].max()) if bool(ne.any()) else 0.0
    print(f"[refdev] {tag}: {int(ne.sum())} of {g.numel()} elements differ, worst |diff| {worst:.3e} "
          f"(|ref|_max {scale:.3e})")
    bad = ne & ~(diff <= atol_rel * scale + rtol * w.abs())
    assert not bool(bad.any()), f"{tag}: {int(bad.sum())} elements beyond rtol {rtol} / atol {atol_rel * scale:.3e}"


class Run:
    """one input set on the device, and the reference device kernels' results for it (computed once)"""

    def __init__(self, name):
        self.name = name
        self.host = S.load(name)
        self.sigma, self.origin, self.points, self.tindex, self.regul = self.dev = [_dev(a) for a in self.host]
        self.rays = self.points.shape[1]
        self.grid = list(self.sigma.shape[1:])
        self.init_grid = S.init_grid(*self.host[:2])
        self.mods = {m: build_ref.load(f"ref_{m}_hip") for m in ("dvr", "dvxlr", "dvxlr_v2")}
        self.cache = {}

    def ref(self, what, arg=None):
        key = (what, arg)
        if key not in self.cache:
            d, m = self.dev, self.mods
            call = {"dvxlr": lambda: m["dvxlr"].render(*d[:4]),
                    "v2": lambda: m["dvxlr_v2"].render_v2(*d),
                    "forward": lambda: m["dvr"].render_forward(*d[:4], self.grid, arg),
                    "render": lambda: m["dvr"].render(*d[:4], arg),
                    "init_dvr": lambda: m["dvr"].init(d[2], d[3], self.init_grid),
                    "init_dvxlr": lambda: m["dvxlr"].init(d[2], d[3], self.init_grid)}[what]
            self.cache[key] = _ref_call(call, rays=self.rays)
        return self.cache[key]


@pytest.fixture(scope="module", params=S.SET_NAMES)
def run(request):
    r = Run(request.param)
    yield r
    r.cache.clear()
    del r
    torch.cuda.empty_cache()


V2 = ["pred", "gt_dist", "dd", "idx", "ray_pred", "indicator"]
EXACT = {"idx", "indicator"}


def _compare_render(tag, got, want):
    for nm, a, b in zip(V2, got, want):
        (_bits if nm in EXACT else _floats)(f"{tag} {nm}", a, b)


def test_reference_device_kernels_match_the_oracle(run):
    """comparison 1: every entry point of the device reference against oracle/dvr_oracle.c"""
    s = run.host
    tag = f"ref-device vs oracle | {run.name} |"
    o = O.dvxlr_render(*s[:4], s[4])
    _compare_render(f"{tag} dvxlr_v2.render_v2", run.ref("v2"), o)
    _compare_render(f"{tag} dvxlr.render", run.ref("dvxlr"), o[:4])
    _bits(f"{tag} per-ray count", (run.ref("v2")[5] >= 0).sum(-1), (_dev(o[5]) >= 0).sum(-1))
    del o
    for ph in S.PHASES:
        w = O.render_forward(*s[:4], ph)
        for nm, a, b in zip(("pred", "gt_dist"), run.ref("forward", ph), w):
            _floats(f"{tag} dvr.render_forward[{ph}] {nm}", a, b)
    for ls in S.LOSSES:
        w = O.render(*s[:4], ls)
        for nm, a, b in zip(("pred", "gt_dist"), run.ref("render", ls), w):
            _floats(f"{tag} dvr.render[{ls}] {nm}", a, b)
    occ = O.init(s[2], s[3], run.init_grid)
    _bits(f"{tag} dvr.init occupancy", run.ref("init_dvr"), occ)
    _bits(f"{tag} dvxlr.init occupancy", run.ref("init_dvxlr"), occ)


def test_product_kernels_match_the_reference_device_kernels(run):
    """comparison 2: the product under each launch variant against the device reference"""
    from vidar_amd.third_lib import dvr, dvxlr, dvxlr_v2
    d = run.dev
    prev = _set_variant("plain")
    try:
        for variant in VARIANTS:
            _set_variant(variant)
            tag = f"product[{variant}] vs ref-device | {run.name} |"
            _compare_render(f"{tag} dvxlr_v2.render_v2", dvxlr_v2.render_v2(*d), run.ref("v2"))
            _compare_render(f"{tag} dvxlr.render", dvxlr.render(*d[:4]), run.ref("dvxlr"))
            for ph in S.PHASES:
                for nm, a, b in zip(("pred", "gt_dist"), dvr.render_forward(*d[:4], run.grid, ph), run.ref("forward", ph)):
                    _floats(f"{tag} dvr.render_forward[{ph}] {nm}", a, b)
            for ls in S.LOSSES:
                for nm, a, b in zip(("pred", "gt_dist"), dvr.render(*d[:4], ls)[:2], run.ref("render", ls)):
                    _floats(f"{tag} dvr.render[{ls}] {nm}", a, b)
            _bits(f"{tag} dvr.init occupancy", dvr.init(d[2], d[3], run.init_grid), run.ref("init_dvr"))
            _bits(f"{tag} dvxlr.init occupancy", dvxlr.init(d[2], d[3], run.init_grid), run.ref("init_dvxlr"))
    finally:
        _restore(prev)


def test_reference_device_scatter_matches_fp64_accumulation(run):
    """get_grad_sigma / get_grad_sigma_v2 of the device reference (float atomicAdd)"""
    s = run.host
    o = O.dvxlr_render(*s[:4], s[4])
    if o[2].size == 0:
        return
    em, grp = S.scatter_inputs(o)
    want = O.dvxlr_get_grad_sigma(em, o[3], s[3], s[0].shape, o[5], grp)
    dem, didx, dind, dgrp = (_dev(a) for a in (em, o[3], o[5], grp))
    tag = f"ref-device vs fp64 | {run.name} |"
    g = _ref_call(run.mods["dvxlr"].get_grad_sigma, dem, didx, run.tindex, run.sigma)[0]
    _floats(f"{tag} dvxlr.get_grad_sigma", g, want[0], rtol=1e-4, atol_rel=1e-5)
    g1, g2 = _ref_call(run.mods["dvxlr_v2"].get_grad_sigma_v2, dem, didx, run.tindex, run.sigma, dind, dgrp)
    _floats(f"{tag} dvxlr_v2.get_grad_sigma_v2 grad_sigma", g1, want[0], rtol=1e-4, atol_rel=1e-5)
    _floats(f"{tag} dvxlr_v2.get_grad_sigma_v2 grad_sigma_regul", g2, want[1], rtol=1e-4, atol_rel=1e-5)


@pytest.mark.parametrize("loss", S.LOSSES)
def test_dvr_render_grad_sigma_where_no_voxel_is_shared(loss):
    """the one set on which dvr.cu:622 has a single value on a device: no two rays of a volume share a voxel, so
    every voxel holds one double product rounded once -- no summation order, hence the host pin's bounds (rtol 1e-4,
    atol 1e-5 * max(1, |ref|_max), tests/test_oracle_dvr.py) for the oracle and for the product alike."""
    from vidar_amd.third_lib import dvr
    r = Run("noshare")
    s = r.host
    idx = O.dvxlr_render(*s[:4])[3]
    assert S.assert_no_shared_voxel(*s[:4], idx) >= 24
    ref = _ref_call(r.mods["dvr"].render, *r.dev[:4], loss)
    want = O.render(*s[:4], loss)
    tag = f"| noshare | dvr.render[{loss}]"
    for nm, a, b in zip(("pred", "gt_dist"), ref, want):
        _floats(f"ref-device vs oracle {tag} {nm}", a, b)
    assert int((ref[2] != 0).sum()) > 100
    _floats(f"ref-device vs oracle {tag} grad_sigma", ref[2], want[2], rtol=1e-4, atol_rel=1e-5)
    got = dvr.render(*r.dev[:4], loss)
    for nm, a, b in zip(("pred", "gt_dist"), got, ref):
        _floats(f"product vs ref-device {tag} {nm}", a, b)
    _floats(f"product vs ref-device {tag} grad_sigma", got[2], ref[2], rtol=1e-4, atol_rel=1e-5)
