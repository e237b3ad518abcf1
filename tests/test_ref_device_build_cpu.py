"""CPU: the recipe of the reference's DEVICE build (oracle/build_ref.py: HIP_TOKENS, build_hip) and the
host-first rule for everything that tests/test_reference_device_gpu.py sends to those kernels.

  * the text hipcc reads is the reference text under the committed token table and nothing else;
  * each built library holds a gfx950 code object with the reference's own kernel names;
  * every input set of the GPU test runs here first through the HOST build of the same kernel bodies (every entry
    point the GPU test calls): voxel indices inside the grid, per-ray counts within MAX_D, results equal to
    oracle/dvr_oracle.c as in tests/test_oracle_dvr.py;
  * the rays on which dvr.render's racy `grad_sigma +=` (dvr.cu:622) is compared on a device share no voxel."""
import re
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest
import torch

import dvr_device_sets as S
from oracle import build_ref
from oracle import dvr as O

ROOT = Path(__file__).resolve().parents[1]
ts = torch.from_numpy
needs_reference = pytest.mark.skipif(not build_ref.available(), reason="reference tree absent")

KERNELS = {
    "ref_dvr_hip": {"init_cuda_kernel", "render_forward_cuda_kernel", "render_cuda_kernel"},
    "ref_dvxlr_hip": {"init_cuda_kernel", "get_grad_sigma_cuda_kernel", "render_cuda_kernel"},
    "ref_dvxlr_v2_hip": {"get_grad_sigma_cuda_v2_kernel", "render_cuda_v2_kernel"},
}


@needs_reference
@pytest.mark.parametrize("name", list(build_ref.HIP_MODULES))
def test_compiler_reads_the_reference_text_under_the_token_table_only(name):
    ref = (build_ref.REF / build_ref.HIP_MODULES[name][0]).read_text()
    text, hits = build_ref.hip_text(ref)
    a, b = ref.split("\n"), text.split("\n")
    assert len(a) == len(b)
    differing = 0
    for ra, rb in zip(a, b):
        if ra != rb:
            differing += 1
            assert build_ref.hip_line(ra)[0] == rb
    assert differing == hits and hits >= 5          # two includes, one synchronise and one dispatch at the least
    assert len(build_ref.HIP_TOKENS) == 3
    assert not re.search(r"\bcuda[A-Z]|<cuda|\.type\(\)", text)
    for word in ("<<<blocks, threads>>>", "__global__"):
        assert ref.count(word) == text.count(word) > 0
    assert ref.count("atomicAdd") == text.count("atomicAdd")


@needs_reference
@pytest.mark.parametrize("name", list(build_ref.HIP_MODULES))
def test_built_library_holds_the_reference_kernels_for_gfx950(name, ref_modules):
    ref_modules("ref_dvr")                      # builds oracle/_ref where it is missing
    so = build_ref.so_path(name)
    assert so.exists(), f"{so.name} was not built"
    sys.path.insert(0, str(ROOT / "tools"))
    import kernel_resources as K
    names = []
    with tempfile.TemporaryDirectory() as d:
        objs = K.code_objects(so, Path(d))
        assert objs, "no gfx950 code object in the library"
        for co in objs:
            names += [k[".name"] for k in K.kernels_of(co)]      # asserts amdhsa.target ends with gfx950
    short = {K.short(n).split("<")[0] for n in K.demangle(names)}
    assert KERNELS[name] <= short, (KERNELS[name] - short, short)


def _np(xs):
    return [x.numpy() for x in xs]


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _close(a, b):
    """the bounds of tests/test_oracle_dvr.py for a volume summed in another order; NaN voxels (the rays of zero
    length poison theirs) must be the same ones."""
    fin = np.abs(a[np.isfinite(a)])
    return np.allclose(a, b, rtol=1e-4, atol=1e-5 * max(1.0, float(fin.max()) if fin.size else 0.0), equal_nan=True)


@pytest.mark.parametrize("name", [*S.SET_NAMES, "noshare"])
def test_device_input_sets_pass_the_host_build_first(name, ref_modules):
    dvr, dvxlr, v2 = ref_modules("ref_dvr"), ref_modules("ref_dvxlr"), ref_modules("ref_dvxlr_v2")
    sigma, origin, points, tindex, regul = S.load(name)
    t = [ts(sigma), ts(origin), ts(points), ts(tindex)]
    o = O.dvxlr_render(sigma, origin, points, tindex, regul)
    r = _np(v2.render_v2(*t, ts(regul)))
    S.assert_in_grid(sigma, r[3], r[5])
    for a, b, nm in zip(r, o, ["pred", "gt", "dd", "idx", "ray_pred", "indicator"]):
        assert _same(a, b), nm
    del r
    r = _np(dvxlr.render(*t))
    for a, b, nm in zip(r, o, ["pred", "gt", "dd", "idx"]):
        assert _same(a, b), nm
    del r
    if o[2].size:
        em, grp = S.scatter_inputs(o)
        og = O.dvxlr_get_grad_sigma(em, o[3], tindex, sigma.shape, o[5], grp)
        g = dvxlr.get_grad_sigma(ts(em), ts(o[3]), t[3], t[0])[0].numpy()
        g1, g2 = _np(v2.get_grad_sigma_v2(ts(em), ts(o[3]), t[3], t[0], ts(o[5]), ts(grp)))
        for a, b in ((g, og[0]), (g1, og[0]), (g2, og[1])):
            assert _close(a, b)
        del em, grp
    idx = o[3]
    del o
    grid = list(sigma.shape[1:])
    for ph in S.PHASES:
        for a, b in zip(_np(dvr.render_forward(*t, grid, ph)), O.render_forward(sigma, origin, points, tindex, ph)):
            assert _same(a, b), ph
    for ls in S.LOSSES:
        r = _np(dvr.render(*t, ls))
        w = O.render(sigma, origin, points, tindex, ls)
        assert _same(r[0], w[0]) and _same(r[1], w[1]), ls
        assert _close(r[2], w[2]), ls
    g = S.init_grid(sigma, origin)
    want = O.init(points, tindex, g)
    assert _same(dvr.init(t[2], t[3], g).numpy(), want) and _same(dvxlr.init(t[2], t[3], g).numpy(), want)
    if name == "noshare":
        live = S.assert_no_shared_voxel(sigma, origin, points, tindex, idx)
        assert live >= 24, f"only {live} rays left"
