"""Golden vectors for the DCNv3 operator: the reference's `dcnv3_core_pytorch`
(bevformer/backbones/ops_dcnv3/functions/dcnv3_func.py:147-190) and its module `DCNv3_pytorch`
(modules/dcnv3.py:95-218) executed in place, in fp64, on the CPU.  Stored: operands, outputs and the gradients of
sum(output * grad_out); for the module also its weights.  Operands and weights are fp32-representable values, so a
fp32 implementation starts from the very same numbers.  -> tests/golden/dcnv3_core.npz, dcnv3_module.npz

STUBS (none of the arithmetic under test lives in them): the compiled extension `DCNv3` (an empty module; only the
pure-torch path is executed) and a package shell `refbackbones` whose __path__ is the reference's backbones directory,
so that the reference files' relative imports resolve without running backbones/__init__.py.

Run in the build container:   python tests/golden/make_dcnv3_golden.py
"""
import importlib
import sys
import types
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).parent
sys.path.insert(0, str(HERE))
import ref_import  # noqa: E402

# (name, N, H, W, G, gc, kh, kw, sh, sw, ph, pw, dh, dw, offset_scale, offset sigma in pixels)
CORE_CASES = [
    ("k3_gc16", 2, 9, 11, 4, 16, 3, 3, 1, 1, 1, 1, 1, 1, 1.0, 1.5),
    ("k3_gc3_s2_d2", 1, 12, 10, 2, 3, 3, 3, 2, 2, 0, 0, 2, 2, 2.5, 1.5),
    ("k1x3_hw", 2, 8, 13, 3, 8, 1, 3, 1, 2, 1, 1, 1, 2, 1.0, 1.5),
    ("k5_gc32_far", 1, 10, 9, 1, 32, 5, 5, 1, 1, 2, 2, 1, 1, 1.0, 12.0),
]


def reference_ops():
    """-> (functions.dcnv3_func, modules.dcnv3) of the reference, imported where they lie"""
    ref_import.install_stubs()
    sys.modules.setdefault("DCNv3", types.ModuleType("DCNv3"))            # STUB: the compiled extension, never called
    if "refbackbones" not in sys.modules:
        pkg = types.ModuleType("refbackbones")                           # STUB: package shell, see the docstring
        pkg.__path__ = [str(ref_import.PLUGIN / "bevformer/backbones")]
        sys.modules["refbackbones"] = pkg
    return (importlib.import_module("refbackbones.ops_dcnv3.functions.dcnv3_func"),
            importlib.import_module("refbackbones.ops_dcnv3.modules.dcnv3"))


def out_size(n, k, s, p, d):
    return (n + 2 * p - (d * (k - 1) + 1)) // s + 1


def core_operands(case, seed):
    _, N, H, W, G, gc, kh, kw, sh, sw, ph, pw, dh, dw, os_, sigma = case
    g = torch.Generator().manual_seed(seed)
    Ho, Wo, P = out_size(H, kh, sh, ph, dh), out_size(W, kw, sw, pw, dw), kh * kw
    f32 = lambda t: t.float().double()
    x = f32(torch.randn(N, H, W, G * gc, generator=g))
    off = f32(torch.randn(N, Ho, Wo, G * P * 2, generator=g) * sigma)
    mask = f32(torch.softmax(torch.randn(N, Ho, Wo, G, P, generator=g), -1).reshape(N, Ho, Wo, G * P))
    gout = f32(torch.randn(N, Ho, Wo, G * gc, generator=g))
    return x, off, mask, gout


def randomise(module, seed, scale=0.05):
    """fp32-representable noise on every parameter (the reference initialises the offset / mask layers to zero, which
    would put every sample exactly on a pixel centre)"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for _, p in sorted(module.named_parameters()):
            p.copy_((p + scale * torch.randn(p.shape, generator=g, dtype=torch.float64)).float().double())


def main():
    fn, mod = reference_ops()
    out = {}
    for ci, case in enumerate(CORE_CASES):
        name = case[0]
        x, off, mask, gout = (t.requires_grad_(True) if i < 3 else t for i, t in enumerate(core_operands(case, 100 + ci)))
        y = fn.dcnv3_core_pytorch(x, off, mask, *case[6:14], case[4], case[5], case[14])
        gi, go, gm = torch.autograd.grad((y * gout).sum(), [x, off, mask])
        for k, v in dict(input=x, offset=off, mask=mask, grad_out=gout, out=y, grad_input=gi, grad_offset=go,
                         grad_mask=gm).items():
            out[f"{name}.{k}"] = v.detach().numpy()
    np.savez_compressed(HERE / "dcnv3_core.npz", **out)

    out = {}
    for name, kw in (("ln", dict(channels=32, group=4)),
                     ("cfs_dw5", dict(channels=24, group=3, dw_kernel_size=5, center_feature_scale=True, offset_scale=2.0))):
        torch.manual_seed(7)
        m = mod.DCNv3_pytorch(**kw).double()
        randomise(m, 11)
        g = torch.Generator().manual_seed(5)
        x = torch.randn(2, 7, 9, kw["channels"], generator=g).float().double().requires_grad_(True)
        y = m(x)
        gout = torch.randn(y.shape, generator=g).float().double()
        params = sorted(m.named_parameters())
        grads = torch.autograd.grad((y * gout).sum(), [x] + [p for _, p in params])
        out[f"{name}.input"], out[f"{name}.grad_out"], out[f"{name}.out"] = x.detach().numpy(), gout.numpy(), y.detach().numpy()
        out[f"{name}.grad_input"] = grads[0].numpy()
        for (k, p), gr in zip(params, grads[1:]):
            out[f"{name}.w.{k}"] = p.detach().numpy().astype(np.float32)
            out[f"{name}.g.{k}"] = gr.numpy()
    np.savez_compressed(HERE / "dcnv3_module.npz", **out)
    for f in ("dcnv3_core.npz", "dcnv3_module.npz"):
        print(f, (HERE / f).stat().st_size)


if __name__ == "__main__":
    main()
