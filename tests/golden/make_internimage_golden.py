"""Golden vectors for the InternImage backbone: the reference's `InternImage(core_op="DCNv3_pytorch")`
(bevformer/backbones/internimage.py:527-702) executed in place, in fp64, on the CPU.  Per case
tests/golden/internimage_<case>.npz holds the input image, the weights (fp32-representable values, stored as fp32), the
outputs of `out_indices`, the cotangents g_i and the gradients of sum_i sum(out_i * g_i) with respect to the input and
every parameter; internimage_<case>.json holds the constructor arguments and the sorted `state_dict` keys with shapes.
Every committed file has to stay below 1 MiB, hence channels = 6 (group sizes 6, 12, 24, 24) and mlp_ratio = 2.

STUBS installed here (none of the arithmetic under test lives in them): `timm.models.layers` (`trunc_normal_` = torch's,
`DropPath` = identity: drop_path_rate is 0 in every case), `mmcv.runner._load_checkpoint`, `mmcv.cnn.constant_init` /
`trunc_normal_init` (no-ops; `init_weights()` is not called), `mmdet.utils.get_root_logger` (a silent logger),
`mmdet.models.builder.BACKBONES` (no-op registry), plus the `DCNv3` / package stubs of make_dcnv3_golden.py.

Run in the build container:   python tests/golden/make_internimage_golden.py
"""
import importlib
import json
import logging
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn as nn

HERE = Path(__file__).parent
sys.path.insert(0, str(HERE))
import ref_import  # noqa: E402
from make_dcnv3_golden import randomise, reference_ops  # noqa: E402

BASE = dict(core_op="DCNv3_pytorch", channels=6, depths=[1, 1, 2, 1], groups=[1, 1, 1, 2], mlp_ratio=2.0,
            drop_path_rate=0.0, out_indices=[0, 1, 2, 3])
CASES = {
    "base": dict(BASE),
    "h_style": dict(BASE, dw_kernel_size=5, res_post_norm=True, level2_post_norm=True, level2_post_norm_block_ids=[0],
                    center_feature_scale=True, offset_scale=2.0),
    "post_norm": dict(BASE, post_norm=True, layer_scale=0.5, out_indices=[1, 2, 3]),
}
IMAGE = (2, 3, 48, 64)


def reference_internimage():
    reference_ops()
    null = logging.getLogger("internimage_golden")
    null.addHandler(logging.NullHandler()); null.propagate = False
    m = ref_import._mod
    m("timm"); m("timm.models")
    m("timm.models.layers", trunc_normal_=nn.init.trunc_normal_, DropPath=lambda p=0.0: nn.Identity())      # STUB
    sys.modules["mmcv.runner"]._load_checkpoint = lambda *a, **k: {}                                            # STUB
    sys.modules["mmcv.cnn"].constant_init = lambda *a, **k: None                                                # STUB
    sys.modules["mmcv.cnn"].trunc_normal_init = lambda *a, **k: None                                            # STUB
    m("mmdet.utils", get_root_logger=lambda *a, **k: null)                                                      # STUB
    m("mmdet.models.builder", BACKBONES=ref_import._Registry())                                                 # STUB
    return importlib.import_module("refbackbones.internimage")


def main():
    ref = reference_internimage()
    for ci, (name, kw) in enumerate(CASES.items()):
        torch.manual_seed(20 + ci)
        model = ref.InternImage(**kw).double()
        randomise(model, 30 + ci)
        g = torch.Generator().manual_seed(40 + ci)
        x = torch.randn(IMAGE, generator=g).float().double().requires_grad_(True)
        outs = model(x)
        cot = [torch.randn(o.shape, generator=g).float().double() for o in outs]
        params = sorted(model.named_parameters())
        grads = torch.autograd.grad(sum((o * c).sum() for o, c in zip(outs, cot)), [x] + [p for _, p in params])
        data = {"input": x.detach().numpy().astype(np.float32), "grad_input": grads[0].numpy()}
        for i, (o, c) in enumerate(zip(outs, cot)):
            data[f"out.{i}"], data[f"cot.{i}"] = o.detach().numpy(), c.numpy().astype(np.float32)
        for (k, p), gr in zip(params, grads[1:]):
            data[f"w.{k}"], data[f"g.{k}"] = p.detach().numpy().astype(np.float32), gr.numpy()
        np.savez_compressed(HERE / f"internimage_{name}.npz", **data)
        keys = sorted((k, list(v.shape)) for k, v in model.state_dict().items())
        (HERE / f"internimage_{name}.json").write_text(json.dumps(dict(kwargs=kw, image=list(IMAGE), state_dict=keys), indent=1) + "\n")
        size = (HERE / f"internimage_{name}.npz").stat().st_size
        print(name, sum(p.numel() for _, p in params), "parameters,", size, "bytes")
        assert size < (1 << 20)


if __name__ == "__main__":
    main()
