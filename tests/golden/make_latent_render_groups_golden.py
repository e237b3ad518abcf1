"""Golden vectors for LatentRendering at other pred_height / reduction / embed_dims than the released 16 / 16 / 256,
from the REFERENCE module itself (imported with mmcv stubbed, see ref_import.py): the grouping of the LoRA channels by
height bin (its view(bs, pred_height, -1, ...)).  Run in the build container:
    python tests/golden/make_latent_render_groups_golden.py"""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(Path(__file__).parent))
import ref_import  # noqa: E402

# name: embed_dims, pred_height, reduction, num_pred_fcs, grid_num, grid_step, act, H, W
CASES = {
    "c64_z1_r16_fc2_exp": (64, 1, 16, 2, 128, 0.5, "exp", 9, 9),            # the constructor defaults, narrow; J = 4
    "c256_z4_r16_sigmoid": (256, 4, 16, 0, 256, 0.5, "sigmoid", 10, 16),    # J = 4
    "c192_z3_r16_sigmoid": (192, 3, 16, 0, 256, 1.0, "sigmoid", 7, 11),     # Z no multiple of 4, A = 12
    "c256_z32_r8_exp": (256, 32, 8, 0, 256, 1.0, "exp", 6, 6),              # Z = A = 32
    "c256_z16_r4_sigmoid": (256, 16, 4, 0, 64, 1.0, "sigmoid", 8, 5),       # A = 64, J = 4
}

if __name__ == "__main__":
    m = ref_import.latent_rendering_module()
    for name, (C, Z, red, fcs, G, step, act, H, W) in CASES.items():
        torch.manual_seed(0)
        mod = m.LatentRendering(embed_dims=C, pred_height=Z, num_pred_fcs=fcs, grid_step=step, grid_num=G,
                                reduction=red, act=act)
        embed = torch.randn(1, H, W, C, requires_grad=True)
        out = mod(embed)
        gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(1))
        params = dict(mod.named_parameters())
        grads = torch.autograd.grad((out * gout).sum(), [embed, *params.values()])
        np.savez_compressed(Path(__file__).parent / f"latent_render_groups_{name}.npz",
                            embed=embed.detach().numpy(), out=out.detach().numpy(), gout=gout.numpy(),
                            grad_embed=grads[0].numpy(),
                            **{"p_" + k: v.detach().numpy() for k, v in params.items()},
                            **{"g_" + k: g.numpy() for k, g in zip(params, grads[1:])})
        print(name, tuple(out.shape), float(out.abs().mean()), {k: tuple(v.shape) for k, v in params.items()})
