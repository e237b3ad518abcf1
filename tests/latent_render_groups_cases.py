"""The settings of the LatentRendering group goldens (tests/golden/make_latent_render_groups_golden.py), shared by
tests/test_latent_render_groups_cpu.py and tests/test_latent_render_groups_gpu.py."""

# name: embed_dims, pred_height, reduction, num_pred_fcs, grid_num, grid_step, act, H, W
GOLDEN_CASES = {
    "c64_z1_r16_fc2_exp": (64, 1, 16, 2, 128, 0.5, "exp", 9, 9),
    "c256_z4_r16_sigmoid": (256, 4, 16, 0, 256, 0.5, "sigmoid", 10, 16),
    "c192_z3_r16_sigmoid": (192, 3, 16, 0, 256, 1.0, "sigmoid", 7, 11),
    "c256_z32_r8_exp": (256, 32, 8, 0, 256, 1.0, "exp", 6, 6),
    "c256_z16_r4_sigmoid": (256, 16, 4, 0, 64, 1.0, "sigmoid", 8, 5),
}


def build(name):
    from vidar_amd.plugin.modules.ray_operations.latent_rendering import LatentRendering
    C, Z, red, fcs, G, step, act, H, W = GOLDEN_CASES[name]
    return LatentRendering(embed_dims=C, pred_height=Z, num_pred_fcs=fcs, grid_step=step, grid_num=G, reduction=red, act=act)
