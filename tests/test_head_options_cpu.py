"""CPU: the prediction head takes the reference's constructor arguments -- its own default ray_grid_num (1026), any
other waypoint count, and use_dist_loss -- and the library carries what they need: the C ABI exports the distance-loss
pair and every ray-march kernel of the code object (streamed `*_any_kernel` forms and `ray_dist_*` included) meets the
resource limits of tests/test_kernel_resources_cpu.py, which enumerates the whole code object and so covers them too;
the rows are named here so that a build without them fails."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest

import vidar_amd.plugin as P
from vidar_amd.configs import VARIANTS, get_config, model_config

ROOT = Path(__file__).resolve().parents[1]
V1_ONLY = ("history_queue_length", "pred_history_frame_num", "pred_future_frame_num", "per_frame_loss_weight")


def head_cfg(cls="ViDARHeadV1", **over):
    cfg = dict(model_config("vidar_1_8_nusc_1future", bev_h=24, bev_w=24)["future_pred_head"])
    cfg.pop("ray_grid_num"); cfg.pop("use_dist_loss")
    cfg["type"] = cls
    if cls != "ViDARHeadV1":
        for k in V1_ONLY:
            cfg.pop(k)
    cfg.update(over)
    return cfg


@pytest.mark.parametrize("cls", ["ViDARHeadBase", "ViDARHeadV1"])
def test_head_builds_with_the_reference_defaults(cls):
    h = P.HEADS.build(head_cfg(cls))                      # no ray_grid_num in the dict
    assert h.ray_grid_num == 1026 and h.ray_grid_step == 1.0
    assert h.use_ce_loss and h.use_dense_loss and not h.use_dist_loss


@pytest.mark.parametrize("cls", ["ViDARHeadBase", "ViDARHeadV1"])
@pytest.mark.parametrize("over", [dict(ray_grid_num=1026), dict(ray_grid_num=37), dict(ray_grid_num=2048, ray_grid_step=0.25),
                                  dict(use_dist_loss=True), dict(ray_grid_num=1024, ray_grid_step=0.5, use_dist_loss=True),
                                  dict(use_dist_loss=True, use_ce_loss=False, use_dense_loss=False)])
def test_head_accepts_ray_grid_num_and_dist_loss(cls, over):
    h = P.HEADS.build(head_cfg(cls, **over))
    for k, v in over.items():
        assert getattr(h, k) == v


def test_a_head_needs_one_loss():
    with pytest.raises(AssertionError):
        P.HEADS.build(head_cfg("ViDARHeadBase", use_ce_loss=False, use_dense_loss=False))


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_named_configs_still_build_with_their_512(name):
    from vidar_amd import train as T
    model = T.build_model(get_config(name, bev_h=24, bev_w=24))
    assert model.future_pred_head.ray_grid_num == 512 and not model.future_pred_head.use_dist_loss


def test_abi_exports_the_distance_pair():
    from vidar_amd import build
    from vidar_amd._lib import declare
    lib = declare(ctypes.CDLL(str(build.build(verbose=False))))
    for n in ("vidar_ray_dist_fwd_f32", "vidar_ray_dist_bwd_f32", "vidar_ray_max_k", "vidar_ray_force_streamed"):
        assert hasattr(lib, n), n
    assert lib.vidar_ray_max_k() >= 2050
    # out-of-range K is still a bad argument (checked before anything touches a device)
    null = ctypes.c_void_p(0)
    for K in (0, -1, lib.vidar_ray_max_k() + 1):
        rc = lib.vidar_ray_argmax_f32(null, null, null, null, null, null, 1, 0, 16, 200, 200, K, 1.0, null)
        assert rc == -22, (K, rc)
    assert lib.vidar_ray_argmax_f32(null, null, null, null, null, null, 1, 0, 16, 200, 200, 1026, 1.0, null) == 0


def test_new_ray_kernels_meet_the_resource_limits():
    from vidar_amd import build
    sys.path.insert(0, str(ROOT / "tools"))
    import kernel_resources
    by = {r["kernel"]: r for r in kernel_resources.table(build.build(verbose=False))}
    for name in ("ray_ce_fwd_any_kernel", "ray_ce_bwd_any_kernel", "ray_gumbel_fwd_any_kernel",
                 "ray_gumbel_bwd_any_kernel", "ray_argmax_any_kernel", "ray_dist_fwd_kernel", "ray_dist_bwd_kernel"):
        r = by[name]
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and not r["dyn_stack"] and r["agpr"] == 0, r
        assert r["vgpr"] <= 128 and r["waves_per_simd"] >= 4, r
