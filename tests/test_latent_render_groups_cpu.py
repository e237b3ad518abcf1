"""CPU: LatentRendering takes any pred_height / reduction / embed_dims the reference's view(bs, pred_height, -1, ...)
takes -- construction, parameter shapes (the reference's names, so its checkpoints load strictly), the config switch and
the C ABI of the grouped stage 2.  The arithmetic is checked on the GPU (tests/test_latent_render_groups_gpu.py)."""
import re
from pathlib import Path

import pytest

from latent_render_groups_cases import GOLDEN_CASES, build

ROOT = Path(__file__).resolve().parents[1]

def test_constructor_defaults_build():
    from vidar_amd.plugin.modules.ray_operations.latent_rendering import LatentRendering
    mod = LatentRendering()                       # the reference's defaults: pred_height 1, reduction 16, 2 fcs, exp
    assert mod.pred_height == 1 and mod.grid_num == 128 and mod.act == "exp"
    assert tuple(mod.unsup_raymarching_head[6].weight.shape) == (1, 256)
    assert tuple(mod.lora_a.weight.shape) == (16, 256) and tuple(mod.lora_b.weight.shape) == (256, 16)


@pytest.mark.parametrize("name", list(GOLDEN_CASES))
def test_parameter_shapes(name):
    C, Z, red, fcs = GOLDEN_CASES[name][:4]
    shapes = {k: tuple(v.shape) for k, v in build(name).named_parameters()}
    want = {f"unsup_raymarching_head.{3 * fcs}.weight": (Z, C), f"unsup_raymarching_head.{3 * fcs}.bias": (Z,),
            "lora_a.weight": (C // red, C), "lora_a.bias": (C // red,), "lora_b.weight": (C, C // red), "lora_b.bias": (C,)}
    for i in range(fcs):
        want.update({f"unsup_raymarching_head.{3 * i}.weight": (C, C), f"unsup_raymarching_head.{3 * i}.bias": (C,),
                     f"unsup_raymarching_head.{3 * i + 1}.weight": (C,), f"unsup_raymarching_head.{3 * i + 1}.bias": (C,)})
    assert shapes == want


@pytest.mark.parametrize("kw", [dict(embed_dims=256, pred_height=3), dict(pred_height=32, reduction=16)])
def test_indivisible_settings_raise_value_error(kw):
    from vidar_amd.plugin.modules.ray_operations.latent_rendering import LatentRendering
    with pytest.raises(ValueError, match="multiples of pred_height"):
        LatentRendering(**kw)


def test_get_config_latent_render_switch():
    from vidar_amd import train as T
    from vidar_amd.configs import get_config
    base = get_config("vidar_1_8_nusc_1future", bev_h=24, bev_w=24)
    assert base == get_config("vidar_1_8_nusc_1future", bev_h=24, bev_w=24, latent_render=None)
    lr = base["model"]["pts_bbox_head"]["transformer"]["encoder"]["transformerlayers"]["latent_render"]
    assert (lr["pred_height"], lr["reduction"]) == (16, 16)
    model = T.build_model(get_config("vidar_1_8_nusc_1future", bev_h=24, bev_w=24, latent_render=dict(pred_height=4)))
    heads = {n: tuple(p.shape) for n, p in model.named_parameters() if n.endswith("unsup_raymarching_head.0.weight")}
    assert len(heads) == 1 and ".layers.2." in next(iter(heads)) and set(heads.values()) == {(4, 256)}
    default = T.build_model(base)
    assert {tuple(p.shape) for n, p in default.named_parameters() if n.endswith("unsup_raymarching_head.0.weight")} == {(16, 256)}
    # the future decoder's layers carry the same entry
    fut = get_config("vidar_1_8_nusc_3future", latent_render=dict(pred_height=4, reduction=8))
    dec = fut["model"]["future_pred_head"]["transformer"]["decoder"]["transformerlayers"]["latent_render"]
    enc = fut["model"]["pts_bbox_head"]["transformer"]["encoder"]["transformerlayers"]["latent_render"]
    assert dec == enc and (dec["pred_height"], dec["reduction"], dec["grid_step"]) == (4, 8, 0.5)


def test_grouped_entries_are_declared_in_header_and_table():
    from vidar_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "vidar_hip.h").read_text(), flags=re.S)
    for name, kinds in (("vidar_latent_render_gather_grouped_fwd_f32", "i 4p 6i 2f p"),
                        ("vidar_latent_render_gather_grouped_bwd_f32", "i 7p 6i 2f p z p")):
        assert _lib._ABI[name] == kinds
        assert re.search(rf"\bint\s+{name}\s*\(", header), name
        assert hasattr(_lib.lib(), name)
