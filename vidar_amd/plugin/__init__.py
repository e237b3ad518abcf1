"""Host-side mirror of the reference's `projects/mmdet3d_plugin` registry surface for the hot path
(same registered type names, constructor kwargs and parameter names).  Importing this package
registers every module, like `importlib.import_module('projects.mmdet3d_plugin')` does in the
reference (tools/train.py:113-137)."""
from . import bricks, backbones, internimage, core_bbox, det_losses  # noqa: F401
from .modules import (temporal_self_attention, spatial_cross_attention, encoder, transformer,  # noqa: F401
                      vidar_decoder, vidar_transformer, decoder)
from .modules.ray_operations import latent_rendering  # noqa: F401
from .dense_heads import vidar_bevformer_head, vidar_head_base, vidar_head_v1, bevformer_head  # noqa: F401
from .detectors import vidar, bevformer  # noqa: F401
from .registry import *  # noqa: F401,F403
from .config import Config  # noqa: F401
