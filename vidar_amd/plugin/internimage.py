"""InternImage image backbone (registry name `InternImage`; bevformer/backbones/internimage.py:527-702 of the
reference) on the DCNv3 operator of csrc/dcnv3.hip.

Same constructor arguments and the same module tree -- `patch_embed.{conv1,norm1,conv2,norm2}`,
`levels.<i>.blocks.<j>.{norm1,dcn,norm2,mlp.fc1,mlp.fc2[,gamma1,gamma2,res_post_norm1,res_post_norm2]}`,
`levels.<i>.{norm,post_norms,downsample.{conv,norm}}` -- so a released InternImage checkpoint loads strictly.
Activations are channel-last between the stem and the outputs; `forward` returns the NCHW maps of `out_indices`."""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.utils.checkpoint as cp

from . import ops_dcnv3 as opsm
from .ops_dcnv3 import build_act_layer, build_norm_layer
from .registry import BACKBONES


class DropPath(nn.Module):
    """stochastic depth: drops the whole residual branch of a sample with probability p (training only)"""

    def __init__(self, drop_prob=0.0):
        super().__init__()
        self.drop_prob = float(drop_prob)

    def forward(self, x):
        if self.drop_prob == 0.0 or not self.training:
            return x
        keep = 1.0 - self.drop_prob
        m = x.new_empty((x.shape[0],) + (1,) * (x.dim() - 1)).bernoulli_(keep)
        return x * m / keep


def trunc_normal_(tensor, mean=0.0, std=1.0, a=-2.0, b=2.0):
    return nn.init.trunc_normal_(tensor, mean=mean, std=std, a=a, b=b)


class StemLayer(nn.Module):
    """two stride-2 3x3 convolutions: NCHW image -> channel-last map at 1/4 resolution"""

    def __init__(self, in_chans=3, out_chans=96, act_layer="GELU", norm_layer="BN"):
        super().__init__()
        self.conv1 = nn.Conv2d(in_chans, out_chans // 2, kernel_size=3, stride=2, padding=1)
        self.norm1 = build_norm_layer(out_chans // 2, norm_layer, "channels_first", "channels_first")
        self.act = build_act_layer(act_layer)
        self.conv2 = nn.Conv2d(out_chans // 2, out_chans, kernel_size=3, stride=2, padding=1)
        self.norm2 = build_norm_layer(out_chans, norm_layer, "channels_first", "channels_last")

    def forward(self, x):
        return self.norm2(self.conv2(self.act(self.norm1(self.conv1(x)))))


class DownsampleLayer(nn.Module):
    def __init__(self, channels, norm_layer="LN"):
        super().__init__()
        self.conv = nn.Conv2d(channels, 2 * channels, kernel_size=3, stride=2, padding=1, bias=False)
        self.norm = build_norm_layer(2 * channels, norm_layer, "channels_first", "channels_last")

    def forward(self, x):
        return self.norm(self.conv(x.permute(0, 3, 1, 2)))


class MLPLayer(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer="GELU", drop=0.0):
        super().__init__()
        self.fc1 = nn.Linear(in_features, hidden_features or in_features)
        self.act = build_act_layer(act_layer)
        self.fc2 = nn.Linear(hidden_features or in_features, out_features or in_features)
        self.drop = nn.Dropout(drop)

    def forward(self, x):
        return self.drop(self.fc2(self.drop(self.act(self.fc1(x)))))


class InternImageLayer(nn.Module):
    """x += branch(dcn);  x += branch(mlp) with the norm before (default), after (`post_norm`) or on both sides
    (`res_post_norm`) of the operator, optionally scaled per channel (`layer_scale`)."""

    def __init__(self, core_op, channels, groups, mlp_ratio=4.0, drop=0.0, drop_path=0.0, act_layer="GELU",
                 norm_layer="LN", post_norm=False, layer_scale=None, offset_scale=1.0, with_cp=False,
                 dw_kernel_size=None, res_post_norm=False, center_feature_scale=False):
        super().__init__()
        self.channels, self.groups, self.mlp_ratio, self.with_cp = channels, groups, mlp_ratio, with_cp
        self.norm1 = build_norm_layer(channels, "LN")
        self.post_norm = post_norm
        self.dcn = core_op(channels=channels, kernel_size=3, stride=1, pad=1, dilation=1, group=groups,
                           offset_scale=offset_scale, act_layer=act_layer, norm_layer=norm_layer,
                           dw_kernel_size=dw_kernel_size, center_feature_scale=center_feature_scale)
        self.drop_path = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self.norm2 = build_norm_layer(channels, "LN")
        self.mlp = MLPLayer(channels, int(channels * mlp_ratio), act_layer=act_layer, drop=drop)
        self.layer_scale = layer_scale is not None
        if self.layer_scale:
            self.gamma1 = nn.Parameter(layer_scale * torch.ones(channels))
            self.gamma2 = nn.Parameter(layer_scale * torch.ones(channels))
        self.res_post_norm = res_post_norm
        if res_post_norm:
            self.res_post_norm1 = build_norm_layer(channels, "LN")
            self.res_post_norm2 = build_norm_layer(channels, "LN")

    def _branches(self, x):
        steps = ((self.norm1, self.dcn, getattr(self, "res_post_norm1", None), getattr(self, "gamma1", None)),
                 (self.norm2, self.mlp, getattr(self, "res_post_norm2", None), getattr(self, "gamma2", None)))
        for norm, op, res_norm, gamma in steps:
            if self.post_norm:
                y = norm(op(x))
            elif self.res_post_norm and not self.layer_scale:
                y = res_norm(op(norm(x)))
            else:
                y = op(norm(x))
            if gamma is not None:
                y = gamma * y
            x = x + self.drop_path(y)
        return x

    def forward(self, x):
        if self.with_cp and x.requires_grad:
            return cp.checkpoint(self._branches, x, use_reentrant=False)
        return self._branches(x)


class InternImageBlock(nn.Module):
    """one resolution level: `depth` layers, the level's norm, then (except at the last level) the downsampling"""

    def __init__(self, core_op, channels, depth, groups, downsample=True, mlp_ratio=4.0, drop=0.0, drop_path=0.0,
                 act_layer="GELU", norm_layer="LN", post_norm=False, offset_scale=1.0, layer_scale=None, with_cp=False,
                 dw_kernel_size=None, post_norm_block_ids=None, res_post_norm=False, center_feature_scale=False):
        super().__init__()
        self.channels, self.depth, self.post_norm = channels, depth, post_norm
        self.center_feature_scale = center_feature_scale
        self.blocks = nn.ModuleList([
            InternImageLayer(core_op=core_op, channels=channels, groups=groups, mlp_ratio=mlp_ratio, drop=drop,
                             drop_path=drop_path[i] if isinstance(drop_path, list) else drop_path,
                             act_layer=act_layer, norm_layer=norm_layer, post_norm=post_norm, layer_scale=layer_scale,
                             offset_scale=offset_scale, with_cp=with_cp, dw_kernel_size=dw_kernel_size,
                             res_post_norm=res_post_norm, center_feature_scale=center_feature_scale)
            for i in range(depth)])
        if not post_norm or center_feature_scale:
            self.norm = build_norm_layer(channels, "LN")
        self.post_norm_block_ids = post_norm_block_ids
        if post_norm_block_ids is not None:
            self.post_norms = nn.ModuleList([build_norm_layer(channels, "LN", eps=1e-6) for _ in post_norm_block_ids])
        self.downsample = DownsampleLayer(channels, norm_layer) if downsample else None

    def forward(self, x, return_wo_downsample=False):
        for i, blk in enumerate(self.blocks):
            x = blk(x)
            if self.post_norm_block_ids is not None and i in self.post_norm_block_ids:
                x = self.post_norms[self.post_norm_block_ids.index(i)](x)
        if not self.post_norm or self.center_feature_scale:
            x = self.norm(x)
        full = x
        if self.downsample is not None:
            x = self.downsample(x)
        return (x, full) if return_wo_downsample else x


@BACKBONES.register_module()
class InternImage(nn.Module):
    """core_op: 'DCNv3' (HIP kernels) or 'DCNv3_pytorch' (grid_sample; any device)."""

    def __init__(self, core_op="DCNv3", channels=64, depths=[3, 4, 18, 5], groups=[3, 6, 12, 24], mlp_ratio=4.0,
                 drop_rate=0.0, drop_path_rate=0.2, drop_path_type="linear", act_layer="GELU", norm_layer="LN",
                 layer_scale=None, offset_scale=1.0, post_norm=False, with_cp=False, dw_kernel_size=None,
                 level2_post_norm=False, level2_post_norm_block_ids=None, res_post_norm=False,
                 center_feature_scale=False, out_indices=(0, 1, 2, 3), init_cfg=None, **kwargs):
        super().__init__()
        if core_op not in ("DCNv3", "DCNv3_pytorch"):
            raise ValueError(f"InternImage: core_op must be 'DCNv3' or 'DCNv3_pytorch', got {core_op!r}")
        self.core_op = core_op
        self.num_levels = self.num_layers = len(depths)
        self.depths, self.channels = depths, channels
        self.num_features = int(channels * 2 ** (self.num_levels - 1))
        self.post_norm, self.mlp_ratio = post_norm, mlp_ratio
        self.init_cfg, self.out_indices = init_cfg, out_indices
        self.level2_post_norm_block_ids = level2_post_norm_block_ids
        self.patch_embed = StemLayer(in_chans=3, out_chans=channels, act_layer=act_layer, norm_layer=norm_layer)
        self.pos_drop = nn.Dropout(p=drop_rate)
        total = sum(depths)
        if drop_path_type == "uniform":
            dpr = [float(drop_path_rate)] * total
        else:
            dpr = [v.item() for v in torch.linspace(0, drop_path_rate, total)]
        self.levels = nn.ModuleList()
        for i in range(self.num_levels):
            self.levels.append(InternImageBlock(
                core_op=getattr(opsm, core_op), channels=int(channels * 2 ** i), depth=depths[i], groups=groups[i],
                mlp_ratio=mlp_ratio, drop=drop_rate, drop_path=dpr[sum(depths[:i]):sum(depths[:i + 1])],
                act_layer=act_layer, norm_layer=norm_layer, post_norm=post_norm, downsample=i < self.num_levels - 1,
                layer_scale=layer_scale, offset_scale=offset_scale, with_cp=with_cp, dw_kernel_size=dw_kernel_size,
                post_norm_block_ids=level2_post_norm_block_ids if (level2_post_norm and i == 2) else None,
                res_post_norm=res_post_norm, center_feature_scale=center_feature_scale))
        self.apply(self._init_weights)
        self.apply(self._init_deform_weights)

    def _init_weights(self, m):
        if isinstance(m, nn.Linear):
            trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.zeros_(m.bias)
        elif isinstance(m, nn.LayerNorm):
            nn.init.zeros_(m.bias)
            nn.init.ones_(m.weight)

    def _init_deform_weights(self, m):
        if isinstance(m, getattr(opsm, self.core_op)):
            m._reset_parameters()

    def init_weights(self):
        """`init_cfg=None`: training from scratch (truncated-normal Linear weights, unit LayerNorms); otherwise
        `init_cfg['checkpoint']` is loaded non-strictly after its `backbone.` / `module.` prefixes are stripped
        (internimage.py:655-678).  -> (missing_keys, unexpected_keys) of the load, or None."""
        if self.init_cfg is None:
            for m in self.modules():
                if isinstance(m, nn.Linear):
                    trunc_normal_(m.weight, mean=0.0, std=0.02, a=-2.0, b=2.0)
                    if m.bias is not None:
                        nn.init.zeros_(m.bias)
                elif isinstance(m, nn.LayerNorm):
                    nn.init.ones_(m.weight)
                    nn.init.zeros_(m.bias)
            return None
        if "checkpoint" not in self.init_cfg:
            raise ValueError(f"{type(self).__name__}: init_cfg must name a `checkpoint`")
        from ..checkpoint import backbone_state_dict
        res = self.load_state_dict(backbone_state_dict(self.init_cfg["checkpoint"]), strict=False)
        return list(res.missing_keys), list(res.unexpected_keys)

    def forward(self, x):
        x = self.pos_drop(self.patch_embed(x))
        outs = []
        for i, level in enumerate(self.levels):
            x, full = level(x, return_wo_downsample=True)
            if i in self.out_indices:
                outs.append(full.permute(0, 3, 1, 2).contiguous())
        return outs
