"""Detection decoder of the BEVFormer fine-tune path: `inverse_sigmoid` and `DetectionTransformerDecoder` restate
projects/mmdet3d_plugin/bevformer/modules/decoder.py:34-129 (iterative reference-point refinement through the head's
reg_branches, intermediate outputs stacked).  Its cross attention is `CustomMSDeformableAttention`
(modules/vidar_decoder.py), i.e. the fused HIP MSDA op at L = 1, P = 4 over the BEV map.

Third party, recalled, unpinned (mmcv is not vendored in the reference):
  * `DetrTransformerDecoderLayer` -- mmcv.cnn.bricks.transformer: a BaseTransformerLayer with
    (self_attn, norm, cross_attn, norm, ffn, norm); forward contract of BaseTransformerLayer.forward (self attention takes
    key = value = query and query_pos as key_pos, cross attention takes the caller's key / value / key_pos);
  * `MultiheadAttention` -- mmcv's wrapper of nn.MultiheadAttention: identity + dropout_layer(proj_drop(attn(q + query_pos,
    k + key_pos, v))) with key = query / value = key / key_pos = query_pos defaults, sequence-first unless batch_first;
    parameter names attn.in_proj_weight, attn.in_proj_bias, attn.out_proj.{weight,bias}."""
from __future__ import annotations

import torch
import torch.nn as nn

from ..registry import ATTENTION, TRANSFORMER_LAYER, TRANSFORMER_LAYER_SEQUENCE
from .custom_base_transformer_layer import MyCustomBaseTransformerLayer
from .encoder import TransformerLayerSequence


def inverse_sigmoid(x, eps=1e-5):
    """decoder.py:34-49"""
    x = x.clamp(min=0, max=1)
    x1 = x.clamp(min=eps)
    x2 = (1 - x).clamp(min=eps)
    return torch.log(x1 / x2)


@ATTENTION.register_module()
class MultiheadAttention(nn.Module):
    def __init__(self, embed_dims, num_heads, attn_drop=0., proj_drop=0., dropout_layer=dict(type="Dropout", drop_prob=0.),
                 init_cfg=None, batch_first=False, dropout=None, **kwargs):
        super().__init__()
        if dropout is not None:                      # deprecated spelling: sets attn_drop and the residual dropout
            attn_drop = dropout
            dropout_layer = dict(type="Dropout", drop_prob=dropout)
        self.embed_dims = embed_dims
        self.num_heads = num_heads
        self.batch_first = batch_first
        self.attn = nn.MultiheadAttention(embed_dims, num_heads, attn_drop, **kwargs)
        self.proj_drop = nn.Dropout(proj_drop)
        if dropout_layer and dropout_layer.get("type", "Dropout") != "Dropout":
            raise NotImplementedError(f"MultiheadAttention dropout_layer type {dropout_layer.get('type')!r}")
        self.dropout_layer = nn.Dropout(dropout_layer.get("drop_prob", 0.)) if dropout_layer else nn.Identity()

    def forward(self, query, key=None, value=None, identity=None, query_pos=None, key_pos=None, attn_mask=None,
                key_padding_mask=None, **kwargs):
        if key is None:
            key = query
        if value is None:
            value = key
        if identity is None:
            identity = query
        if key_pos is None and query_pos is not None and query_pos.shape == key.shape:
            key_pos = query_pos
        if query_pos is not None:
            query = query + query_pos
        if key_pos is not None:
            key = key + key_pos
        if self.batch_first:
            query, key, value = (t.transpose(0, 1) for t in (query, key, value))
        out = self.attn(query=query, key=key, value=value, attn_mask=attn_mask, key_padding_mask=key_padding_mask)[0]
        if self.batch_first:
            out = out.transpose(0, 1)
        return identity + self.dropout_layer(self.proj_drop(out))


@TRANSFORMER_LAYER.register_module()
class DetrTransformerDecoderLayer(MyCustomBaseTransformerLayer):
    def __init__(self, attn_cfgs, feedforward_channels, ffn_dropout=0.0, operation_order=None,
                 act_cfg=dict(type="ReLU", inplace=True), norm_cfg=dict(type="LN"), ffn_num_fcs=2, **kwargs):
        kwargs.setdefault("batch_first", False)       # mmcv's BaseTransformerLayer default (the custom base says True)
        super().__init__(attn_cfgs=attn_cfgs, feedforward_channels=feedforward_channels, ffn_dropout=ffn_dropout,
                         operation_order=operation_order, act_cfg=act_cfg, norm_cfg=norm_cfg, ffn_num_fcs=ffn_num_fcs,
                         **kwargs)
        assert len(operation_order) == 6
        assert set(operation_order) == {"self_attn", "norm", "cross_attn", "ffn"}

    def forward(self, query, key=None, value=None, query_pos=None, key_pos=None, attn_masks=None,
                query_key_padding_mask=None, key_padding_mask=None, **kwargs):
        norm_index = attn_index = ffn_index = 0
        identity = query
        if attn_masks is None:
            attn_masks = [None] * self.num_attn
        for layer in self.operation_order:
            if layer == "self_attn":
                query = self.attentions[attn_index](
                    query, query, query, identity if self.pre_norm else None, query_pos=query_pos, key_pos=query_pos,
                    attn_mask=attn_masks[attn_index], key_padding_mask=query_key_padding_mask, **kwargs)
                attn_index += 1
                identity = query
            elif layer == "norm":
                query = self.norms[norm_index](query)
                norm_index += 1
            elif layer == "cross_attn":
                query = self.attentions[attn_index](
                    query, key, value, identity if self.pre_norm else None, query_pos=query_pos, key_pos=key_pos,
                    attn_mask=attn_masks[attn_index], key_padding_mask=key_padding_mask, **kwargs)
                attn_index += 1
                identity = query
            elif layer == "ffn":
                query = self.ffns[ffn_index](query, identity if self.pre_norm else None)
                ffn_index += 1
        return query


@TRANSFORMER_LAYER_SEQUENCE.register_module()
class DetectionTransformerDecoder(TransformerLayerSequence):
    def __init__(self, *args, return_intermediate=False, **kwargs):
        super().__init__(*args, **kwargs)
        self.return_intermediate = return_intermediate
        self.fp16_enabled = False

    def forward(self, query, *args, reference_points=None, reg_branches=None, key_padding_mask=None, **kwargs):
        """query [num_query, bs, C]; reference_points [bs, num_query, 3] in [0, 1] (decoder.py:66-129)"""
        output = query
        intermediate, intermediate_reference_points = [], []
        for lid, layer in enumerate(self.layers):
            reference_points_input = reference_points[..., :2].unsqueeze(2)         # [bs, num_query, 1 level, 2]
            output = layer(output, *args, reference_points=reference_points_input, key_padding_mask=key_padding_mask,
                           **kwargs)
            output = output.permute(1, 0, 2)
            if reg_branches is not None:
                tmp = reg_branches[lid](output)
                assert reference_points.shape[-1] == 3
                new_reference_points = torch.zeros_like(reference_points)
                new_reference_points[..., :2] = tmp[..., :2] + inverse_sigmoid(reference_points[..., :2])
                new_reference_points[..., 2:3] = tmp[..., 4:5] + inverse_sigmoid(reference_points[..., 2:3])
                reference_points = new_reference_points.sigmoid().detach()
            output = output.permute(1, 0, 2)
            if self.return_intermediate:
                intermediate.append(output)
                intermediate_reference_points.append(reference_points)
        if self.return_intermediate:
            return torch.stack(intermediate), torch.stack(intermediate_reference_points)
        return output, reference_points
