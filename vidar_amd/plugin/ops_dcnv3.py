"""DCNv3, the core operator of InternImage: Python surface of csrc/dcnv3.hip.

Mirrors bevformer/backbones/ops_dcnv3 of the reference: `DCNv3Function` (functions/dcnv3_func.py:18-108, same 15
arguments), `dcnv3_core_pytorch` (:147-190, the pure-torch form) and the modules `DCNv3` / `DCNv3_pytorch`
(modules/dcnv3.py:95-345) with the reference's constructor arguments and parameter names (`dw_conv.0`, `dw_conv.1.1`,
`offset`, `mask`, `input_proj`, `output_proj`, `center_feature_scale_proj_{weight,bias}`), so released InternImage
checkpoints load key for key.  `DCNv3` runs the HIP kernels and has no CPU path; `DCNv3_pytorch` is `F.grid_sample`
arithmetic on any device and is what the kernels are compared with."""
from __future__ import annotations

import warnings

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from ..third_lib import dcnv3 as _ext


class DCNv3Function(Function):
    """output = DCNv3Function.apply(input, offset, mask, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w,
    dilation_h, dilation_w, group, group_channels, offset_scale, im2col_step).  The kernels are fp32: fp16 / bf16
    operands are computed in fp32 and every result comes back in its operand's dtype."""

    @staticmethod
    def forward(ctx, input, offset, mask, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w,
                group, group_channels, offset_scale, im2col_step):
        ctx.geometry = (kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, group,
                        group_channels, offset_scale)
        ctx.im2col_step = im2col_step
        if not (input.is_cuda and offset.is_cuda and mask.is_cuda):
            raise RuntimeError("DCNv3Function runs on the GPU only (use DCNv3_pytorch / dcnv3_core_pytorch on the host)")
        ops = tuple(_fp32(t) for t in (input, offset, mask))
        ctx.dtypes = (input.dtype, offset.dtype, mask.dtype)
        out = _ext.dcnv3_forward(*ops, *ctx.geometry, im2col_step)
        ctx.save_for_backward(input, offset, mask)
        return out.to(input.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        ops = tuple(_fp32(t) for t in ctx.saved_tensors)
        grads = _ext.dcnv3_backward(*ops, *ctx.geometry, _fp32(grad_output), ctx.im2col_step)
        return tuple(g.to(d) for g, d in zip(grads, ctx.dtypes)) + (None,) * 12


def _fp32(t):
    if t.dtype in (torch.float16, torch.bfloat16):
        t = t.float()
    return t.contiguous()


def dcnv3_core_pytorch(input, offset, mask, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h,
                       dilation_w, group, group_channels, offset_scale):
    """The DCNv3 sum on `F.grid_sample` (bilinear, zero padding), differentiable in input, offset and mask.

    Point p = i_w * kernel_h + j_h of output pixel (ho, wo) samples the UNPADDED input at pixel
        x = wo*stride_w - pad_w + (i_w*dilation_w + offset_w) * offset_scale + c_w * (1 - offset_scale)
    with c_w = (dilation_w*(kernel_w-1)) // 2 (y alike): the kernels' location.  Zero padding of grid_sample is the
    kernels' rule (a corner outside the image adds nothing), so no padded copy of the input is made."""
    N, H, W, C = input.shape
    _, Ho, Wo, _ = offset.shape
    P = kernel_h * kernel_w
    dt, dev = input.dtype, input.device
    ar = lambda n: torch.arange(n, dtype=dt, device=dev)
    cw, ch = (dilation_w * (kernel_w - 1)) // 2, (dilation_h * (kernel_h - 1)) // 2
    base_x = (ar(Wo) * stride_w - pad_w + cw - cw * offset_scale).view(1, 1, Wo, 1, 1)
    base_y = (ar(Ho) * stride_h - pad_h + ch - ch * offset_scale).view(1, Ho, 1, 1, 1)
    tap_x = (ar(kernel_w) * dilation_w).view(kernel_w, 1).expand(kernel_w, kernel_h).reshape(1, 1, 1, 1, P)
    tap_y = (ar(kernel_h) * dilation_h).view(1, kernel_h).expand(kernel_w, kernel_h).reshape(1, 1, 1, 1, P)
    off = offset.reshape(N, Ho, Wo, group, P, 2)
    x = base_x + (tap_x + off[..., 0]) * offset_scale                 # [N,Ho,Wo,G,P] pixels
    y = base_y + (tap_y + off[..., 1]) * offset_scale
    grid = torch.stack(((2 * x + 1) / W - 1, (2 * y + 1) / H - 1), -1)           # align_corners=False
    grid = grid.permute(0, 3, 1, 2, 4, 5).reshape(N * group, Ho * Wo, P, 2)
    planes = input.reshape(N, H, W, group, group_channels).permute(0, 3, 4, 1, 2).reshape(N * group, group_channels, H, W)
    sampled = F.grid_sample(planes, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    weight = mask.reshape(N, Ho * Wo, group, P).permute(0, 2, 1, 3).reshape(N * group, 1, Ho * Wo, P)
    out = (sampled * weight).sum(-1).reshape(N, group * group_channels, Ho, Wo)
    return out.permute(0, 2, 3, 1).contiguous()


class Permute(nn.Module):
    def __init__(self, *dims):
        super().__init__()
        self.dims = dims

    def forward(self, x):
        return x.permute(*self.dims)


def to_channels_first():
    return Permute(0, 3, 1, 2)


def to_channels_last():
    return Permute(0, 2, 3, 1)


def build_norm_layer(dim, norm_layer, in_format="channels_last", out_format="channels_last", eps=1e-6):
    """nn.Sequential of the norm and the layout changes around it; the norm's index inside the Sequential is part of
    the checkpoint key ('LN' from channels_first: `.1`, otherwise `.0`)."""
    if norm_layer == "BN":
        seq = [to_channels_first()] if in_format == "channels_last" else []
        seq.append(nn.BatchNorm2d(dim))
        if out_format == "channels_last":
            seq.append(to_channels_last())
    elif norm_layer == "LN":
        seq = [to_channels_last()] if in_format == "channels_first" else []
        seq.append(nn.LayerNorm(dim, eps=eps))
        if out_format == "channels_first":
            seq.append(to_channels_first())
    else:
        raise NotImplementedError(f"build_norm_layer does not support {norm_layer}")
    return nn.Sequential(*seq)


def build_act_layer(act_layer):
    if act_layer == "ReLU":
        return nn.ReLU(inplace=True)
    if act_layer == "SiLU":
        return nn.SiLU(inplace=True)
    if act_layer == "GELU":
        return nn.GELU()
    raise NotImplementedError(f"build_act_layer does not support {act_layer}")


class _DCNv3Base(nn.Module):
    """input (N,H,W,C) -> output (N,H,W,C):  output_proj(dcnv3(input_proj(x), offset(f), softmax(mask(f)))) with
    f = act(norm(depthwise_conv(x)))."""

    def __init__(self, channels=64, kernel_size=3, dw_kernel_size=None, stride=1, pad=1, dilation=1, group=4,
                 offset_scale=1.0, act_layer="GELU", norm_layer="LN", center_feature_scale=False):
        super().__init__()
        if channels % group != 0:
            raise ValueError(f"channels must be divisible by group, but got {channels} and {group}")
        gc = channels // group
        if gc & (gc - 1):
            warnings.warn("DCNv3: channels // group is not a power of 2; the kernels serve it with idle lanes")
        dw_kernel_size = kernel_size if dw_kernel_size is None else dw_kernel_size
        self.channels, self.kernel_size, self.dw_kernel_size = channels, kernel_size, dw_kernel_size
        self.stride, self.pad, self.dilation = stride, pad, dilation
        self.group, self.group_channels, self.offset_scale = group, gc, offset_scale
        self.center_feature_scale = center_feature_scale
        self.dw_conv = nn.Sequential(
            nn.Conv2d(channels, channels, kernel_size=dw_kernel_size, stride=1, padding=(dw_kernel_size - 1) // 2,
                      groups=channels),
            build_norm_layer(channels, norm_layer, "channels_first", "channels_last"),
            build_act_layer(act_layer))
        self.offset = nn.Linear(channels, group * kernel_size * kernel_size * 2)
        self.mask = nn.Linear(channels, group * kernel_size * kernel_size)
        self.input_proj = nn.Linear(channels, channels)
        self.output_proj = nn.Linear(channels, channels)
        self._reset_parameters()
        if center_feature_scale:
            self.center_feature_scale_proj_weight = nn.Parameter(torch.zeros(group, channels))
            self.center_feature_scale_proj_bias = nn.Parameter(torch.zeros(group))

    def _reset_parameters(self):
        for lin in (self.offset, self.mask):
            nn.init.zeros_(lin.weight)
            nn.init.zeros_(lin.bias)
        for lin in (self.input_proj, self.output_proj):
            nn.init.xavier_uniform_(lin.weight)
            nn.init.zeros_(lin.bias)

    def _core(self, x, offset, mask):
        raise NotImplementedError

    def forward(self, input):
        N, H, W, _ = input.shape
        x = self.input_proj(input)
        feat = self.dw_conv(input.permute(0, 3, 1, 2))
        offset = self.offset(feat)
        mask = F.softmax(self.mask(feat).reshape(N, H, W, self.group, -1), -1).reshape(N, H, W, -1)
        y = self._core(x, offset, mask.type(x.dtype))
        if self.center_feature_scale:
            s = F.linear(feat, self.center_feature_scale_proj_weight, self.center_feature_scale_proj_bias).sigmoid()
            s = s.repeat_interleave(self.group_channels, dim=-1)          # one scale per group, for its channels
            y = y * (1 - s) + x * s
        return self.output_proj(y)

    def _args(self):
        k, s, p, d = self.kernel_size, self.stride, self.pad, self.dilation
        return (k, k, s, s, p, p, d, d, self.group, self.group_channels, self.offset_scale)


class DCNv3_pytorch(_DCNv3Base):
    def _core(self, x, offset, mask):
        return dcnv3_core_pytorch(x, offset, mask, *self._args())


class DCNv3(_DCNv3Base):
    def _core(self, x, offset, mask):
        return DCNv3Function.apply(x, offset, mask, *self._args(), 256)
