"""`DCNv3`: the two functions of the reference's compiled extension
(bevformer/backbones/ops_dcnv3/src/vision.cpp; called from functions/dcnv3_func.py:39-43, :54-58), on
csrc/dcnv3.hip.  Channel-last fp32 tensors on the GPU; `im2col_step` only batches the reference's launches and is
accepted and ignored.  No CPU path: host tensors raise RuntimeError like the reference's AT_ERROR("Not implemented
on the CPU")."""
from __future__ import annotations

import torch

from .._lib import lib, check, ptr, stream_of, workspace
from .. import deterministic
from ._common import check_input


def _geometry(input, offset, mask, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w,
              group, group_channels):
    for x, nm in ((input, "input"), (offset, "offset"), (mask, "mask")):
        check_input(x, nm)
    if input.dim() != 4 or offset.dim() != 4 or mask.dim() != 4:
        raise RuntimeError("expected input[N,H,W,C], offset[N,Ho,Wo,G*P*2], mask[N,Ho,Wo,G*P]")
    ints = [int(v) for v in (kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, group,
                             group_channels)]
    kh, kw, sh, sw, ph, pw, dh, dw, G, gc = ints
    if min(kh, kw, sh, sw, dh, dw, G, gc) <= 0 or min(ph, pw) < 0:
        raise ValueError("DCNv3: kernel, stride, dilation, group and group_channels must be positive, pad >= 0")
    N, H, W, C = input.shape
    if C != G * gc:
        raise RuntimeError(f"Input shape and kernel channels wont match: ({C} vs {G * gc}).")
    eh, ew = dh * (kh - 1) + 1, dw * (kw - 1) + 1
    if H + 2 * ph < eh or W + 2 * pw < ew:
        raise ValueError("DCNv3: the kernel extent is larger than the padded input")
    Ho, Wo = (H + 2 * ph - eh) // sh + 1, (W + 2 * pw - ew) // sw + 1
    P = kh * kw
    if tuple(offset.shape) != (N, Ho, Wo, G * P * 2) or tuple(mask.shape) != (N, Ho, Wo, G * P):
        raise RuntimeError(f"DCNv3: offset / mask must be [{N},{Ho},{Wo},{G * P * 2}] / [{N},{Ho},{Wo},{G * P}], got "
                           f"{tuple(offset.shape)} / {tuple(mask.shape)}")
    if offset.device != input.device or mask.device != input.device:
        raise RuntimeError("DCNv3: input, offset and mask must be on one device")
    return (N, H, W, Ho, Wo), ints


def dcnv3_forward(input, offset, mask, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w,
                  group, group_channels, offset_scale, im2col_step):
    """-> output [N,Ho,Wo,group*group_channels]"""
    (N, H, W, Ho, Wo), g = _geometry(input, offset, mask, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w,
                                     dilation_h, dilation_w, group, group_channels)
    out = torch.empty((N, Ho, Wo, input.shape[3]), dtype=torch.float32, device=input.device)
    with torch.cuda.device(input.device):
        check(lib().vidar_dcnv3_forward_f32(ptr(input), ptr(offset), ptr(mask), ptr(out), N, H, W, *g,
                                            float(offset_scale), stream_of(input)), "DCNv3.dcnv3_forward")
    return out


def dcnv3_backward(input, offset, mask, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w,
                   group, group_channels, offset_scale, grad_output, im2col_step):
    """-> [grad_input, grad_offset, grad_mask]"""
    deterministic.require("dcnv3 backward")
    (N, H, W, Ho, Wo), g = _geometry(input, offset, mask, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w,
                                     dilation_h, dilation_w, group, group_channels)
    check_input(grad_output, "grad_output")
    if tuple(grad_output.shape) != (N, Ho, Wo, input.shape[3]) or grad_output.device != input.device:
        raise RuntimeError(f"DCNv3: grad_output must be [{N},{Ho},{Wo},{input.shape[3]}] on the input's device")
    grad_input = torch.empty_like(input)
    grad_offset = torch.empty_like(offset)
    grad_mask = torch.empty_like(mask)
    with torch.cuda.device(input.device):
        L = lib()
        ws, wp, wn = workspace(L.vidar_dcnv3_backward_workspace_bytes, N, H, W, *g, like=input)
        check(L.vidar_dcnv3_backward_f32(ptr(input), ptr(offset), ptr(mask), ptr(grad_output), ptr(grad_input),
                                         ptr(grad_offset), ptr(grad_mask), N, H, W, *g,
                                         float(offset_scale), wp, wn, stream_of(input)),
              "DCNv3.dcnv3_backward")
    return [grad_input, grad_offset, grad_mask]
