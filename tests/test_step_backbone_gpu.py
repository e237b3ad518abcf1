"""GPU: the training step WITH the image backbone in the regime the benchmark times, per parameter tensor.

ResNet101-DCNv2 + FPN on `trained_like` weights (vidar_amd/weights.py: every DCNv2 tap ~1.5 px off its pixel, non-uniform
masks, per-query deformable-attention offsets), 2 cameras of 96 x 160 -- stage 3 is 6 x 10 and stage 4 is 3 x 5, the smallest
maps at which all 26 DCNv2 blocks keep interior pixels; the same step meets the LDS-window col2im, `conv3x3_few` and the
fused stem.  The HIP step against the same step routed to the CPU oracle (same weights, images, rays, gumbel noise): every
loss term (rtol 2e-3 / atol 1e-5, as tests/test_step_gpu.py) and every one of the 334 gradient tensors by the rule of
tests/grad_parity.py, |got - ref| <= 2e-2 * |ref| with no term in the whole gradient's norm -- the backbone holds 4e-5 of
that norm, so an aggregate bound cannot see it.  GEMM modes auto / lib / f32 (bf16x3 is another arithmetic class: its
report is printed, not asserted), per-GPU batch 1 and 2.

InternImage-T (depths [1, 1, 2, 1], no stochastic depth, DCNv3 offsets of 0.5 .. 2 px): `core_op="DCNv3"` on the device
against `core_op="DCNv3_pytorch"` on the host with the same state_dict, same rule."""
import copy

import numpy as np
import pytest
import torch

import grad_parity as GP
from vidar_amd import gemm as G

pytestmark = pytest.mark.gpu


def _device_step(model, ref, mode):
    GP.fix_step(model).cuda()
    with G.use(mode):
        return GP.step(model, GP.to_device(ref["batch"]))


def _check(what, ref, losses, grads, assert_rule=True):
    assert set(losses) == set(ref["losses"])
    if assert_rule:
        for k, v in ref["losses"].items():
            np.testing.assert_allclose(losses[k], v, rtol=2e-3, atol=1e-5, err_msg=k)
    print(f"{what}: aggregate relative gradient error {GP.aggregate(grads, ref['grads']):.3e}")
    bad = GP.compare(ref["names"], grads, ref["grads"], GP.COEFF, what=what)
    assert not (bad and assert_rule), GP.report(bad)


@pytest.mark.parametrize("mode,bs", [("auto", 1), ("lib", 1), ("f32", 1), ("auto", 2)])
def test_resnet_dcn_step_matches_oracle_step_per_tensor(mode, bs):
    ref = GP.reference("resnet", bs)
    assert len(ref["names"]) == 334
    losses, grads = _device_step(copy.deepcopy(ref["model"]), ref, mode)
    _check(f"resnet101-dcn {mode} bs{bs}", ref, losses, grads)


def test_resnet_dcn_step_bf16x3_report():
    """16-bit-significand products: measured and printed next to the fp32 modes, nothing asserted beyond finiteness"""
    ref = GP.reference("resnet", 1)
    losses, grads = _device_step(copy.deepcopy(ref["model"]), ref, "bf16x3")
    assert all(np.isfinite(v) for v in losses.values()) and all(torch.isfinite(g).all() for g in grads)
    _check("resnet101-dcn bf16x3 bs1 (not asserted)", ref, losses, grads, assert_rule=False)


def test_internimage_t_step_matches_pytorch_core_step_per_tensor():
    ref = GP.reference("internimage")
    assert len(ref["names"]) == 324
    model = GP.internimage_model("DCNv3")
    model.load_state_dict(ref["model"].state_dict(), strict=True)
    assert GP.trainable_names(model) == ref["names"]
    losses, grads = _device_step(model, ref, "auto")
    _check("internimage-t auto bs1", ref, losses, grads)
