"""GPU: whole-model checks at a reduced BEV (24x24) -- the HIP training step against the same step
with every op routed to the CPU oracle (same weights, same sample, same gumbel noise), and the
evaluation path (history BEV -> decode -> chamfer)."""
import numpy as np
import pytest
import torch

import grad_parity as GP
from test_plugin_cpu import _small_batch

pytestmark = pytest.mark.gpu


def _to(batch, dev):
    return dict(img_metas=batch["img_metas"], gt_points=[g.to(dev) for g in batch["gt_points"]],
                img_feats=[f.to(dev) for f in batch["img_feats"]])


def _batch_of(name, bs, bev=24):
    """bs samples of the small rig (bs = 1, bev 24: test_plugin_cpu._small_batch); bev 50 = BASELINE configs[0]'s
    grid, with proportionally larger feature pyramids and ray sets."""
    from vidar_amd.configs import get_config
    from vidar_amd.synthetic import fpn_features, make_sample
    if bs == 1 and bev == 24:
        return _small_batch(name)
    cfg = get_config(name, bev_h=bev, bev_w=bev)
    ms, gts = [], []
    rays = 200 if bev == 24 else 800
    shapes = [(15, 25), (8, 13), (4, 7), (2, 4)] if bev == 24 else [(29, 50), (15, 25), (8, 13), (4, 7)]
    for s_ in range(bs):
        m, g = make_sample(s_, rays_per_frame=rays, future_frames=cfg["future_frames"], num_cams=cfg["num_cams"])
        ms.append(m); gts.append(torch.from_numpy(g))
    feats = fpn_features(0, 5, num_cams=cfg["num_cams"], shapes=shapes, bs=bs)
    return cfg, dict(img_metas=ms, gt_points=gts, img_feats=feats)


@pytest.mark.parametrize("name,bs,bev", [("vidar_1_8_nusc_1future", 1, 24), ("vidar_1_8_nusc_3future", 1, 24),
                                         ("vidar_OpenScene_mini_full_3future", 1, 24),   # 8 cameras (BASELINE config 4)
                                         ("vidar_1_8_nusc_1future", 2, 24),              # per-GPU batch 2 (BASELINE config 3)
                                         ("vidar_1_8_nusc_1future", 1, 50)])             # BASELINE configs[0]'s 50 x 50 BEV
def test_hip_step_matches_cpu_oracle_step(name, bs, bev):
    from oracle import cpu_ops
    from vidar_amd import train as T
    from vidar_amd.plugin.dense_heads import ray_ops
    torch.manual_seed(0); np.random.seed(0)
    cfg, batch = _batch_of(name, bs, bev)
    model = T.build_model(cfg).eval()          # eval: dropout off, identical control flow
    for m in model.modules():
        if hasattr(m, "random_drop_prev_rate"):
            m.random_drop_prev_rate = 0.0
    # BEV self-attention starts with every sampling point exactly ON a pixel centre (integer ring
    # offsets around cell centres): there the bilinear kernel has a kink and d/d(location) is
    # one-sided, so CPU and GPU may legitimately pick different sides.  Move off the kinks.
    g_ = torch.Generator().manual_seed(11)
    for n_, p_ in model.named_parameters():
        if n_.endswith("sampling_offsets.bias"):
            p_.data += torch.randn(p_.shape, generator=g_) * 0.3
    noise = -torch.empty(20000, 512).exponential_(generator=torch.Generator().manual_seed(3)).log()
    model.future_pred_head.gumbel_noise_fn = lambda R, K: noise[:R].to(next(model.parameters()).device)
    model.train(); model.apply(lambda m: setattr(m, "p", 0.0) if isinstance(m, torch.nn.Dropout) else None)
    with cpu_ops.patched():
        ref = model(return_loss=True, **batch)
        ref_total = sum(ref.values())
        ref_grads = torch.autograd.grad(ref_total, [p for p in model.parameters() if p.requires_grad])
    model.cuda()
    out = model(return_loss=True, **_to(batch, "cuda"))
    for k in ref:
        np.testing.assert_allclose(float(out[k]), float(ref[k]), rtol=2e-3, atol=1e-5, err_msg=k)
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    grads = torch.autograd.grad(sum(out.values()), [p for p in model.parameters() if p.requires_grad])
    num = sum(float(((a.cpu() - b) ** 2).sum()) for a, b in zip(grads, ref_grads))
    den = sum(float((b ** 2).sum()) for b in ref_grads)
    assert (num / den) ** 0.5 < 5e-3, f"relative gradient error {(num / den) ** 0.5:.2e}"
    # ... and per parameter tensor, so that a wrong gradient on a small tensor (a bias, level_embeds, lora_a)
    # cannot hide in the aggregate: relative L2 error <= 2e-2 per tensor with no floor in the whole gradient's
    # norm, and exactly zero where the reference is (tests/grad_parity.py)
    bad = GP.compare(names, grads, ref_grads, GP.COEFF, what=f"{name} bs{bs} bev{bev}")
    assert not bad, GP.report(bad)


def test_forward_test_reports_chamfer_per_frame():
    from vidar_amd import train as T
    torch.manual_seed(0); np.random.seed(0)
    from vidar_amd.configs import get_config
    from vidar_amd.synthetic import fpn_features, make_sample
    cfg = get_config("vidar_1_8_nusc_3future", bev_h=24, bev_w=24)
    metas, gt = make_sample(0, rays_per_frame=200, future_frames=6)     # GT clouds for the 6 test futures
    batch = dict(img_metas=[metas], gt_points=[torch.from_numpy(gt)],
                 img_feats=fpn_features(0, 5, shapes=[(15, 25), (8, 13), (4, 7), (2, 4)]))
    model = T.build_model(cfg).cuda()
    res = model(return_loss=False, **_to(batch, "cuda"))[0]
    assert set(res) == {f"frame.{i}" for i in range(7)}      # current + 6 test futures
    for v in res.values():
        assert v["count"] == 1 and np.isfinite(v["chamfer_distance"]) and v["chamfer_distance"] >= 0
        assert np.isfinite(v["l1_error"]) and v["l1_error"] >= 0 and np.isfinite(v["absrel_error"])
