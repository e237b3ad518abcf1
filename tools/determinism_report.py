"""Are two seeded training steps bit-equal?  A report, not a gate.

    python tools/determinism_report.py [--bev 12] [--config vidar_1_8_nusc_1future]

Runs the same seeded step twice (same weights, sample, dropout and gumbel streams) at a small BEV, without and with the
image backbone, with the deterministic mode (vidar_amd/deterministic.py) off and on, and prints per parameter whether
the two gradients are the same bits.  With the mode on it also sets torch.use_deterministic_algorithms(True,
warn_only=True) and lists which torch ops and which own ops warned.  Whether hipBLASLt / MIOpen / torch's own backward ops
reproduce is their business: this only shows what they do here."""
import argparse
import json
import sys
import warnings
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def make_batch(cfg, with_backbone, bev, dev):
    from bench import synthetic_images
    from vidar_amd.synthetic import fpn_features, make_sample
    div = max(1, 200 // bev // 2)                     # images and pyramids shrink with the BEV
    metas, gt = make_sample(0, rays_per_frame=200, future_frames=cfg["future_frames"], num_cams=cfg["num_cams"],
                            img_hw=cfg["img_hw"])
    batch = dict(img_metas=[metas], gt_points=[torch.from_numpy(gt).to(dev)])
    if with_backbone:
        qhw = (cfg["img_hw"][0] // div, cfg["img_hw"][1] // div)
        for m in metas:
            m["img_shape"] = [(qhw[0], qhw[1], 3)] * cfg["num_cams"]
            k = np.diag([1.0 / div, 1.0 / div, 1.0, 1.0])
            m["lidar2img"] = [k @ a for a in m["lidar2img"]]
        batch["img"] = synthetic_images(0, 5, cfg["num_cams"], cfg["img_hw"], "cpu", scale=div).to(dev)
    else:
        shapes = [((h + div - 1) // div, (w + div - 1) // div) for h, w in cfg["fpn_shapes"]]
        batch["img_feats"] = [f.to(dev) for f in fpn_features(0, 5, num_cams=cfg["num_cams"], shapes=shapes)]
    return batch


def step_grads(model, batch):
    torch.manual_seed(1234); np.random.seed(1234)
    model.zero_grad(set_to_none=True)
    losses = model(return_loss=True, **batch)
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}, \
        {k: float(v) for k, v in losses.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="vidar_1_8_nusc_1future")
    ap.add_argument("--bev", type=int, default=12)
    args = ap.parse_args()
    from vidar_amd import deterministic, train as T
    from vidar_amd.configs import get_config
    dev = torch.device("cuda", 0)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "config": args.config, "bev": args.bev}))
    for with_backbone in (False, True):
        cfg = get_config(args.config, bev_h=args.bev, bev_w=args.bev, with_backbone=with_backbone)
        torch.manual_seed(0); np.random.seed(0)
        model = T.build_model(cfg).to(dev).train()
        batch = make_batch(cfg, with_backbone, args.bev, dev)
        for mode in (False, True):
            torch.use_deterministic_algorithms(mode, warn_only=True)
            deterministic._warned.clear()
            try:
                with warnings.catch_warnings(record=True) as caught, deterministic.use(None):
                    warnings.simplefilter("always")
                    step_grads(model, batch)                                   # warm-up: lazy initialisation, tuning
                    a, la = step_grads(model, batch)
                    b, lb = step_grads(model, batch)
            finally:
                torch.use_deterministic_algorithms(False)
            equal = {n: bool(torch.equal(a[n].view(torch.int32), b[n].view(torch.int32))) for n in a}
            differ = sorted(n for n, e in equal.items() if not e)
            torch_warned = sorted({str(w.message).split("(")[0].strip()[:120] for w in caught
                                   if "deterministic" in str(w.message) and "vidar_amd" not in str(w.message)})
            head = dict(backbone=with_backbone, deterministic_mode=mode, parameters=len(equal),
                        bit_equal=len(equal) - len(differ), losses_bit_equal=la == lb,
                        own_ops_warned=deterministic.warned(), torch_ops_warned=torch_warned)
            print(json.dumps(head))
            for n in sorted(equal):
                worst = float((a[n] - b[n]).abs().max())
                print(f"  {'equal ' if equal[n] else 'DIFFER'} {n}" + ("" if equal[n] else f"  max|a-b| {worst:.3e}"))


if __name__ == "__main__":
    main()
