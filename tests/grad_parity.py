"""Per-tensor gradient comparison of two training steps, and the image-backbone step setups that use it
(tests/test_grad_parity_cpu.py, tests/test_step_backbone_gpu.py, tests/test_step_gpu.py, tests/test_data_bridge_gpu.py).

The rule is per parameter tensor, in L2 norms taken in fp64, with NO term in the norm of the whole gradient:
    |ref| == 0   ->  got must be exactly zero (unused parameters, e.g. positional_encoding.{row,col}_embed.weight)
    otherwise    ->  |got - ref| <= coeff * |ref|
An aggregate bound, or a floor proportional to the whole gradient's norm, lets every tensor that holds little of that norm
be entirely wrong: in the ResNet101-DCNv2 step below all of `img_backbone.*` holds 4e-5 of it.

COEFF = 2e-2 is the coefficient the HIP step has always been held to against the oracle-routed step."""
import copy
import functools

import numpy as np
import torch

COEFF = 2e-2
IMG_HW = (96, 160)          # ResNet stage 3 is 6 x 10, stage 4 is 3 x 5: the smallest maps whose DCNv2 blocks keep interior pixels


def compare(names, got, ref, coeff=COEFF, what=""):
    """-> the failing tensors, one dict(name, err, ref, got, ratio) each (ratio = err / (coeff * |ref|); inf where |ref| == 0
    and got is not exactly zero).  Prints the five largest ratios, so that a run's log holds the measured values."""
    names, got, ref = list(names), list(got), list(ref)
    assert len(names) == len(got) == len(ref), (len(names), len(got), len(ref))
    rows = []
    for n, a, b in zip(names, got, ref):
        a, b = a.detach().double().cpu(), b.detach().double().cpu()
        assert a.shape == b.shape, (n, a.shape, b.shape)
        err, nb = float((a - b).norm()), float(b.norm())
        if nb == 0.0:
            ratio = 0.0 if not bool(a.any()) else float("inf")
        else:
            ratio = err / (coeff * nb)
        if ratio != ratio:                                   # a NaN anywhere fails its tensor
            ratio = float("inf")
        rows.append(dict(name=n, err=err, ref=nb, got=float(a.norm()), ratio=ratio))
    rows.sort(key=lambda r: -r["ratio"])
    print(f"grad parity {what}: {len(rows)} tensors, coeff {coeff:.1e}, largest err / (coeff * |ref|):")
    for r in rows[:5]:
        print(f"  {r['ratio']:.3e}  {r['name']}  |err| {r['err']:.3e}  |ref| {r['ref']:.3e}")
    return [r for r in rows if not r["ratio"] <= 1.0]


def report(bad):
    return "per-parameter gradient mismatch:\n" + "\n".join(
        f"{r['name']}: |err| {r['err']:.3e} vs |ref| {r['ref']:.3e} (|got| {r['got']:.3e}, ratio {r['ratio']:.3e})" for r in bad)


def aggregate(got, ref):
    """relative L2 error over all tensors together (what the step tests bounded before the per-tensor rule)"""
    num = sum(float(((a.detach().double().cpu() - b.detach().double().cpu()) ** 2).sum()) for a, b in zip(got, ref))
    den = sum(float((b.detach().double() ** 2).sum()) for b in ref)
    return (num / den) ** 0.5


# ---- the image-backbone steps --------------------------------------------------------------------------------------------

def image_batch(bs=1, num_cams=2, hw=IMG_HW):
    """forward_train kwargs on the host: images [bs, 5, num_cams, 3, *hw] (randn, seed 0), 200 rays per frame"""
    from vidar_amd.synthetic import make_sample
    metas, gts = [], []
    for s in range(bs):
        m, g = make_sample(s, rays_per_frame=200, num_cams=num_cams, img_hw=hw)
        for f in m:
            f["img_shape"] = [(hw[0], hw[1], 3)] * num_cams
        metas.append(m); gts.append(torch.from_numpy(g))
    img = torch.randn(bs, 5, num_cams, 3, hw[0], hw[1], generator=torch.Generator().manual_seed(0))
    return dict(img_metas=metas, gt_points=gts, img=img)


def to_device(batch, dev="cuda"):
    return dict(img_metas=copy.deepcopy(batch["img_metas"]), gt_points=[g.to(dev) for g in batch["gt_points"]],
                img=batch["img"].to(dev))


_NOISE = []


def fix_step(model):
    """no dropped history frame, no dropout, one fixed gumbel noise (that of test_step_gpu); train mode"""
    for m in model.modules():
        if hasattr(m, "random_drop_prev_rate"):
            m.random_drop_prev_rate = 0.0
    model.train()
    model.apply(lambda m: setattr(m, "p", 0.0) if isinstance(m, torch.nn.Dropout) else None)
    if not _NOISE:
        _NOISE.append(-torch.empty(20000, 512).exponential_(generator=torch.Generator().manual_seed(3)).log())
    model.future_pred_head.gumbel_noise_fn = lambda R, K: _NOISE[0][:R].to(next(model.parameters()).device)
    return model


def _config(with_backbone, num_cams=2):
    from vidar_amd.configs import get_config
    cfg = get_config("vidar_1_8_nusc_1future", bev_h=24, bev_w=24, with_backbone=with_backbone)
    tr = cfg["model"]["pts_bbox_head"]["transformer"]
    tr["num_cams"] = num_cams
    tr["encoder"]["transformerlayers"]["attn_cfgs"][1]["num_cams"] = num_cams
    cfg["model"]["use_grid_mask"] = False
    return cfg


def step(model, batch):
    """-> (losses {name: float}, gradients of their sum, one per trainable parameter, on the host)"""
    params = [p for p in model.parameters() if p.requires_grad]
    out = model(return_loss=True, **batch)
    grads = torch.autograd.grad(sum(out.values()), params)
    return {k: float(v.detach()) for k, v in out.items()}, [g.detach().cpu() for g in grads]


def trainable_names(model):
    return [n for n, p in model.named_parameters() if p.requires_grad]


def resnet_model(batch, seed=1):
    """ResNet101-DCNv2 + FPN in the benchmark's `trained_like` regime (vidar_amd/weights.py), calibrated on `batch` on the host"""
    from oracle import cpu_ops
    from vidar_amd import train as T
    from vidar_amd import weights as W
    torch.manual_seed(0); np.random.seed(0)
    model = T.build_model(_config(True))
    for m in model.img_backbone.modules():                  # 101 layers of fp32 stay comparable between device and host
        if isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data.fill_(0.5)
    fix_step(model)
    with cpu_ops.patched():
        rep = W.apply_trained_like(model, batch, seed=seed)
    assert rep["uncalibrated"] == [] and rep["dcn_layers"] == 26 and rep["msda_layers"] == 12, rep
    return model


II_OFFSET_SCALE = 0.1       # test_dcnv3_gpu._randomise scale: DCNv3 offsets of 0.5 .. 2 px standard deviation (asserted)


def internimage_model(core_op):
    """InternImage-T, depths [1, 1, 2, 1], no stochastic depth; core_op 'DCNv3' (HIP) or 'DCNv3_pytorch' (grid_sample)"""
    import warnings
    import vidar_amd.plugin as P
    from test_dcnv3_gpu import _randomise
    torch.manual_seed(0); np.random.seed(0)
    cfg = _config("internimage_t")
    cfg["model"]["img_backbone"].update(depths=[1, 1, 2, 1], drop_path_rate=0.0, core_op=core_op)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = P.build_detector(cfg["model"])
    assert model.img_backbone.core_op == core_op
    _randomise(model.img_backbone, 5, II_OFFSET_SCALE)
    # no `trained_like` here: BEV self-attention keeps its init ring, every sampling point exactly ON a pixel centre, where
    # the bilinear kernel has a kink and host and device may pick different sides (measured: the 12 TSA sampling_offsets
    # tensors off by 34 .. 66 % of |ref|, every other tensor inside the rule).  Off the kinks, as test_step_gpu does.
    g = torch.Generator().manual_seed(11)
    for n, p in model.named_parameters():
        if n.endswith("sampling_offsets.bias"):
            p.data += torch.randn(p.shape, generator=g) * 0.3
    return fix_step(model)


def dcnv3_offset_stds(model, batch):
    """standard deviation of every DCNv3 layer's offset output (pixels: offset_scale = 1) in one no-grad forward pass"""
    from oracle import cpu_ops
    from vidar_amd.plugin.ops_dcnv3 import _DCNv3Base
    stds, hooks = {}, []

    def record(name):
        def hook(mod, args, out):
            stds.setdefault(name, float(out.std()))
        return hook
    for n, m in model.named_modules():
        if isinstance(m, _DCNv3Base):
            assert m.offset_scale == 1.0
            hooks.append(m.offset.register_forward_hook(record(n)))
    try:
        with cpu_ops.patched(), torch.no_grad():
            model(return_loss=True, **batch)
    finally:
        for h in hooks:
            h.remove()
    return stds


@functools.lru_cache(maxsize=None)
def reference(kind, bs=1):
    """the oracle-routed step on the host, computed once per session and left unchanged by its users:
    -> dict(model (host, never moved: deep-copy it), batch, names, losses, grads)"""
    from oracle import cpu_ops
    batch = image_batch(bs)
    if kind == "resnet":
        model = resnet_model(batch)
    elif kind == "internimage":
        model = internimage_model("DCNv3_pytorch")
        stds = dcnv3_offset_stds(model, batch)
        assert len(stds) == 5 and all(0.5 <= s <= 2.0 for s in stds.values()), stds
    else:
        raise KeyError(kind)
    with cpu_ops.patched():
        losses, grads = step(model, to_device(batch, "cpu"))
    return dict(model=model, batch=batch, names=trainable_names(model), losses=losses, grads=grads)
