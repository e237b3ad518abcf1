"""GPU: the fused detection loss tail (csrc/det_loss.hip) against the fp64 restatement of tests/test_bevformer_det_cpu.py,
with the PyTorch fp32 composition as the yardstick of what fp32 can do (the kernels may be at most 4 x as far from fp64:
slack for different expf / logf implementations, not a target); bitwise run-to-run equality; the fine-tune training
step fused vs VIDAR_DET_LOSS=torch; the host-sync budget; the decoder's cross attention shape against the MSDA oracle.
Measured figures are printed (run with -s to keep them) and recorded in profiles/kbench_det.md."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from test_bevformer_det_cpu import CASES, FPN_SMALL, cost_fp64, loss_fp64, tail_case

pytestmark = pytest.mark.gpu
sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
ARGS = (0.25, 2.0, 2.0, 0.25)           # alpha, gamma, cls_weight, reg_weight of the released configs
FULL = [(6, 1, 900, [0]), (6, 1, 900, [1]), (6, 1, 900, [37]), (6, 2, 900, [150, 37]), (6, 2, 900, [512, 0]),
        (6, 1, 900, [150]), (6, 2, 900, [0, 0])]


def record(line):
    """print a measured figure and, when VIDAR_DET_RECORD names a file, append it there (profiles/kbench_det.md is written
    from that file)"""
    import os
    print(line)
    if os.environ.get("VIDAR_DET_RECORD"):
        with open(os.environ["VIDAR_DET_RECORD"], "a") as f:
            f.write(line + "\n")


def dev(c):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in c.items()}


def blocks(cost, NL, Q, c):
    out = []
    for l in range(NL):
        row = []
        for b, G in enumerate(c["counts"]):
            s = int(c["gt_start"][b])
            row.append(cost[l, Q * s:Q * (s + G)].reshape(Q, G).double().cpu())
        out.append(row)
    return out


def max_err(got, want):
    return max([float((g - w).abs().max()) for gr, wr in zip(got, want) for g, w in zip(gr, wr) if w.numel()] or [0.0])


def check_cost(c, NL, B, Q, C, what):
    from scipy.optimize import linear_sum_assignment
    from vidar_amd.plugin.dense_heads import det_ops as D
    d = dev(c)
    total = sum(c["counts"])
    want = cost_fp64(c)
    hip = D.match_cost(d["cls"], d["box"], d["gt_norm"], d["gt_label"], d["gt_start"], total, *ARGS)
    ref = D.match_cost_torch(d["cls"], d["box"], d["gt_norm"], d["gt_label"], c["counts"], *ARGS)
    assert hip.shape == ref.shape == (NL, Q * total)
    e_hip, e_ref = max_err(blocks(hip, NL, Q, c), want), max_err(blocks(ref, NL, Q, c), want)
    record(f"match_cost {what}: max |err| vs fp64  hip {e_hip:.3e}  torch fp32 {e_ref:.3e}")
    assert e_hip <= 4 * e_ref, (e_hip, e_ref)
    matched = D.hungarian(hip, NL, Q, c["counts"]).cpu().numpy()
    assert matched.shape == (NL, B, Q) and matched.dtype == np.int32
    for l in range(NL):
        for b, G in enumerate(c["counts"]):
            m = matched[l, b]
            assert int((m >= 0).sum()) == min(Q, G) and (G == 0 or len(set(m[m >= 0].tolist())) == min(Q, G))
            if G:
                rows, cols = linear_sum_assignment(want[l][b].numpy())
                best = float(want[l][b][rows, cols].sum())
                got = float(want[l][b][np.nonzero(m >= 0)[0], m[m >= 0]].sum())
                assert abs(got - best) <= 1e-6 * abs(best), (l, b, got, best)
    return matched, e_hip, e_ref


@pytest.mark.parametrize("NL,B,Q,counts", FULL, ids=[f"B{f[1]}-G{'_'.join(map(str, f[3]))}" for f in FULL])
def test_match_cost_full_size(NL, B, Q, counts):
    check_cost(tail_case(100 + sum(counts), NL, B, Q, 10, counts), NL, B, Q, 10, f"B {B} G {counts}")


@pytest.mark.parametrize("case", CASES, ids=[f"case{c[0]}" for c in CASES])
def test_match_cost_small_cases_and_their_assignments(case):
    from vidar_amd.plugin.dense_heads import det_ops as D
    seed, NL, B, Q, C, counts = case
    c = tail_case(seed, NL, B, Q, C, [min(n, 40) for n in counts])
    c["gt_label"] = c["gt_label"] % C
    matched, _, _ = check_cost(c, NL, B, Q, C, f"case {seed}")
    cpu = D.solve(D.match_cost_torch(c["cls"], c["box"], c["gt_norm"], c["gt_label"], c["counts"], *ARGS).numpy(), NL, Q, c["counts"])
    assert np.array_equal(matched, cpu)                     # the assignment the CPU composition (and the assigner) finds


def loss_both(c, NL, B, Q, C, what):
    from vidar_amd.plugin.dense_heads import det_ops as D
    d = dev(c)
    total = sum(c["counts"])
    cost = D.match_cost(d["cls"], d["box"], d["gt_norm"], d["gt_label"], d["gt_start"], total, *ARGS)
    matched = D.hungarian(cost, NL, Q, c["counts"])
    labels = D.labels_from_matched(matched, d["gt_label"], d["gt_start"], C)
    cw = torch.tensor([1.0] * 8 + [0.2] * 2)
    w = torch.tensor([[1.0, 0.5]]).repeat(NL, 1)

    def run(fn, cls, box, gt, cw_, w_):
        cls, box = cls.clone().requires_grad_(True), box.clone().requires_grad_(True)
        s = fn(cls, box, labels.to(cls.device), matched.to(cls.device), gt, d["gt_start"].to(cls.device), cw_, 0.25, 2.0)
        return (s.detach(),) + tuple(g.detach() for g in torch.autograd.grad((s * w_).sum(), [cls, box]))
    hip = run(D.DetLossFunction.apply, d["cls"], d["box"], d["gt_norm"], cw.cuda(), w.cuda())
    again = run(D.DetLossFunction.apply, d["cls"], d["box"], d["gt_norm"], cw.cuda(), w.cuda())
    for a, b in zip(hip, again):
        assert torch.equal(a, b), "two calls on the same inputs must agree bit for bit"
    ref = run(D.det_loss_sums_torch, d["cls"], d["box"], d["gt_norm"], cw.cuda(), w.cuda())
    f64 = run(D.det_loss_sums_torch, c["cls"].double(), c["box"].double(), c["gt_norm"].double(), cw.double(), w.double())
    want_sums = loss_fp64(c, labels.cpu(), matched.cpu(), cw)
    torch.testing.assert_close(f64[0], want_sums, rtol=1e-9, atol=1e-9)
    for nm, h, r, t in zip(("sums", "grad_cls", "grad_box"), hip, ref, f64):
        e_hip = float((h.double().cpu() - t).abs().max())          # plain max abs error, as for the cost
        e_ref = float((r.double().cpu() - t).abs().max())
        record(f"det_loss {what} {nm}: max |err| vs fp64  hip {e_hip:.3e}  torch fp32 {e_ref:.3e}  (|fp64|_max {float(t.abs().max()):.3e})")
        assert e_hip <= 4 * e_ref, (nm, e_hip, e_ref)
    if total == 0:
        assert float(hip[0][:, 1].abs().max()) == 0.0 and float(hip[2].abs().max()) == 0.0
    nonfinite = ~torch.isfinite(c["gt_norm"]).all(-1)
    return int(nonfinite.sum())


@pytest.mark.parametrize("NL,B,Q,counts", FULL, ids=[f"B{f[1]}-G{'_'.join(map(str, f[3]))}" for f in FULL])
def test_det_loss_full_size(NL, B, Q, counts):
    n_bad = loss_both(tail_case(200 + sum(counts), NL, B, Q, 10, counts), NL, B, Q, 10, f"B {B} G {counts}")
    if sum(counts) >= 37:
        assert n_bad > 0                       # rows with NaN velocities are among the targets


@pytest.mark.parametrize("case", CASES, ids=[f"case{c[0]}" for c in CASES])
def test_det_loss_small_cases(case):
    seed, NL, B, Q, C, counts = case
    c = tail_case(seed, NL, B, Q, C, [min(n, 40) for n in counts])
    c["gt_label"] = c["gt_label"] % C
    loss_both(c, NL, B, Q, C, f"case {seed}")


def test_bad_arguments_are_refused():
    from vidar_amd.plugin.dense_heads import det_ops as D
    c = dev(tail_case(1, 2, 1, 6, 10, [3]))
    wide = torch.zeros(2, 1, 6, 65, device="cuda")
    with pytest.raises(ValueError):
        D.match_cost(wide, c["box"], c["gt_norm"], c["gt_label"], c["gt_start"], 3, *ARGS)


def finetune_batch(bs=1, num_query=900):
    from vidar_amd.configs import get_config
    from vidar_amd.plugin.core_bbox import LiDARInstance3DBoxes
    from vidar_amd.synthetic import fpn_features, make_sample
    cfg = get_config("finetune/vidar_1_8_nusc_1future", bev_h=24, bev_w=24)          # the BEV size of _small_batch
    cfg["model"]["pts_bbox_head"]["num_query"] = num_query
    metas, boxes, labels = [], [], []
    for s in range(bs):
        m, _, b, l = make_sample(s, queue_length=cfg["queue_length"], rays_per_frame=10, with_boxes=True)
        metas.append(m); boxes.append(LiDARInstance3DBoxes(b)); labels.append(torch.from_numpy(l))
    feats = [f.cuda() for f in fpn_features(0, cfg["queue_length"] + 1, shapes=FPN_SMALL, bs=bs)]
    return cfg, dict(img_metas=metas, img_feats=feats, gt_bboxes_3d=boxes, gt_labels_3d=labels)


@pytest.mark.parametrize("bs", [1, 2])
def test_forward_train_fused_equals_the_torch_path(bs, monkeypatch):
    from vidar_amd import train as T
    torch.manual_seed(0); np.random.seed(0)
    cfg, batch = finetune_batch(bs)
    model = T.build_model(cfg).cuda().train()
    model.apply(lambda m: setattr(m, "p", 0.0) if isinstance(m, torch.nn.Dropout) else None)
    for m in model.modules():
        if isinstance(m, torch.nn.MultiheadAttention):
            m.dropout = 0.0
    params = [p for p in model.parameters() if p.requires_grad]
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    res = {}
    for mode in ("torch", "hip"):
        monkeypatch.setenv("VIDAR_DET_LOSS", mode)
        out = model(return_loss=True, **batch)
        res[mode] = ({k: float(v) for k, v in out.items()}, torch.autograd.grad(sum(out.values()), params))
    ref, out = res["torch"][0], res["hip"][0]
    assert set(ref) == set(out) and len(out) == 12
    for k in ref:
        print(f"{k}: fused {out[k]:.6f} torch {ref[k]:.6f}")
        np.testing.assert_allclose(out[k], ref[k], rtol=2e-3, atol=1e-5, err_msg=k)
    grads, ref_grads = res["hip"][1], res["torch"][1]
    num = sum(float(((a - b) ** 2).sum()) for a, b in zip(grads, ref_grads))
    den = sum(float((b ** 2).sum()) for b in ref_grads)
    record(f"forward_train bs {bs}: fused vs torch path, relative gradient error {(num / den) ** 0.5:.2e}")
    assert (num / den) ** 0.5 < 5e-3
    bad = []
    for n, a, b in zip(names, grads, ref_grads):
        err = float((a - b).norm())
        if err > 2e-2 * float(b.norm()) + 1e-4 * den ** 0.5:
            bad.append(f"{n}: |err| {err:.3e} vs |grad| {float(b.norm()):.3e}")
    assert not bad, "per-parameter gradient mismatch:\n" + "\n".join(bad)


@pytest.mark.parametrize("bs", [1, 2])
def test_host_syncs_of_one_finetune_step(bs, monkeypatch):
    """fused: the encoder's planned read + the one cost copy (+ one tolerated spare).  torch: the reference's structure, one
    blocking cost copy per (decoder layer, sample) at least -- counted by the same counter, which must see the difference."""
    from sync_count import count_syncs
    from vidar_amd import train as T
    torch.manual_seed(0); np.random.seed(0)
    cfg, batch = finetune_batch(bs)
    model = T.build_model(cfg).cuda().train()
    opt = T.build_optimizer(model)
    counts = {}
    for mode in ("hip", "torch"):
        monkeypatch.setenv("VIDAR_DET_LOSS", mode)
        for _ in range(2):
            T.train_step(model, opt, batch)
        counts[mode] = count_syncs(lambda: T.train_step(model, opt, batch))
        record(f"{mode}: {counts[mode][0]} host syncs in one fine-tune step (bs {bs}): {dict(counts[mode][1])}")
    assert counts["hip"][0] <= 3, dict(counts["hip"][1])
    assert counts["torch"][0] >= 6 * bs and counts["torch"][0] > counts["hip"][0], dict(counts["torch"][1])


@pytest.mark.parametrize("B", [1, 2])
def test_decoder_cross_attention_shape_matches_the_msda_oracle(B):
    """900 object queries over the 200 x 200 BEV, L = 1, P = 4: forward and backward under the tolerances of
    tests/test_msda_gpu.py::test_full_size_matches_oracle (same kink exemption for grad_loc)."""
    from oracle import msda as M
    from vidar_amd.plugin.modules import multi_scale_deformable_attn_function as F
    shapes, Nq, P = [(200, 200)], 900, 4
    value, sh, loc, w = M.make_case(21 + B, B, shapes, Nq, P=P)
    gout = torch.randn(B, Nq, 256, generator=torch.Generator().manual_seed(5))
    v, l_, w_ = (t.double().requires_grad_(True) for t in (value, loc, w))
    ref = M.msda_grid_sample(v, sh, l_, w_)
    rv, rl, rw = torch.autograd.grad((ref * gout.double()).sum(), [v, l_, w_])
    lsi = M.level_start_index(shapes).cuda()
    dv, dl, dw = value.cuda(), loc.cuda(), w.cuda()
    out = F._msda_forward(dv, sh.cuda(), lsi, dl, dw)
    torch.testing.assert_close(out.cpu().double(), ref.detach(), rtol=1e-4, atol=1e-4)
    got = [g.cpu().double() for g in F._msda_backward(dv, sh.cuda(), lsi, dl, dw, gout.cuda())]
    wh = torch.tensor([[w__, h__] for h__, w__ in shapes], dtype=torch.float64).view(1, 1, 1, 1, 1, 2)
    pixel = loc.double() * wh - 0.5
    live = ((pixel > -1 - 1e-4) & (pixel < wh + 1e-4)).all(-1, keepdim=True)
    kink = (((pixel - pixel.round()).abs() < 1e-4).any(-1, keepdim=True) & live).expand_as(loc)
    assert float(kink[..., 0].double().sum() / live.double().sum()) < 2e-3
    got[1] = torch.where(kink, rl, got[1])
    for g, r, nm in zip(got, (rv, rl, rw), ["grad_value", "grad_loc", "grad_w"]):
        scale = max(1.0, float(r.abs().max()))
        torch.testing.assert_close(g, r, rtol=2e-4, atol=1e-4 * scale, msg=lambda m: nm + m)


# ---- the reference's golden (tests/golden/make_bevformer_det_golden.py) on the GPU -------------------------------------
def test_golden_head_forward_loss_and_gradients_on_the_gpu():
    """the CPU golden test's comparison, HIP ops and the fused loss tail: same tolerances"""
    import test_bevformer_det_golden_cpu as G
    from vidar_amd.plugin.core_bbox import LiDARInstance3DBoxes
    gold = G.load_gold()
    data, meta = gold
    model = G.build(gold, "cuda").train()
    head = model.pts_bbox_head
    feats = [torch.from_numpy(data["feats0"]).cuda(), torch.from_numpy(data["feats1"]).cuda()]
    preds = head(feats, [G.frame_meta(data)], torch.from_numpy(data["prev_bev"]).cuda())
    for k in ("bev_embed", "all_cls_scores", "all_bbox_preds"):
        np.testing.assert_allclose(preds[k].detach().cpu().numpy(), data[k], err_msg=k, **G.OUT_TOL)
    losses = head.loss([LiDARInstance3DBoxes(torch.from_numpy(data["train_boxes"]))], [torch.from_numpy(data["train_labels"])], preds)
    for n, want in zip(data["loss_names"], data["loss_values"]):
        np.testing.assert_allclose(float(losses[str(n)]), want, err_msg=str(n), **G.LOSS_TOL)
    names = [str(n) for n in data["grad_names"]]
    params = dict(model.named_parameters())
    grads = torch.autograd.grad(sum(losses.values()), [params["pts_bbox_head." + n] for n in names])
    for n, g in zip(names, grads):
        G.grad_close(g.cpu().numpy(), data["grad/pts_bbox_head." + n], n)


@pytest.mark.parametrize("name", ["mixed", "empty_and_over", "square", "no_gt", "single"])
def test_golden_loss_cases_fused_assignments_identical(name):
    """HIP cost -> assignments identical to the reference's on every stable golden case; fused losses and gradients against
    the reference's loss dictionary"""
    import test_bevformer_det_golden_cpu as G
    from vidar_amd.plugin.core_bbox import LiDARInstance3DBoxes
    from vidar_amd.plugin.dense_heads import det_ops as D
    gold = G.load_gold()
    data, meta = gold
    case, p, boxes, labels = G.loss_case(data, meta, name)
    counts, Q = case["counts"], case["Q"]
    head = G.build(gold, "cuda").pts_bbox_head
    cls = torch.from_numpy(data[p + "cls"]).cuda().requires_grad_(True)
    box = torch.from_numpy(data[p + "box"]).cuda().requires_grad_(True)
    gt_norm, gt_label = G.pack(boxes, labels)
    start = torch.from_numpy(D.gt_starts(counts)).cuda()
    cost = D.match_cost(cls, box, gt_norm.cuda().contiguous(), gt_label.cuda(), start, sum(counts), *ARGS)
    assert np.array_equal(D.hungarian(cost, 6, Q, counts).cpu().numpy(), data[p + "matched"])
    got = head.loss([LiDARInstance3DBoxes(b) for b in boxes], labels,
                    dict(all_cls_scores=cls, all_bbox_preds=box, enc_cls_scores=None, enc_bbox_preds=None))
    for k, v in zip((str(n) for n in data[p + "loss_names"]), data[p + "loss_values"]):
        np.testing.assert_allclose(float(got[k]), v, err_msg=k, **G.LOSS_TOL)
    g = torch.autograd.grad(sum(got.values()), [cls, box])
    G.grad_close(g[0].cpu().numpy(), data[p + "grad_cls"], "grad_cls"); G.grad_close(g[1].cpu().numpy(), data[p + "grad_box"], "grad_box")


def test_golden_video_inference_on_the_gpu():
    import test_bevformer_det_golden_cpu as G
    gold = G.load_gold()
    model = G.build(gold, "cuda").eval()
    G.check_sequence(G.run_sequence(model, gold[0], gold[1], "cuda"), gold[0])
