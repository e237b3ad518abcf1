"""CPU: the BEVFormer detection branch against golden vectors produced by the reference's OWN source text
(tests/golden/make_bevformer_det_golden.py: PerceptionTransformer.forward, DetectionTransformerDecoder, the body of
BEVFormerHead, HungarianAssigner3D, BBox3DL1Cost, normalize_bbox, NMSFreeCoder, BEVFormer.forward_test, executed in place;
the loss modules on that side are mmdet's binary-cross-entropy form of the focal loss, not this package's formula).
Tolerances are the ones the existing golden tests of the same width apply: outputs rtol 2e-4 / atol 2e-5
(tests/test_transformer_golden_cpu.py:58), gradients rtol 2e-3 / atol 2e-5 x max(1, |ref|_max) (:66), losses
rtol 5e-4 / atol 1e-6 (tests/test_detector_golden_cpu.py:86), decoded boxes rtol 1e-3 / atol 1e-5 (:65).
Hungarian assignments must be IDENTICAL on every case (the generator keeps only cases whose assignment survives +-1e-4
relative noise on the fp64 cost matrix)."""
import copy
import json
from pathlib import Path

import numpy as np
import pytest
import torch

GOLD = Path(__file__).parent / "golden"
OUT_TOL = dict(rtol=2e-4, atol=2e-5)
LOSS_TOL = dict(rtol=5e-4, atol=1e-6)
BOX_TOL = dict(rtol=1e-3, atol=1e-5)


def grad_close(got, ref, what):
    np.testing.assert_allclose(got, ref, rtol=2e-3, atol=2e-5 * max(1.0, float(np.abs(ref).max())), err_msg=what)


@pytest.fixture(scope="module")
def gold():
    return load_gold()


class Shards(dict):
    @property
    def files(self):
        return list(self)


def load_gold():
    meta = json.loads((GOLD / "bevformer_det_small.json").read_text())
    data = Shards()
    for n in range(meta["shards"]):
        with np.load(GOLD / f"bevformer_det_small.{n}.npz", allow_pickle=False) as z:
            data.update({k: z[k] for k in z.files})
    return data, meta


def build(gold, device="cpu"):
    import vidar_amd.plugin as P
    data, meta = gold
    model = P.build_detector(copy.deepcopy(meta["cfg"]))
    sd = {k[3:]: torch.from_numpy(data[k]) for k in data.files if k.startswith("sd/")}
    model.load_state_dict(sd, strict=True)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if isinstance(m, torch.nn.MultiheadAttention):
            m.dropout = 0.0
    return model.to(device)


def frame_meta(data, prefix=None):
    m = dict(lidar2img=[x for x in data["lidar2img"]], img_shape=[tuple(int(v) for v in s) for s in data["img_shape"]])
    if prefix is None:
        m.update(can_bus=data["meta2_can_bus"].copy(), lidar2global_rotation=data["meta2_lidar2global_rotation"])
    return m


def test_head_parameter_names_and_shapes_equal_the_reference_heads(gold):
    """the full sorted (name, shape) list recorded from the reference's BEVFormerHead"""
    import vidar_amd.plugin as P
    data, meta = gold
    model = P.build_detector(copy.deepcopy(meta["cfg"]))
    mine = [[k[len("pts_bbox_head."):], list(v.shape)] for k, v in sorted(model.state_dict().items())
            if k.startswith("pts_bbox_head.")]
    assert mine == meta["head_state_dict"]
    assert len(mine) > 150 and sorted(model.state_dict()) == sorted("pts_bbox_head." + k for k, _ in meta["head_state_dict"])


def test_full_size_recipe_has_the_reference_layout_scaled_up(gold):
    """the released-size recipe has exactly the reference head's key list (shapes at width 256 / 6 + 6 layers differ)"""
    import vidar_amd.plugin as P
    from vidar_amd.configs import get_config
    data, meta = gold
    small = {k for k, _ in meta["head_state_dict"]}
    full = {k[len("pts_bbox_head."):] for k in P.build_detector(get_config("finetune/vidar_1_8_nusc_1future", bev_h=12, bev_w=12)["model"]).state_dict()}
    strip = lambda ks: {k for k in ks if ".encoder.layers." not in k}       # the golden has 2 encoder layers, the recipe 6
    assert strip(small) == strip(full)
    enc = lambda ks, i: {k.split(f".encoder.layers.{i}.")[1] for k in ks if f".encoder.layers.{i}." in k}
    assert enc(small, 0) == enc(full, 0) and enc(small, 1) == enc(full, 2)   # plain layer / the LatentRendering layer


def test_head_forward_loss_gradients_and_assignments_match_the_reference(gold):
    from oracle import cpu_ops
    from vidar_amd.plugin.core_bbox import LiDARInstance3DBoxes
    from vidar_amd.plugin.dense_heads import det_ops as D
    data, meta = gold
    model = build(gold).train()
    head = model.pts_bbox_head
    feats = [torch.from_numpy(data["feats0"]), torch.from_numpy(data["feats1"])]
    with cpu_ops.patched():
        preds = head(feats, [frame_meta(data)], torch.from_numpy(data["prev_bev"]))
        np.testing.assert_allclose(preds["bev_embed"].detach().numpy(), data["bev_embed"], **OUT_TOL)
        np.testing.assert_allclose(preds["all_cls_scores"].detach().numpy(), data["all_cls_scores"], **OUT_TOL)
        np.testing.assert_allclose(preds["all_bbox_preds"].detach().numpy(), data["all_bbox_preds"], **OUT_TOL)
        boxes, labels = torch.from_numpy(data["train_boxes"]), torch.from_numpy(data["train_labels"])
        losses = head.loss([LiDARInstance3DBoxes(boxes)], [labels], preds)
        assert sorted(losses) == [str(n) for n in data["loss_names"]] and len(losses) == 12
        for n, want in zip(data["loss_names"], data["loss_values"]):
            np.testing.assert_allclose(float(losses[str(n)].detach()), want, err_msg=str(n), **LOSS_TOL)
        names = [str(n) for n in data["grad_names"]]
        params = dict(model.named_parameters())
        assert sorted("pts_bbox_head." + n for n in names) == sorted(k for k, p in params.items() if p.requires_grad)
        grads = torch.autograd.grad(sum(losses.values()), [params["pts_bbox_head." + n] for n in names])
    for n, g in zip(names, grads):
        grad_close(g.numpy(), data["grad/pts_bbox_head." + n], n)
    # the assignment of every decoder layer, from the packed cost composition the fused kernels implement
    c = pack([boxes], [labels])
    cost = D.match_cost_torch(preds["all_cls_scores"].detach(), preds["all_bbox_preds"].detach(), c[0], c[1], [5], 0.25, 2.0, 2.0, 0.25)
    assert np.array_equal(D.solve(cost.numpy(), 6, 12, [5])[:, 0], data["train_matched"])


def pack(boxes, labels):
    from vidar_amd.plugin.core_bbox import LiDARInstance3DBoxes, normalize_bbox
    raw = [LiDARInstance3DBoxes(b) for b in boxes]
    gt = torch.cat([torch.cat((r.gravity_center, r.tensor[:, 3:]), 1) for r in raw])
    return (normalize_bbox(gt) if gt.shape[0] else torch.zeros((0, 10))), torch.cat(labels).to(torch.int32)


def loss_case(data, meta, name):
    case = next(c for c in meta["loss_cases"] if c["name"] == name)
    p = f"case/{name}/"
    boxes = [torch.from_numpy(data[p + f"boxes{b}"]).reshape(-1, 9) for b in range(case["B"])]
    labels = [torch.from_numpy(data[p + f"labels{b}"]).long() for b in range(case["B"])]
    return case, p, boxes, labels


CASE_NAMES = ("mixed", "empty_and_over", "square", "no_gt", "single")


def test_generator_kept_enough_stable_problems(gold):
    data, meta = gold
    assert [c["name"] for c in meta["loss_cases"]] == list(CASE_NAMES)
    assert meta["stable_problems"] >= 6 and meta["unstable_cases_dropped"] >= 0
    assert any(0 in c["counts"] for c in meta["loss_cases"]) and any(max(c["counts"]) > c["Q"] for c in meta["loss_cases"])


@pytest.mark.parametrize("name", CASE_NAMES)
def test_loss_cases_match_the_reference_in_both_plans(gold, name):
    """the reference-structured path (BEVFormerHead.loss on CPU tensors) AND the packed composition of the fused kernels
    against the reference's loss dictionary, gradients and assignments"""
    from vidar_amd.plugin.core_bbox import LiDARInstance3DBoxes
    from vidar_amd.plugin.dense_heads import det_ops as D
    data, meta = gold
    case, p, boxes, labels = loss_case(data, meta, name)
    NL, B, Q, counts = 6, case["B"], case["Q"], case["counts"]
    head = build(gold).pts_bbox_head
    want = dict(zip((str(n) for n in data[p + "loss_names"]), data[p + "loss_values"]))
    cls = torch.from_numpy(data[p + "cls"]).requires_grad_(True)
    box = torch.from_numpy(data[p + "box"]).requires_grad_(True)
    got = head.loss([LiDARInstance3DBoxes(b) for b in boxes], labels,
                    dict(all_cls_scores=cls, all_bbox_preds=box, enc_cls_scores=None, enc_bbox_preds=None))
    for k, v in want.items():
        np.testing.assert_allclose(float(got[k].detach()), v, err_msg=k, **LOSS_TOL)
    g = torch.autograd.grad(sum(got.values()), [cls, box])
    grad_close(g[0].numpy(), data[p + "grad_cls"], "grad_cls"); grad_close(g[1].numpy(), data[p + "grad_box"], "grad_box")
    # packed plan
    gt_norm, gt_label = pack(boxes, labels)
    start = torch.from_numpy(D.gt_starts(counts))
    cost = D.match_cost_torch(cls.detach(), box.detach(), gt_norm, gt_label, counts, 0.25, 2.0, 2.0, 0.25)
    matched = D.solve(cost.numpy(), NL, Q, counts)
    assert np.array_equal(matched, data[p + "matched"])
    m = torch.from_numpy(matched)
    sums = D.det_loss_sums_torch(cls, box, D.labels_from_matched(m, gt_label, start, 10), m, gt_norm, start, head.code_weights, 0.25, 2.0)
    pos = max(sum(min(Q, c) for c in counts), 1)
    packed = {}
    for l in range(NL):
        key = "" if l == NL - 1 else f"d{l}."
        packed[key + "loss_cls"] = torch.nan_to_num(sums[l, 0] * 2.0 / pos)
        packed[key + "loss_bbox"] = torch.nan_to_num(sums[l, 1] * 0.25 / pos)
    for k, v in want.items():
        np.testing.assert_allclose(float(packed[k].detach()), v, err_msg="packed " + k, **LOSS_TOL)
    g = torch.autograd.grad(sum(packed.values()), [cls, box])
    grad_close(g[0].numpy(), data[p + "grad_cls"], "packed grad_cls"); grad_close(g[1].numpy(), data[p + "grad_box"], "packed grad_box")


def run_sequence(model, data, meta, device="cpu"):
    out = []
    for t in range(3):
        m = frame_meta(data, prefix=t)
        m.update(can_bus=data[f"test/{t}/can_bus_in"].copy(), lidar2global_rotation=data[f"test/{t}/lidar2global_rotation"], scene_token=meta["test_scene_tokens"][t])
        feats = [torch.from_numpy(data[f"test/{t}/feats0"]).to(device), torch.from_numpy(data[f"test/{t}/feats1"]).to(device)]
        res = model(return_loss=False, img_metas=[[m]], img_feats=[feats])[0]["pts_bbox"]
        out.append((res, model.prev_frame_info["prev_bev"].detach().cpu().numpy()))
    return out


def check_sequence(out, data):
    for t, (res, bev) in enumerate(out):
        np.testing.assert_allclose(bev, data[f"test/{t}/prev_bev_after"], **OUT_TOL)
        assert np.array_equal(res["labels_3d"].numpy(), data[f"test/{t}/labels"])
        np.testing.assert_allclose(res["scores_3d"].numpy(), data[f"test/{t}/scores"], **BOX_TOL)
        np.testing.assert_allclose(res["boxes_3d"].tensor.numpy(), data[f"test/{t}/boxes"], **BOX_TOL)
        assert len(res["scores_3d"]) > 0


def test_video_mode_inference_matches_the_reference_over_two_scenes(gold):
    """3 frames, the third from another scene: prev_bev carry, can_bus delta rewriting, scene-change reset, NMSFreeCoder.decode
    and get_bboxes (bottom-centred z) against the reference's forward_test"""
    from oracle import cpu_ops
    data, meta = gold
    model = build(gold).eval()
    with cpu_ops.patched():
        check_sequence(run_sequence(model, data, meta), data)
