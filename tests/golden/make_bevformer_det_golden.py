"""Golden vectors for the BEVFormer detection branch from the reference's own source text.

Executed in place (nothing of it is copied here):
  * bevformer/modules/transformer.py (PerceptionTransformer incl. forward), decoder.py (DetectionTransformerDecoder,
    CustomMSDeformableAttention, inverse_sigmoid), custom_base_transformer_layer.py -- imported as modules through
    ref_mmcv_functional.reference_modules();
  * bevformer/dense_heads/bevformer_head.py: the body of class BEVFormerHead (_init_layers, init_weights, forward,
    _get_target_single, get_targets, loss_single, loss, get_bboxes) exec'd inside a throw-away nn.Module (its base class
    DETRHead is mmdet code);
  * core/bbox/util.py, core/bbox/assigners/hungarian_assigner_3d.py, core/bbox/match_costs/match_cost.py,
    core/bbox/coders/nms_free_coder.py -- loaded as files;
  * bevformer/detectors/bevformer.py: forward_pts_train, forward_train, forward_test, simple_test_pts, simple_test exec'd
    inside a throw-away class.
Third party, recalled, unpinned (mmcv / mmdet / mmdet3d cannot be installed): the stand-ins of ref_mmcv_functional.py plus,
below, mmcv's MultiheadAttention wrapper and DetrTransformerDecoderLayer (the reference's MyCustomBaseTransformerLayer
forward with mmcv's batch_first=False), mmdet's FocalLossCost, py_sigmoid_focal_loss-style FocalLoss (the
binary_cross_entropy_with_logits form, NOT the product's formula), L1Loss, PseudoSampler semantics, multi_apply,
reduce_mean (single process), AssignResult, and a minimal LiDARInstance3DBoxes / bbox3d2result.

Writes DATA only: tests/golden/bevformer_det_small.<n>.npz (shards below 1 MiB; inputs, seeded weights by key, outputs, losses, gradients,
assignments, loss-only cases) and bevformer_det_small.json (config, the (name, shape) list of the reference head, case list,
number of unstable cases dropped).  Reduced width: embed 64, 2 heads, BEV 12 x 12, 3 cameras, 6 decoder layers.
    python tests/golden/make_bevformer_det_golden.py"""
import copy
import json
import sys
import types
from functools import partial
from pathlib import Path

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[1]
sys.path.insert(0, str(HERE)); sys.path.insert(0, str(ROOT))
import ref_mmcv_functional as R  # noqa: E402
from make_transformer_golden import BEV, CAMS, D, HEADS, PC, SHAPES, perturb, transformer_cfg  # noqa: E402

NQ, NCLS, NDEC = 12, 10, 6
POST = [-61.2, -61.2, -10.0, 61.2, 61.2, 10.0]
# loss-only cases on seeded predictions: (name, seed, B, Q, ground-truth counts); G = 0, G > Q and G = Q are among them
LOSS_CASES = [("mixed", 1, 2, 30, [7, 12]), ("empty_and_over", 2, 2, 9, [0, 14]), ("square", 3, 1, 12, [12]),
              ("no_gt", 4, 2, 9, [0, 0]), ("single", 5, 1, 20, [1])]


# ------------------------------------------------------------------------------ recalled third-party pieces
class MultiheadAttention(R.BaseModule):
    """[3P] mmcv 1.4.0 wrapper of nn.MultiheadAttention"""

    def __init__(self, embed_dims, num_heads, attn_drop=0., proj_drop=0., dropout_layer=dict(type="Dropout", drop_prob=0.),
                 init_cfg=None, batch_first=False, **kwargs):
        super().__init__(init_cfg)
        if "dropout" in kwargs:
            attn_drop = kwargs["dropout"]
            dropout_layer = dict(dropout_layer, drop_prob=kwargs.pop("dropout"))
        self.embed_dims, self.num_heads, self.batch_first = embed_dims, num_heads, batch_first
        self.attn = nn.MultiheadAttention(embed_dims, num_heads, attn_drop, **kwargs)
        self.proj_drop = nn.Dropout(proj_drop)
        self.dropout_layer = nn.Dropout(dropout_layer["drop_prob"]) if dropout_layer else nn.Identity()

    def forward(self, query, key=None, value=None, identity=None, query_pos=None, key_pos=None, attn_mask=None,
                key_padding_mask=None, **kwargs):
        if key is None:
            key = query
        if value is None:
            value = key
        if identity is None:
            identity = query
        if key_pos is None:
            if query_pos is not None and query_pos.shape == key.shape:
                key_pos = query_pos
        if query_pos is not None:
            query = query + query_pos
        if key_pos is not None:
            key = key + key_pos
        if self.batch_first:
            query, key, value = query.transpose(0, 1), key.transpose(0, 1), value.transpose(0, 1)
        out = self.attn(query=query, key=key, value=value, attn_mask=attn_mask, key_padding_mask=key_padding_mask)[0]
        if self.batch_first:
            out = out.transpose(0, 1)
        return identity + self.dropout_layer(self.proj_drop(out))


def py_sigmoid_focal_loss(pred, target, gamma, alpha):
    """[3P] mmdet py_sigmoid_focal_loss, elementwise"""
    p = pred.sigmoid()
    t = F.one_hot(target, pred.shape[1] + 1)[:, :pred.shape[1]].type_as(pred)
    pt = (1 - p) * t + p * (1 - t)
    w = (alpha * t + (1 - alpha) * (1 - t)) * pt.pow(gamma)
    return F.binary_cross_entropy_with_logits(pred, t, reduction="none") * w


class FocalLoss(nn.Module):
    def __init__(self, use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0):
        super().__init__()
        self.use_sigmoid, self.gamma, self.alpha, self.loss_weight = use_sigmoid, gamma, alpha, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None):
        loss = py_sigmoid_focal_loss(pred, target, self.gamma, self.alpha)
        if weight is not None:
            loss = loss * weight.view(-1, 1)
        return self.loss_weight * loss.sum() / avg_factor


class L1Loss(nn.Module):
    def __init__(self, loss_weight=1.0):
        super().__init__()
        self.loss_weight = loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None):
        if target.numel() == 0:
            return pred.sum() * 0
        return self.loss_weight * ((pred - target).abs() * weight).sum() / avg_factor


class FocalLossCost:
    def __init__(self, weight=1., alpha=0.25, gamma=2, eps=1e-12):
        self.weight, self.alpha, self.gamma, self.eps = weight, alpha, gamma, eps

    def __call__(self, cls_pred, gt_labels):
        cls_pred = cls_pred.sigmoid()
        neg_cost = -(1 - cls_pred + self.eps).log() * (1 - self.alpha) * cls_pred.pow(self.gamma)
        pos_cost = -(cls_pred + self.eps).log() * self.alpha * (1 - cls_pred).pow(self.gamma)
        return (pos_cost[:, gt_labels] - neg_cost[:, gt_labels]) * self.weight


class AssignResult:
    def __init__(self, num_gts, gt_inds, max_overlaps, labels=None):
        self.num_gts, self.gt_inds, self.max_overlaps, self.labels = num_gts, gt_inds, max_overlaps, labels


class PseudoSampler:
    def sample(self, assign_result, bboxes, gt_bboxes):
        pos = torch.nonzero(assign_result.gt_inds > 0, as_tuple=False).squeeze(-1).unique()
        neg = torch.nonzero(assign_result.gt_inds == 0, as_tuple=False).squeeze(-1).unique()
        gi = assign_result.gt_inds[pos] - 1
        return types.SimpleNamespace(pos_inds=pos, neg_inds=neg, pos_assigned_gt_inds=gi,
                                     pos_gt_bboxes=gt_bboxes[gi, :] if gt_bboxes.numel() else gt_bboxes.view(-1, gt_bboxes.shape[-1]))


class Boxes:
    """[3P] LiDARInstance3DBoxes: bottom-centred tensor, gravity_center lifts z by h / 2"""

    def __init__(self, tensor, box_dim=9):
        self.tensor = torch.as_tensor(tensor, dtype=torch.float32).reshape(-1, box_dim)

    @property
    def gravity_center(self):
        c = self.tensor[:, :3].clone()
        c[:, 2] = c[:, 2] + self.tensor[:, 5] * 0.5
        return c

    def to(self, device):
        return self


def multi_apply(func, *args, **kwargs):
    pfunc = partial(func, **kwargs) if kwargs else func
    return tuple(map(list, zip(*map(pfunc, *args))))


# ------------------------------------------------------------------------------ the reference, assembled
MATCHES = []          # (cost matrix fp64 of every assign call, rows, cols) in call order


def reference_stack():
    mods = R.reference_modules()
    dec = sys.modules["refbev.modules.decoder"]
    base = sys.modules["refbev.modules.custom_base_transformer_layer"].MyCustomBaseTransformerLayer
    R.ATTENTION.register_module(module=MultiheadAttention)

    class DetrTransformerDecoderLayer(base):
        """[3P] mmcv: BaseTransformerLayer (the reference's copy of its forward) with batch_first=False"""

        def __init__(self, attn_cfgs, feedforward_channels=None, ffn_dropout=0.0, operation_order=None,
                     act_cfg=dict(type="ReLU", inplace=True), norm_cfg=dict(type="LN"), ffn_num_fcs=2, **kwargs):
            kwargs.setdefault("batch_first", False)
            super().__init__(attn_cfgs=attn_cfgs, operation_order=operation_order, norm_cfg=norm_cfg, **kwargs)
    R.TRANSFORMER_LAYER.register_module(module=DetrTransformerDecoderLayer)

    util = _load("projects.mmdet3d_plugin.core.bbox.util", R.PLUGIN / "core/bbox/util.py", pkgs=True)
    registry = R.Registry("x")
    costs = R.Registry("match cost")
    costs.register_module(module=FocalLossCost)
    R._mod("mmdet.core"); R._mod("mmdet.core.bbox", BaseBBoxCoder=object)
    R._mod("mmdet.core.bbox.builder", BBOX_ASSIGNERS=registry, BBOX_CODERS=registry)
    R._mod("mmdet.core.bbox.assigners", AssignResult=AssignResult, BaseAssigner=object)
    R._mod("mmdet.core.bbox.match_costs", build_match_cost=lambda cfg: R.build_from_cfg(cfg, costs))
    R._mod("mmdet.core.bbox.match_costs.builder", MATCH_COST=costs)
    R._mod("mmdet.models.utils.transformer", inverse_sigmoid=dec.inverse_sigmoid)
    sys.modules["mmcv"].jit = lambda *a, **k: (lambda f: f)
    _load("ref_match_cost", R.PLUGIN / "core/bbox/match_costs/match_cost.py")
    costs.register_module(name="IoUCost", module=type("IoUCost", (), {"__init__": lambda self, weight=0.0: None}))
    assigner_mod = _load("ref_assigner", R.PLUGIN / "core/bbox/assigners/hungarian_assigner_3d.py")
    real_lsa = assigner_mod.linear_sum_assignment

    def recording(cost):
        r, c = real_lsa(cost)
        MATCHES.append((np.asarray(cost, dtype=np.float64).copy(), r.copy(), c.copy()))
        return r, c
    assigner_mod.linear_sum_assignment = recording
    coder_mod = _load("ref_coder", R.PLUGIN / "core/bbox/coders/nms_free_coder.py")

    ident = lambda *a, **k: (lambda f: f)
    ns = dict(copy=copy, torch=torch, nn=nn, Linear=nn.Linear, bias_init_with_prob=sys.modules["mmcv.cnn"].bias_init_with_prob,
              TORCH_VERSION=torch.__version__, digit_version=sys.modules["mmcv.utils"].digit_version, multi_apply=multi_apply,
              reduce_mean=lambda t: t, inverse_sigmoid=dec.inverse_sigmoid, normalize_bbox=util.normalize_bbox,
              force_fp32=ident, auto_fp16=ident)
    src = (R.PLUGIN / "bevformer/dense_heads/bevformer_head.py").read_text()
    a = src.index("    def _init_layers(self):")
    b = src.index("@HEADS.register_module()\nclass BEVFormerHead_GroupDETR")
    exec("class RefHead(torch.nn.Module):\n" + src[a:b], ns)
    dsrc = (R.PLUGIN / "bevformer/detectors/bevformer.py").read_text()
    c = dsrc.index("    def forward_pts_train(")
    d = dsrc.index("    def forward_dummy(")
    e = dsrc.index("    @auto_fp16(apply_to=('img', 'points'))\n    def forward_train(")
    ns2 = dict(torch=torch, copy=copy, np=np, auto_fp16=ident,
               bbox3d2result=lambda b, s, l: dict(boxes_3d=b.tensor, scores_3d=s, labels_3d=l))
    exec("class RefDet(torch.nn.Module):\n" + dsrc[c:d] + "\n" + dsrc[e:], ns2)
    return ns["RefHead"], ns2["RefDet"], assigner_mod.HungarianAssigner3D, coder_mod.NMSFreeCoder


def _load(name, path, pkgs=False):
    import importlib.util
    if pkgs:
        parts = name.split(".")
        for i in range(1, len(parts)):
            if ".".join(parts[:i]) not in sys.modules:
                R._mod(".".join(parts[:i])).__path__ = []
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def head_cfg():
    t = transformer_cfg()
    t["decoder"] = dict(
        type="DetectionTransformerDecoder", num_layers=NDEC, return_intermediate=True,
        transformerlayers=dict(type="DetrTransformerDecoderLayer",
                               attn_cfgs=[dict(type="MultiheadAttention", embed_dims=D, num_heads=HEADS, dropout=0.1),
                                          dict(type="CustomMSDeformableAttention", embed_dims=D, num_heads=HEADS, num_levels=1)],
                               ffn_cfgs=dict(type="FFN", embed_dims=D, feedforward_channels=128, num_fcs=2, ffn_drop=0.1,
                                             act_cfg=dict(type="ReLU", inplace=True)),
                               feedforward_channels=128, ffn_dropout=0.1,
                               operation_order=("self_attn", "norm", "cross_attn", "norm", "ffn", "norm")))
    return dict(type="BEVFormerHead", bev_h=BEV, bev_w=BEV, num_query=NQ, num_classes=NCLS, in_channels=D,
                sync_cls_avg_factor=True, with_box_refine=True, as_two_stage=False, transformer=t,
                bbox_coder=dict(type="NMSFreeCoder", post_center_range=POST, pc_range=PC, max_num=20, voxel_size=[0.2, 0.2, 8],
                                num_classes=NCLS),
                positional_encoding=dict(type="LearnedPositionalEncoding", num_feats=D // 2, row_num_embed=BEV, col_num_embed=BEV),
                loss_cls=dict(type="FocalLoss", use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=2.0),
                loss_bbox=dict(type="L1Loss", loss_weight=0.25), loss_iou=dict(type="GIoULoss", loss_weight=0.0))


ASSIGNER = dict(type="HungarianAssigner3D", cls_cost=dict(type="FocalLossCost", weight=2.0),
                reg_cost=dict(type="BBox3DL1Cost", weight=0.25), iou_cost=dict(type="IoUCost", weight=0.0), pc_range=PC)


def model_cfg():
    return dict(type="BEVFormer", use_grid_mask=False, video_test_mode=True, backwarded_prev_frame_num=0,
                pts_bbox_head=head_cfg(), train_cfg=dict(pts=dict(assigner=ASSIGNER)))


def build_head(RefHead, Assigner, Coder, num_query=NQ):
    cfg = head_cfg()
    h = RefHead()
    h.bev_h = h.bev_w = BEV
    h.with_box_refine, h.as_two_stage = True, False
    h.num_reg_fcs, h.embed_dims, h.code_size = 2, D, 10
    h.num_classes = h.cls_out_channels = NCLS
    h.num_query = num_query
    h.bg_cls_weight, h.sync_cls_avg_factor = 0, True
    h.pc_range = PC
    h.real_w, h.real_h = PC[3] - PC[0], PC[4] - PC[1]
    h.bbox_coder = Coder(pc_range=PC, voxel_size=[0.2, 0.2, 8], post_center_range=POST, max_num=20, num_classes=NCLS)
    h.loss_cls, h.loss_bbox = FocalLoss(True, 2.0, 0.25, 2.0), L1Loss(0.25)
    h.assigner = Assigner(cls_cost=ASSIGNER["cls_cost"], reg_cost=ASSIGNER["reg_cost"], iou_cost=ASSIGNER["iou_cost"], pc_range=PC)
    h.sampler = PseudoSampler()
    h.positional_encoding = R.build_from_cfg(cfg["positional_encoding"], R.POSITIONAL_ENCODING)
    h.transformer = R.build_from_cfg(cfg["transformer"], R.TRANSFORMER)
    h._init_layers()
    h.code_weights = nn.Parameter(torch.tensor([1.0] * 8 + [0.2] * 2), requires_grad=False)
    h.init_weights()
    return h


def stable(cost, rows, cols, seeds=(0, 1, 2, 3)):
    """the assignment survives +-1e-4 relative noise on the fp64 cost matrix"""
    from scipy.optimize import linear_sum_assignment
    for s in seeds:
        noise = 1 + 1e-4 * (2 * np.random.default_rng(s).random(cost.shape) - 1)
        r, c = linear_sum_assignment(cost * noise)
        if not (np.array_equal(r, rows) and np.array_equal(c, cols)):
            return False
    return True


def matched_of(calls, Q):
    out = []
    for cost, rows, cols in calls:
        m = np.full(Q, -1, np.int32)
        m[rows] = cols
        out.append(m)
    return out


def main():
    from vidar_amd.synthetic import boxes_3d, make_sample
    RefHead, RefDet, Assigner, Coder = reference_stack()
    torch.manual_seed(0); np.random.seed(0)
    head = build_head(RefHead, Assigner, Coder)
    perturb(head, seed=6)
    for m in head.modules():
        if isinstance(m, nn.Dropout):
            m.p = 0.0
        if isinstance(m, nn.MultiheadAttention):
            m.dropout = 0.0
    out = {}
    meta_json = dict(cfg=model_cfg(), head_state_dict=[[k, list(v.shape)] for k, v in sorted(head.state_dict().items())])
    out.update({"sd/pts_bbox_head." + k: v.detach().numpy() for k, v in head.state_dict().items()})

    # ---- training step: one sample, previous BEV given, 5 boxes ---------------------------------------------------
    metas = make_sample(0, rays_per_frame=1, num_cams=CAMS)[0]
    g = torch.Generator().manual_seed(3)
    feats = [torch.randn(1, CAMS, D, h, w, generator=g) for h, w in SHAPES]
    prev_bev = torch.randn(1, BEV * BEV, D, generator=g)
    dropped = 0
    seed = 40
    while True:                                   # re-seed the boxes until all six assignments are stable
        boxes, labels = boxes_3d(seed, num=5, nan_velocity_rate=0.0)
        boxes[1, 7:] = np.nan                     # one target without a velocity estimate (bevformer_head.py:383)
        head.train()
        del MATCHES[:]
        preds = head(feats, [metas[2]], prev_bev)
        losses = head.loss([Boxes(boxes)], [torch.from_numpy(labels)], preds, img_metas=[metas[2]])
        if all(stable(*m) for m in MATCHES):
            break
        dropped += 1; seed += 1
    params = dict(head.named_parameters())
    names = [n for n, p in params.items() if p.requires_grad]
    grads = torch.autograd.grad(sum(losses.values()), [params[n] for n in names], allow_unused=True)
    out.update(feats0=feats[0].numpy(), feats1=feats[1].numpy(), prev_bev=prev_bev.numpy(), train_boxes=boxes, train_labels=labels,
               train_boxes_seed=np.array(seed), all_cls_scores=preds["all_cls_scores"].detach().numpy(),
               all_bbox_preds=preds["all_bbox_preds"].detach().numpy(), bev_embed=preds["bev_embed"].detach().numpy(),
               loss_names=np.array(sorted(losses)), loss_values=np.array([float(losses[k]) for k in sorted(losses)]),
               train_matched=np.stack(matched_of(MATCHES, NQ)),
               grad_names=np.array([n for n, gr in zip(names, grads) if gr is not None]))
    out.update({"grad/pts_bbox_head." + n: gr.numpy() for n, gr in zip(names, grads) if gr is not None})
    meta_json["params_without_gradient"] = [n for n, gr in zip(names, grads) if gr is None]
    for k in ("can_bus", "lidar2global_rotation"):
        out["meta2_" + k] = np.asarray(metas[2][k])
    out["lidar2img"] = np.stack(metas[2]["lidar2img"]); out["img_shape"] = np.asarray(metas[2]["img_shape"])

    # ---- loss-only cases on seeded predictions (reference loss / assigner, NDEC layers) ----------------------------
    cases = []
    for name, seed, B, Q, counts in LOSS_CASES:
        tries = 0
        while True:
            gg = torch.Generator().manual_seed(seed * 100 + tries)
            cls = (torch.randn(NDEC, B, Q, NCLS, generator=gg) * 2 - 2).requires_grad_(True)
            box = torch.randn(NDEC, B, Q, 10, generator=gg).requires_grad_(True)
            bl = [boxes_3d(seed * 1000 + tries * 10 + b, num=n, nan_velocity_rate=0.2) for b, n in enumerate(counts)]
            head.num_query = Q
            del MATCHES[:]
            ld = head.loss([Boxes(b) for b, _ in bl], [torch.from_numpy(l) for _, l in bl],
                           dict(all_cls_scores=cls, all_bbox_preds=box, enc_cls_scores=None, enc_bbox_preds=None))
            if all(stable(*m) for m in MATCHES):
                break
            dropped += 1; tries += 1
        gc, gb = torch.autograd.grad(sum(ld.values()), [cls, box])
        # assign() returns early for G = 0: rebuild [NDEC, B, Q] with -1 rows there
        it = iter(matched_of(MATCHES, Q))
        matched = np.stack([np.stack([next(it) if counts[b] else np.full(Q, -1, np.int32) for b in range(B)]) for _ in range(NDEC)])
        p = f"case/{name}/"
        out.update({p + "cls": cls.detach().numpy(), p + "box": box.detach().numpy(), p + "grad_cls": gc.numpy(), p + "grad_box": gb.numpy(),
                    p + "matched": matched, p + "loss_names": np.array(sorted(ld)),
                    p + "loss_values": np.array([float(ld[k]) for k in sorted(ld)])})
        for b, (bx, lb) in enumerate(bl):
            out[p + f"boxes{b}"] = bx; out[p + f"labels{b}"] = lb
        cases.append(dict(name=name, B=B, Q=Q, counts=counts, problems=NDEC * sum(1 for c in counts if c)))
    head.num_query = NQ
    meta_json.update(loss_cases=cases, unstable_cases_dropped=dropped,
                     stable_problems=NDEC + sum(c["problems"] for c in cases))
    assert meta_json["stable_problems"] >= 6

    # ---- video-mode inference: 3 frames, 2 scenes (bevformer.py:291-347) --------------------------------------------
    det = RefDet()
    det.pts_bbox_head = head
    det.video_test_mode = True
    det.prev_frame_info = dict(prev_bev=None, scene_token=None, prev_pos=0, prev_angle=0)
    seq_feats = [[torch.randn(1, CAMS, D, h, w, generator=g) for h, w in SHAPES] for _ in range(3)]
    det.extract_feat = lambda img, img_metas=None: img                      # the "image" IS the feature pyramid
    det.eval()
    poses = ([10.0, 5.0, 0.0, 30.0], [11.0, 5.5, 0.0, 33.0], [50.0, 9.0, 0.0, 90.0])
    for t in range(3):
        m = copy.deepcopy(metas[t + 1])
        m["can_bus"][:3], m["can_bus"][-1] = poses[t][:3], poses[t][3]
        m["scene_token"] = "scene a" if t < 2 else "scene b"
        m["box_type_3d"] = Boxes
        can_bus_in = m["can_bus"].copy()                       # absolute ego pose, as the data pipeline hands it over
        with torch.no_grad():
            res = det.forward_test([[m]], img=[seq_feats[t]])[0]["pts_bbox"]
        out.update({f"test/{t}/boxes": res["boxes_3d"].numpy(), f"test/{t}/scores": res["scores_3d"].numpy(),
                    f"test/{t}/labels": res["labels_3d"].numpy(), f"test/{t}/feats0": seq_feats[t][0].numpy(),
                    f"test/{t}/feats1": seq_feats[t][1].numpy(), f"test/{t}/can_bus_in": can_bus_in,
                    f"test/{t}/lidar2global_rotation": np.asarray(m["lidar2global_rotation"]),
                    f"test/{t}/prev_bev_after": det.prev_frame_info["prev_bev"].numpy()})
    meta_json["test_scene_tokens"] = ["scene a", "scene a", "scene b"]

    # shards below the repository's size limit for one file: greedy fill in key order, bevformer_det_small.<n>.npz
    for f in HERE.glob("bevformer_det_small.*.npz"):
        f.unlink()
    shard, size, n = {}, 0, 0
    for k, v in out.items():
        v = np.asarray(v)
        if shard and size + v.nbytes > 800 * 1024:
            np.savez_compressed(HERE / f"bevformer_det_small.{n}.npz", **shard)
            shard, size, n = {}, 0, n + 1
        shard[k] = v; size += v.nbytes
    np.savez_compressed(HERE / f"bevformer_det_small.{n}.npz", **shard)
    meta_json["shards"] = n + 1
    (HERE / "bevformer_det_small.json").write_text(json.dumps(meta_json, indent=1))
    print("wrote bevformer_det_small.*.npz / .json:", {k: round(float(v), 5) for k, v in losses.items()}, "dropped", dropped,
          "problems", meta_json["stable_problems"], "no grad:", meta_json["params_without_gradient"])


if __name__ == "__main__":
    main()
