"""GPU: the detection fine-tune recipe fed from an info pkl (the fixture of tests/det_data_cases.py) on the reduced model of
tests/test_data_bridge_gpu.py (small images, BEV 24 x 24).

One item of DetectionSequenceDataset goes through build_dataloader and finish_batch into BEVFormer.forward_train -- boxes and
labels as the host lists the head stages through its pinned arena --, and the same images, metas and boxes are handed over
directly as device tensors: the loss dictionaries are equal BIT FOR BIT (every forward kernel is deterministic; gradients are
not compared, the backward scatters use fp32 atomics).  Once with the host image path and once with device_images=True, which
the project pins to the same tensor.  Then tools/train.py itself on the fixture.

The project's own forward kernels repeat their bits; the library convolutions do not by default.  Measured on an MI355X:
with the default solver choice the 3x3 convolutions of the FPN (`img_neck.fpn_convs.*`, library code) return other bits for
the same input from call to call at this reduced size, and repeated forward_train calls on ONE item then differ in 4 to 9 of
the 12 loss terms by 2.4e-7 .. 1.4e-6 -- between two calls on the very same device tensors as much as between the two
routes.  `torch.backends.cudnn.deterministic = True` is the library's switch for that; the tests of this file run under it
(restored afterwards), and five calls in any order then agree in every bit."""
import copy
import importlib.util
import json
import random
from pathlib import Path

import numpy as np
import pytest
import torch

import det_data_cases as F

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module", autouse=True)
def deterministic_library_convolutions():
    """the convolution library picks order-dependent solvers for the FPN's 3x3 convolutions unless told not to"""
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = before


@pytest.fixture(scope="module")
def ann(tmp_path_factory):
    return F.det_mini_nuscenes(tmp_path_factory.mktemp("det_mini"))


def dataset(ann, **kw):
    from vidar_amd.configs import dataset_kwargs, get_config
    from vidar_amd.data import DetectionSequenceDataset
    return DetectionSequenceDataset(ann, augment=True, **dict(dataset_kwargs(get_config("finetune/vidar_1_8_nusc_1future")), **kw))


@pytest.fixture(scope="module")
def model():
    from vidar_amd import train as T
    from vidar_amd.configs import get_config, set_num_cams
    cfg = get_config("finetune/vidar_1_8_nusc_1future", bev_h=24, bev_w=24, with_backbone=True)
    set_num_cams(cfg["model"], 2)
    cfg["model"]["use_grid_mask"] = False                  # (draws from numpy's generator; pinned in test_grid_mask_cpu)
    torch.manual_seed(1)
    model = T.build_model(cfg)
    for m in model.img_backbone.modules():                 # caffe-style images (+-128) through a random-init backbone
        if isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data.fill_(0.5)
    model.cuda().train()
    model.apply(lambda m: setattr(m, "p", 0.0) if isinstance(m, torch.nn.Dropout) else None)
    for m in model.modules():
        if isinstance(m, torch.nn.MultiheadAttention):
            m.dropout = 0.0
    return model


@pytest.fixture(scope="module")
def direct(ann, model):
    """the item of the HOST image path handed over directly: everything a device tensor -> (item, loss dict)"""
    from vidar_amd.plugin.core_bbox import LiDARInstance3DBoxes
    ds = dataset(ann)
    assert ds.usable_index == [10]
    random.seed(3); np.random.seed(3)
    item = ds[0]
    losses = model(return_loss=True, img=item["img"][None].cuda(), img_metas=[copy.deepcopy(item["img_metas"])],
                   gt_bboxes_3d=[LiDARInstance3DBoxes(item["gt_bboxes_3d"].tensor.cuda())],
                   gt_labels_3d=[item["gt_labels_3d"].cuda()])
    return item, {k: v.detach().clone() for k, v in losses.items()}


@pytest.mark.parametrize("device_images", [False, True])
def test_loader_item_gives_the_losses_of_the_direct_tensors_bit_for_bit(ann, model, direct, device_images):
    from vidar_amd.data.loader import build_dataloader, finish_batch
    item, want = direct
    ds = dataset(ann, device_images=device_images)
    random.seed(3); np.random.seed(3)
    batch = next(iter(build_dataloader(ds, samples_per_gpu=1, workers_per_gpu=0, num_replicas=1, rank=0, seed=0)))
    assert ("img_raw" in batch) == device_images
    batch = finish_batch(batch, torch.device("cuda", 0))
    assert sorted(batch) == ["gt_bboxes_3d", "gt_labels_3d", "img", "img_metas"] and batch["img"].is_cuda
    assert not batch["gt_bboxes_3d"][0].tensor.is_cuda and not batch["gt_labels_3d"][0].is_cuda      # staged by the head
    assert [batch["img_metas"][0][t]["sample_idx"] for t in range(4)] == [item["img_metas"][t]["sample_idx"] for t in range(4)]
    assert torch.equal(batch["gt_bboxes_3d"][0].tensor, item["gt_bboxes_3d"].tensor) and len(item["gt_labels_3d"]) > 3
    assert torch.equal(batch["img"][0].cpu(), item["img"])                                         # host and device path: one tensor
    got = {k: v.detach() for k, v in model(return_loss=True, **batch).items()}
    assert list(got) == list(want) and len(got) == 12
    for k in want:
        print(k, float(got[k]), float(want[k]))
        assert torch.isfinite(got[k]) and torch.equal(got[k], want[k]), k


@pytest.mark.parametrize("device_assign", [False, True])
def test_train_launcher_runs_the_recipe_on_the_info_file(ann, tmp_path, monkeypatch, capsys, device_assign):
    from vidar_amd import gemm_tuning
    from vidar_amd.plugin.dense_heads import det_ops
    monkeypatch.setattr(gemm_tuning, "enable", lambda **kw: {})         # TunableOp is process-wide state: not this test's
    checked = []
    real = det_ops.check_assign_status
    monkeypatch.setattr(det_ops, "check_assign_status", lambda status: (checked.append(status), real(status))[1])
    spec = importlib.util.spec_from_file_location("vidar_tools_train", ROOT / "tools" / "train.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    work = tmp_path / "run"
    argv = ["finetune/vidar_1_8_nusc_1future", "--bev", "24", "24", "--cams", "2", "--ann-file", str(ann), "--workers", "0",
            "--iters", "2", "--work-dir", str(work)] + (["--device-assign", "--device-images"] if device_assign else [])
    try:
        tool.main(argv)
    finally:
        det_ops.set_assign(None)
    assert "finished 2 iterations" in capsys.readouterr().out
    rec = [json.loads(line) for line in (work / "log.jsonl").read_text().splitlines()]
    assert len(rec) == 1 and rec[0]["iter"] == 2 and len([k for k in rec[0] if "loss_" in k]) == 12
    assert all(np.isfinite(v) for k, v in rec[0].items() if "loss" in k) and rec[0]["loss"] > 0
    if device_assign:                                      # the status was read where the log line was written, and was clean
        assert len(checked) == 1 and checked[0] is not None and checked[0].is_cuda and int(checked[0].abs().sum()) == 0
    else:
        assert checked == []
    ckpt = torch.load(work / "latest.pth", map_location="cpu", weights_only=False)
    assert ckpt["meta"]["iter"] == 2 and any(k.startswith("pts_bbox_head.") for k in ckpt["state_dict"])
