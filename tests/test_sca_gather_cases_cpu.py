"""CPU: the restatement of tests/sca_gather_cases.py held to the module's own torch formulation, so that the GPU test
compares csrc/bev_prep.hip with something that is itself pinned: the fp64 projection and tables to
BEVFormerEncoder.point_sampling and visible_query_index on the same inputs, rows32 / combine32 to the advanced index and
index_add that SpatialCrossAttention uses when it is given no plan; and the committed seeds: the redraw loop converges
and leaves every anchor outside the margins, with the cameras as the case describes them."""
import numpy as np
import pytest
import torch

import sca_gather_cases as SC


@pytest.mark.parametrize("Q", SC.PLAN_Q)
def test_anchor_redraw_converges_and_keeps_the_margins(Q):
    ref, rounds = SC.anchors(Q)
    print(f"Q = {Q}: {rounds} redraw rounds")
    assert rounds <= SC.MAX_REDRAWS and ref.shape == (SC.ND, Q, 3) and ref.dtype == torch.float32
    assert float(ref.min()) >= 0.0 and float(ref.max()) <= 1.0
    c = SC.plan_case(Q)
    assert float((c["cz"] - SC.Z_EPS).abs().min()) >= SC.MARGIN
    assert float(SC.border_distance(c["u"], c["v"]).min()) >= SC.MARGIN
    assert not bool(SC.too_close(c["u"], c["v"], c["cz"]).any())


@pytest.mark.parametrize("Q", SC.PLAN_Q)
def test_cameras_are_what_the_case_says(Q):
    c = SC.plan_case(Q)
    vis = c["mask"].any(-1)                                              # [F, N, B, Q]
    per_cam = vis[:, :, 0].sum(-1)                                       # batch item 0
    for f in range(SC.NF):
        assert sorted(per_cam[f].tolist())[0] == 0 and sorted(per_cam[f].tolist())[-1] == Q
    assert not torch.equal(vis[:, :, 0], vis[:, :, 1])                   # the item-0 rule matters
    if Q >= 63:
        assert all(0 < sorted(per_cam[f].tolist())[1] < Q for f in range(SC.NF))      # the third camera is mixed
        pin = c["cz"][0, 1, 1]                                           # frame 0, camera 1, item 1: a pinhole
        assert bool((pin < 0).any()) and bool((pin > 1).any())           # anchors behind it and in front of it
        assert c["count"].unique().numel() >= 2


@pytest.mark.parametrize("Q", SC.PLAN_Q)
def test_tables_equal_the_modules_torch_formulation(Q):
    from vidar_amd.plugin.modules.encoder import BEVFormerEncoder
    from vidar_amd.plugin.modules.spatial_cross_attention import visible_query_index
    c = SC.plan_case(Q)
    ref_b = c["ref_3d"][None].repeat(SC.NB, 1, 1, 1)
    for f in range(SC.NF):
        metas = [dict(lidar2img=[np.asarray(m) for m in c["l2i"][f, b].double().numpy()],
                      img_shape=[(int(SC.IMG_H), int(SC.IMG_W), 3)]) for b in range(SC.NB)]
        ref_cam, mask = BEVFormerEncoder.point_sampling(None, ref_b, SC.PC_RANGE, metas)
        assert torch.equal(mask, c["mask"][f])
        far = c["cz"][f] >= 1.0
        want = torch.stack((c["u"][f], c["v"][f]), -1)
        torch.testing.assert_close(ref_cam.double()[far], want[far], rtol=2e-4, atol=1e-5)
        idx, valid, count = visible_query_index(mask)
        n = idx.shape[1]
        assert n == int(c["lens"][f].max())
        assert torch.equal(valid, c["valid"][f, :, :n].bool())
        assert torch.equal(idx[valid], c["idx"][f, :, :n][valid])
        assert torch.equal(count, c["count"][f])
        # the rest of the contract, which the torch formulation has no word for
        lens = c["lens"][f].long()
        for cam in range(SC.NCAM):
            k, row, inv = int(lens[cam]), c["idx"][f, cam], c["slot_of"][f, cam].long()
            assert torch.equal(row[k:], torch.arange(k, Q)) and row.unique().numel() >= Q - k
            assert bool((row[:k][1:] > row[:k][:-1]).all())
            seen = inv >= 0
            assert int(seen.sum()) == k and torch.equal(row[inv[seen]], torch.nonzero(seen).view(-1))


@pytest.mark.parametrize("case", SC.GATHER_CASES, ids=SC.gather_id)
def test_gathers_equal_the_advanced_index_and_index_add(case):
    B, C, S, with_count = case
    t, d = SC.gather_tables(), SC.gather_inputs(B, C, S)
    idx, valid, slot_of = t["idx"], t["valid"], t["slot_of"]
    count = t["count"][:B] if with_count else None
    vmask = valid[:, :S].bool()[None, :, :, None]
    # rebatch: query[:, idx] * vmask (spatial_cross_attention.py, the path without a plan); finite inputs, for NaN * 0
    x = d["x"] / count[..., None] if with_count else d["x"]
    assert torch.equal(SC.rows32(d["x"], idx, valid, count, S), x[:, idx[:, :S]] * vmask)
    # scatter-back: index_add of the masked rows over the flattened index, then / count; in fp64, where the order of the
    # additions does not show at 1e-12
    y = d["y"].double() * vmask
    slots = torch.zeros(B, SC.GQ, C, dtype=torch.float64)
    for j in range(B):
        slots[j].index_add_(0, idx[:, :S].reshape(-1), y[j].reshape(-1, C))
    if with_count:
        slots = slots / count.double()[..., None]
    got64 = SC.combine32(d["y"].double(), slot_of, count, S)
    torch.testing.assert_close(got64, slots, rtol=1e-12, atol=1e-12)
    # the sequential fp32 form is within its own bound of fp64, and blind to the NaN rows
    got32 = SC.combine32(d["y"], slot_of, count, S)
    assert bool(((got32.double() - got64).abs() <= SC.combine_bound(d["y"], slot_of, count, S)).all())
    assert torch.equal(SC.combine32(d["y_nan"], slot_of, count, S), got32)
    assert torch.equal(SC.rows32(d["x_nan"], idx, valid, count, S), SC.rows32(d["x"], idx, valid, count, S))
    if S:
        assert bool(torch.isnan(d["x_nan"]).any()) and (S < 37 or bool(torch.isnan(d["y_nan"]).any()))


def test_hand_built_tables_are_consistent():
    t = SC.gather_tables()
    assert t["lens"] == [32, 16, 3] and int(t["dead"].sum()) == 5
    for n, k in enumerate(t["lens"]):
        row, inv = t["idx"][n], t["slot_of"][n].long()
        assert bool(t["valid"][n, :k].all()) and not bool(t["valid"][n, k:].any())
        assert bool(t["dead"][row[k:]].all()) and not bool(t["dead"][row[:k]].any())
        assert torch.equal(row[inv[inv >= 0]], torch.nonzero(inv >= 0).view(-1)) and int((inv >= 0).sum()) == k
        assert not torch.equal(row[:k], row[:k].sort().values)            # shuffled: slot != rank
    assert sorted(t["count"].unique().tolist()) == [1.0, 2.0, 3.0]
    # two queries are seen by all three cameras, and there the order of the additions shows: the cameras taken in the
    # order 2, 1, 0 give other bits
    assert int((t["slot_of"] >= 0).all(0).sum()) == 2
    y = SC.gather_inputs(2, 256, 37)["y"]
    assert not torch.equal(SC.combine32(y.flip(1), t["slot_of"].flip(0), None, 37), SC.combine32(y, t["slot_of"], None, 37))
