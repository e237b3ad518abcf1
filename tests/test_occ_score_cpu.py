"""CPU: the occupancy score without a GPU -- the per-voxel decisions and the beam weight of csrc/occ_score_math.h through a
stand-alone host program against the torch restatement (tests/occ_score_cases.py), forecast.occupancy_metrics and
evaluate.occupancy_summary on hand-worked tables, and the argument checks of the entry points."""
import ctypes
import math
import os
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import occ_score_cases as OC
import ray_stats_cases as RS

ROOT = Path(__file__).resolve().parents[1]
NAN = float("nan")


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("occ_score_host") / "occ_score_host"
    base = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", f"-I{ROOT / 'vidar_amd' / 'csrc'}",
            str(ROOT / "tests" / "occ_score_host.cpp"), "-o", str(exe)]
    # a stand-alone program with its own main: the host sanitizers apply when the toolchain ships their runtimes
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.run(base, check=True)
    return exe


def run_host(exe, tmp_path, planes, thresholds, bins, floors, L, K, step):
    V, T, R = planes.shape[1], len(thresholds), len(L)
    blob = struct.pack("<5i", V, T, bins, R, K) + struct.pack("<4f", *floors, step)
    blob += np.asarray(thresholds, np.float32).tobytes() + planes.astype(np.float32).tobytes()
    blob += np.asarray(L, np.float32).tobytes()
    (tmp_path / "in.bin").write_bytes(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True,
                         env=env)
    assert run.returncode == 0, run.stderr[-2000:]
    raw = (tmp_path / "out.bin").read_bytes()
    ncols = OC.columns(T, bins)
    sizes = [(np.float64, ncols), (np.int32, V), (np.float32, V), (np.float32, R * K), (np.int32, R)]
    out, at = [], 0
    for dt, n in sizes:
        out.append(np.frombuffer(raw, dtype=dt, count=n, offset=at))
        at += n * np.dtype(dt).itemsize
    assert at == len(raw)
    return out


@pytest.mark.parametrize("thresholds,bins", [((0.25,), 0), ((0.25, 0.5, 0.25), 10), ((0.0, 0.125, 0.25, 0.3, 0.5, 0.5, 0.75, 1.0), 16)],
                         ids=["T1-B0", "T3-B10", "T8-B16"])
def test_header_against_the_torch_restatement(host_program, tmp_path, thresholds, bins):
    pred, meas = OC.lattice(1, 2079, seed=11)
    floor, hits, th = OC.on_a_boundary(pred, meas, thresholds)
    assert floor > 0 and hits > 0 and th > 0                          # values sit exactly on every kind of boundary
    for plane, bad in enumerate((NAN, math.inf, -math.inf, NAN)):      # one voxel per plane: hit_p, free_p, hit_m, free_m
        (pred if plane < 2 else meas)[0, plane % 2, 100 + 7 * plane] = bad
    planes = torch.cat([pred[0], meas[0]]).numpy()
    floors = (0.5, 0.5, 0.125)
    rng = np.random.default_rng(2)
    step, K = 0.25, 65
    L = np.concatenate([0.5 + 30.0 * rng.uniform(0, 1, 60), [0.125, 0.25, 0.375, 16.25, 16.125, 16.375, 1e-30, 3e38]])
    table, flags, o_p, a, trips = run_host(host_program, tmp_path, planes, thresholds, bins, floors, L, K, step)

    want = OC.table(pred, meas, thresholds, bins)[0].numpy()
    print("table", table.tolist())
    assert np.array_equal(np.delete(table, 4), np.delete(want, 4))    # every count, exactly
    assert abs(table[4] - want[4]) <= 1e-12 * want[4] and want[4] > 0
    v = OC.classify(pred, meas, *floors)
    for bit, key in enumerate(("pred_ok", "meas_ok", "both", "y")):
        assert np.array_equal((flags >> bit) & 1, v[key][0].numpy().astype(np.int32)), key
    both = v["both"][0].numpy()
    assert np.array_equal(o_p[both], v["o_p"][0].numpy()[both])       # fp32 division: the same bits
    assert int(((flags >> 4) & 1).sum()) == 2079 - 4 and not (flags[[100, 107, 114, 121]] & 7).any()

    # the beam weight: fp32, operation for operation
    Lt = torch.from_numpy(L.astype(np.float32))
    d = (torch.arange(K, dtype=torch.float32) + 0.5) * step
    want_a = ((Lt.view(-1, 1) - d.view(1, -1)) / step).clamp(0, 1).numpy()
    a = a.reshape(len(L), K)
    assert np.array_equal(a, want_a)
    n_adding = (want_a > 0).sum(1)
    for r in range(len(L)):
        assert n_adding[r] <= trips[r] <= min(K, n_adding[r] + 2), (r, L[r], trips[r], n_adding[r])
        assert not a[r, trips[r]:].any()                              # nothing that adds is left out of the march
    assert trips[-1] == K and trips[-2] == 1 and a[-2].max() == 0.0


# ---- occupancy_metrics / occupancy_summary -----------------------------------------------------------------------------
HAND = [10, 8, 4, 2, 1.0,   2, 1, 0,   0, 0, 2,   3, 1,   1, 1]           # T = 2 (0.25, 0.5), B = 2


def test_metrics_of_a_hand_worked_table():
    from vidar_amd import forecast as FC
    assert FC.occupancy_columns((0.25, 0.5), 2) == ["n_pred", "n_meas", "n_both", "n_occ", "brier", "tp@0.25", "fp@0.25",
                                                    "fn@0.25", "tp@0.5", "fp@0.5", "fn@0.5", "cnt.0", "pos.0", "cnt.1", "pos.1"]
    m = FC.occupancy_metrics(torch.tensor([HAND], dtype=torch.float64), (0.25, 0.5), 2)
    assert (m["n_pred"], m["n_meas"], m["n_both"], m["n_occ"]) == (10.0, 8.0, 4.0, 2.0)
    assert m["coverage"] == 0.5 and m["brier"] == 0.25
    assert m["iou"] == [2 / 3, 0.0] and m["recall"] == [1.0, 0.0]
    assert m["precision"][0] == 2 / 3 and math.isnan(m["precision"][1])   # nothing called occupied at 0.5: 0 / 0
    assert m["reliability"] == dict(cnt=[3.0, 1.0], freq=[1 / 3, 1.0])
    # leading dimensions are summed: [bs, F, columns]
    stacked = torch.tensor([[HAND, HAND], [HAND, [0] * 15]], dtype=torch.float64)
    m3 = FC.occupancy_metrics(stacked, (0.25, 0.5), 2)
    assert m3["n_both"] == 12.0 and m3["iou"] == m["iou"] and m3["brier"] == 0.25
    # every denominator zero
    z = FC.occupancy_metrics(np.zeros((1, 15)), (0.25, 0.5), 2)
    assert all(math.isnan(z[k]) for k in ("coverage", "brier"))
    assert all(math.isnan(x) for k in ("iou", "precision", "recall") for x in z[k])
    assert all(math.isnan(x) for x in z["reliability"]["freq"]) and z["reliability"]["cnt"] == [0.0, 0.0]
    with pytest.raises(ValueError):
        FC.occupancy_metrics(np.zeros((1, 14)), (0.25, 0.5), 2)
    with pytest.raises(ValueError):
        FC.occupancy_metrics(np.zeros((1, 5)), (), 0)
    with pytest.raises(ValueError):
        FC.occupancy_columns((0.25, NAN), 2)


def test_summary_equals_pooling_the_raw_counts():
    from vidar_amd import evaluate as E
    from vidar_amd import forecast as FC
    th, bins = (0.125, 0.25, 0.5), 10
    names = FC.occupancy_columns(th, bins)
    rng = np.random.default_rng(4)
    tables = rng.integers(0, 50, size=(3, 2, len(names))).astype(np.float64)       # three samples, two frames
    tables[..., 4] = rng.uniform(0, 9, size=(3, 2))
    tables[:, 1, 5:8] = 0                                                           # frame 1: IoU at 0.125 is 0 / 0
    results = [{f"frame.{f}": dict(count=1, chamfer_distance=1.0 + s, l1_error=0.5, absrel_error=0.25,
                                   **{f"occ.{n}": float(v) for n, v in zip(names, tables[s, f])}) for f in range(2)}
               for s in range(3)]
    plain = E.summarize([{k: {m: v for m, v in d.items() if not m.startswith("occ.")} for k, d in r.items()}
                         for r in results])
    summary = E.summarize(results)
    for k in plain:                                                   # the additive entries leave the others alone
        assert all(summary[k][m] == plain[k][m] for m in plain[k])
    occ = E.occupancy_summary(summary)
    assert sorted(occ) == ["frame.0", "frame.1"] and E.occupancy_summary(plain) == {}
    for f in range(2):
        want = FC.occupancy_metrics(tables[:, f], th, bins)
        got = occ[f"frame.{f}"]
        assert got["thresholds"] == list(th)
        for k in ("coverage", "brier"):
            assert got[k] == pytest.approx(want[k], rel=1e-12)
        for k in ("iou", "precision", "recall"):
            assert got[k] == pytest.approx(want[k], rel=1e-12, nan_ok=True)
        assert got["reliability"]["freq"] == pytest.approx(want["reliability"]["freq"], rel=1e-12, nan_ok=True)
        assert got["n_both"] == pytest.approx(want["n_both"] / 3, rel=1e-12)        # a mean per sample, as every entry
    assert math.isnan(occ["frame.1"]["iou"][0]) and not math.isnan(occ["frame.0"]["iou"][0])
    assert "occupancy" in E.format_occupancy(occ) and "iou" in E.format_occupancy(occ)


def test_the_switch(monkeypatch):
    from vidar_amd.plugin.utils import eval_utils
    monkeypatch.delenv("VIDAR_OCC_METRICS", raising=False)
    assert eval_utils.occupancy_metrics() is None                     # off by default
    monkeypatch.setenv("VIDAR_OCC_METRICS", "1")
    assert eval_utils.occupancy_metrics() == {}
    prev = eval_utils.set_occupancy_metrics(False)
    try:
        assert prev is None and eval_utils.occupancy_metrics() is None
        eval_utils.set_occupancy_metrics(True, thresholds=(0.3,), min_evidence=None, bins=4)
        assert eval_utils.occupancy_metrics() == dict(thresholds=(0.3,), bins=4)
        with pytest.raises(TypeError):
            eval_utils.set_occupancy_metrics(True, threshold=0.3)
    finally:
        eval_utils.set_occupancy_metrics(None)
    monkeypatch.setenv("VIDAR_OCC_METRICS", "0")
    assert eval_utils.occupancy_metrics() is None


# ---- argument checks, no GPU -------------------------------------------------------------------------------------------
def test_entry_points_check_their_arguments():
    from vidar_amd._lib import BAD_ARG, lib
    L = lib()
    nbytes = ctypes.c_int64(-1)
    out = ctypes.addressof(nbytes)
    assert L.vidar_occ_score_workspace_bytes(3, 100003, 2, 10, out) == 0
    assert nbytes.value == 3 * 25 * (5 + 6 + 20) * 8                  # 25 tiles of 4096 voxels
    assert L.vidar_occ_score_workspace_bytes(0, 0, 1, 0, out) == 0 and nbytes.value == 0
    for S, V, T, B in ((-1, 1, 1, 0), (1, -1, 1, 0), (1, 1, 0, 0), (1, 1, 9, 0), (1, 1, 1, -1), (1, 1, 1, 17), (65536, 1, 1, 0)):
        assert L.vidar_occ_score_workspace_bytes(S, V, T, B, out) == BAD_ARG, (S, V, T, B)
    assert L.vidar_occ_score_workspace_bytes(1, 1, 1, 0, None) == BAD_ARG

    th = (ctypes.c_float * 2)(0.25, 0.5)
    nan_th = (ctypes.c_float * 2)(0.25, NAN)
    tp, fake = ctypes.addressof(th), 4096                             # `fake`: never dereferenced -- every call below
    score = lambda pred, meas, t, table, S, V, T, B, ws, wsn, floors=(0.5, 0.5, 0.125): \
        L.vidar_occ_score_f32(pred, meas, t, table, S, V, T, B, *floors, ws, wsn, None)     # returns before a launch
    assert score(None, None, tp, None, 0, 100, 2, 10, None, 0) == 0   # nothing to score: no launch, nothing needed
    assert score(None, None, tp, None, 4, 0, 2, 10, None, 0) == 0
    assert score(fake, fake, ctypes.addressof(nan_th), fake, 1, 100, 2, 10, fake, 1 << 20) == BAD_ARG
    assert score(fake, fake, tp, fake, 1, 100, 2, 10, fake, 1 << 20, floors=(NAN, 0.5, 0.125)) == BAD_ARG
    assert score(fake, fake, None, fake, 1, 100, 2, 10, fake, 1 << 20) == BAD_ARG
    for T, B in ((0, 10), (9, 10), (2, 17), (2, -1)):
        assert score(fake, fake, tp, fake, 1, 100, T, B, fake, 1 << 20) == BAD_ARG
    for S, V in ((-1, 100), (1, -100)):
        assert score(fake, fake, tp, fake, S, V, 2, 10, fake, 1 << 20) == BAD_ARG
    need = 31 * 8
    for pred, meas, table, ws, wsn in ((None, fake, fake, fake, need), (fake, None, fake, fake, need),
                                       (fake, fake, None, fake, need), (fake, fake, fake, None, need),
                                       (fake, fake, fake, fake, need - 8), (fake, fake, fake, fake + 4, need),
                                       (fake, fake, fake + 4, fake, need)):
        assert score(pred, meas, tp, table, 1, 100, 2, 10, ws, wsn) == BAD_ARG

    sweep = lambda F_, R, Z, Y, X, K: L.vidar_sweep_evidence_f32(fake, fake, fake, fake, fake, F_, R, Z, Y, X, K, 1.0,
                                                                 None, 0, None)
    for dims in ((0, 4, 4, 10, 96, 64), (2, -1, 4, 10, 96, 64), (2, 4, 0, 10, 96, 64), (2, 4, 4, 10, 96, 0),
                 (2, 4, 4, 10, 96, L.vidar_ray_max_k() + 1)):
        assert sweep(*dims) == BAD_ARG, dims


def test_wrappers_have_no_cpu_path():
    from vidar_amd import forecast as FC
    from vidar_amd.plugin.dense_heads import ray_ops
    grid = torch.zeros(1, 2, 2, 4, 4, 4)
    with pytest.raises(RuntimeError):
        FC.occupancy_score(grid, grid)
    origin, pts, tindex = RS.rays()
    with pytest.raises(RuntimeError):
        ray_ops.sweep_evidence(origin, pts, tindex, (RS.F_, RS.Z, RS.Y, RS.X))
