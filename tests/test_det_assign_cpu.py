"""CPU: the assignment solver of csrc/det_assign_math.h (the body of the kernel of csrc/det_assign.hip) through the
stand-alone host program tests/det_assign_host.cpp, against scipy.optimize.linear_sum_assignment: exact assignments on
continuous costs, equal totals on exact ties, lane-count independence, SciPy's two refusals as status codes; the entry
points' argument checks and the switch of det_ops, none of which needs a GPU."""
import math
import os
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

from test_bevformer_det_cpu import CASES, tail_case

ROOT = Path(__file__).resolve().parents[1]
ARGS = (0.25, 2.0, 2.0, 0.25)           # alpha, gamma, cls_weight, reg_weight of the released configs
# (seed, NL, B, Q, C, counts): the full-size shapes of the fine-tune step
LARGE = [(137, 1, 1, 900, 10, [37]), (250, 1, 2, 900, 10, [150, 37]), (612, 1, 1, 900, 10, [512])]


def build_host_program(directory):
    exe = Path(directory) / "det_assign_host"
    base = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", f"-I{ROOT / 'vidar_amd' / 'csrc'}",
            str(ROOT / "tests" / "det_assign_host.cpp"), "-o", str(exe)]
    # a stand-alone program with its own main: the host sanitizers apply when the toolchain ships their runtimes
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.run(base, check=True)
    return exe


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    return build_host_program(tmp_path_factory.mktemp("det_assign_host"))


def run_host(exe, tmp, cost, NL, Q, counts, lanes=64, transpose=1, raw=False):
    """cost [NL, Q * total_g] float32 (numpy) -> matched [NL, B, Q], status [NL * B] of the host program"""
    from vidar_amd.plugin.dense_heads import det_ops as D
    B, total = len(counts), int(sum(counts))
    cost = np.ascontiguousarray(cost, dtype=np.float32).reshape(NL, Q * total)
    blob = struct.pack("<4i", NL, B, Q, total) + D.gt_starts(counts).astype("<i4").tobytes() + cost.tobytes()
    src, dst = Path(tmp) / "assign_in.bin", Path(tmp) / f"assign_out_{lanes}_{transpose}.bin"
    src.write_bytes(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe), str(src), str(dst), str(lanes), str(transpose)], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stderr[-2000:]
    data = dst.read_bytes()
    if raw:
        return data
    out = np.frombuffer(data, dtype=np.int32)
    assert out.size == NL * B * Q + NL * B
    return out[:NL * B * Q].reshape(NL, B, Q).copy(), out[NL * B * Q:].copy()


def case_cost(seed, NL, B, Q, C, counts):
    from vidar_amd.plugin.dense_heads import det_ops as D
    c = tail_case(seed, NL, B, Q, C, counts)
    c["gt_label"] = c["gt_label"] % C
    return D.match_cost_torch(c["cls"], c["box"], c["gt_norm"], c["gt_label"], counts, *ARGS).numpy()


def problem_blocks(cost, NL, Q, counts):
    from vidar_amd.plugin.dense_heads import det_ops as D
    start = D.gt_starts(counts)
    for l in range(NL):
        for b, G in enumerate(counts):
            yield l, b, G, cost[l, Q * int(start[b]):Q * int(start[b + 1])].reshape(Q, G)


def check_every_problem(matched, status, cost, NL, Q, counts):
    """count and distinctness as check_cost of test_bevformer_det_gpu.py has them, and the total against SciPy's:
    |total - SciPy total| <= 1e-9 * max(1, |total|) under math.fsum -- fp64 eps (1.1e-16) x ~1e4 dual updates x costs of
    order 1e2 is ~1e-10; the bound leaves 10 x over that"""
    assert matched.shape == (NL, len(counts), Q) and matched.dtype == np.int32
    assert not status.any()
    for l, b, G, blk in problem_blocks(cost, NL, Q, counts):
        m = matched[l, b]
        assert int((m >= 0).sum()) == min(Q, G) and len(set(m[m >= 0].tolist())) == min(Q, G)
        assert m.max(initial=-1) < max(G, 1) and m.min(initial=-1) >= -1
        if G:
            rows, cols = linear_sum_assignment(blk)
            best = math.fsum(blk[rows, cols].astype(np.float64))
            got = math.fsum(blk[np.nonzero(m >= 0)[0], m[m >= 0]].astype(np.float64))
            print(f"problem ({l}, {b}) {Q} x {G}: total {got!r}  SciPy {best!r}  difference {got - best:.3e}")
            assert abs(got - best) <= 1e-9 * max(1.0, abs(got)), (l, b, got, best)


@pytest.mark.parametrize("case", CASES + LARGE, ids=[f"seed{c[0]}-Q{c[3]}-G{'_'.join(map(str, c[5]))}" for c in CASES + LARGE])
def test_continuous_costs_give_scipys_assignment(host_program, tmp_path, case):
    from vidar_amd.plugin.dense_heads import det_ops as D
    seed, NL, B, Q, C, counts = case
    counts = [min(n, 40) for n in counts] if Q < 900 else counts
    cost = case_cost(seed, NL, B, Q, C, counts)
    matched, status = run_host(host_program, tmp_path, cost, NL, Q, counts)
    check_every_problem(matched, status, cost, NL, Q, counts)
    assert np.array_equal(matched, D.solve(cost, NL, Q, counts))


@pytest.mark.parametrize("shape", [(40, 17), (17, 40)], ids=["40x17", "17x40"])
def test_exact_ties_give_scipys_total(host_program, tmp_path, shape):
    """integer costs 0..3: many optimal assignments; two correct solvers differ, so only the total is pinned"""
    Q, G = shape
    seeds = 5
    cost = np.stack([np.random.default_rng(s).integers(0, 4, (Q, G)).astype(np.float32).reshape(-1) for s in range(seeds)])
    matched, status = run_host(host_program, tmp_path, cost, seeds, Q, [G])
    check_every_problem(matched, status, cost, seeds, Q, [G])
    for l in range(seeds):
        m, blk = matched[l, 0], cost[l].reshape(Q, G)
        rows, cols = linear_sum_assignment(blk)
        assert math.fsum(blk[np.nonzero(m >= 0)[0], m[m >= 0]].astype(np.float64)) == math.fsum(blk[rows, cols].astype(np.float64))


def test_lane_width_and_layout_do_not_change_a_byte(host_program, tmp_path):
    """lowest column on equal minima: widths 1, 64, 256 (and 3, no divisor of anything) write identical bytes, with and
    without the transposed copy -- on continuous costs, on ties and on a file with refused problems"""
    files = [(case_cost(250, 1, 2, 900, 10, [150, 37]), 1, 900, [150, 37]),
             (case_cost(1, 3, 2, 30, 10, [7, 12]), 3, 30, [7, 12]),
             (np.random.default_rng(0).integers(0, 4, (2, 40 * 57)).astype(np.float32), 2, 40, [17, 40])]
    bad = np.random.default_rng(1).random((2, 12 * 10)).astype(np.float32)
    bad[0, 7] = np.nan
    bad[1, 12 * 5:] = np.inf
    files.append((bad, 2, 12, [5, 5]))
    for cost, NL, Q, counts in files:
        want = run_host(host_program, tmp_path, cost, NL, Q, counts, lanes=1, transpose=0, raw=True)
        for lanes, transpose in ((1, 1), (3, 1), (64, 0), (64, 1), (256, 0), (256, 1)):
            assert run_host(host_program, tmp_path, cost, NL, Q, counts, lanes=lanes, transpose=transpose, raw=True) == want


def test_invalid_entries_become_status_codes(host_program, tmp_path):
    """SciPy raises 'matrix contains invalid numeric entries' for NaN / -inf and 'cost matrix is infeasible' when +inf
    cannot be avoided; the solver reports 1 resp. 2 for that problem alone and writes -1 in its row"""
    from vidar_amd.plugin.dense_heads import det_ops as D
    rng = np.random.default_rng(7)
    Q, counts = 12, [5, 5, 5, 5, 5, 14]
    total = sum(counts)
    cost = rng.random((2, Q * total)).astype(np.float32) * 10
    start = D.gt_starts(counts)

    def block(l, b):
        return cost[l, Q * start[b]:Q * start[b + 1]].reshape(Q, counts[b])
    block(0, 0)[3, 2] = np.nan
    block(0, 2)[11, 4] = -np.inf
    block(0, 3)[:, 1] = np.inf                      # Q > G: every ground truth must be matched, this one cannot be
    block(0, 4)[:6, 1] = np.inf                     # avoidable: six other queries remain for that ground truth
    block(1, 4)[2, :] = np.inf                      # avoidable: the query stays background
    block(1, 5)[:, 9] = np.inf                      # Q < G: two ground truths stay unmatched, this one among them
    block(1, 1)[0, 0] = np.inf
    matched, status = run_host(host_program, tmp_path, cost, 2, Q, counts)
    want_status = np.zeros((2, 6), np.int32)
    want_status[0, 0] = want_status[0, 2] = 1
    want_status[0, 3] = 2
    assert np.array_equal(status.reshape(2, 6), want_status)
    for l in range(2):
        for b, G in enumerate(counts):
            if want_status[l, b]:
                assert (matched[l, b] == -1).all()
                with pytest.raises(ValueError, match="invalid numeric" if want_status[l, b] == 1 else "infeasible"):
                    linear_sum_assignment(block(l, b))
            else:
                rows, cols = linear_sum_assignment(block(l, b))
                want = np.full(Q, -1, np.int32)
                want[rows] = cols
                assert np.array_equal(matched[l, b], want), (l, b)
    # a square problem whose only finite perfect matching does not exist: one column of +inf
    sq = rng.random((1, 6 * 6)).astype(np.float32)
    sq.reshape(6, 6)[:, 4] = np.inf
    matched, status = run_host(host_program, tmp_path, sq, 1, 6, [6])
    assert status.tolist() == [2] and (matched == -1).all()


@pytest.mark.parametrize("Q,counts", [(1, [1]), (1, [9]), (9, [1]), (1, [0]), (5, [0, 1, 0]), (2, [2, 3])],
                         ids=["1x1", "Q1", "G1", "Q1-G0", "G0-G1-G0", "small"])
def test_smallest_shapes(host_program, tmp_path, Q, counts):
    from vidar_amd.plugin.dense_heads import det_ops as D
    NL = 2
    cost = np.random.default_rng(Q + sum(counts)).random((NL, Q * sum(counts))).astype(np.float32)
    matched, status = run_host(host_program, tmp_path, cost, NL, Q, counts, lanes=64)
    check_every_problem(matched, status, cost, NL, Q, counts)
    assert np.array_equal(matched, D.solve(cost, NL, Q, counts))


def test_entry_points_check_their_arguments_without_a_gpu():
    """the workspace query answers on the host; the launch entry refuses bad calls before any HIP call and returns 0 for
    an empty grid, so all of it comes back on a machine without a GPU"""
    import ctypes
    from vidar_amd._lib import BAD_ARG, lib
    q, f = lib().vidar_det_assign_workspace_bytes, lib().vidar_det_assign_f32
    n = ctypes.c_int64(-5)
    assert q(6, 2, 900, 187, ctypes.addressof(n)) == 0 and n.value >= 0
    assert q(6, 1, 900, 2048, ctypes.addressof(n)) == 0 and n.value >= 0          # the extent the header promises
    assert q(6, 1, 2048, 1024, ctypes.addressof(n)) == 0 and n.value >= 0
    assert q(0, 0, 0, 0, ctypes.addressof(n)) == 0 and n.value == 0
    for NL, B, Q, total in ((6, 1, 900, 2049), (6, 1, 2049, 10), (6, 1, 1025, 1025), (1, 1, 2048, 1025)):
        assert q(NL, B, Q, total, ctypes.addressof(n)) == 0 and n.value == -1, (NL, B, Q, total)     # unsupported
    for NL, B, Q, total in ((-1, 1, 9, 3), (1, -1, 9, 3), (1, 1, -9, 3), (1, 1, 9, -3), (1 << 20, 1 << 20, 9, 3)):
        assert q(NL, B, Q, total, ctypes.addressof(n)) == BAD_ARG
        assert f(None, None, None, None, NL, B, Q, total, None, 0, None) == BAD_ARG
    assert q(1, 1, 9, 3, None) == BAD_ARG
    fake = 4096                                                   # a non-NULL address that is never dereferenced
    assert f(None, None, None, None, 0, 2, 900, 37, None, 0, None) == 0           # no problem: no launch
    assert f(None, None, None, None, 6, 0, 900, 0, None, 0, None) == 0
    assert f(fake, fake, fake, fake, 6, 1, 900, 2049, fake, 1 << 40, None) == BAD_ARG      # unsupported extent
    assert f(None, fake, fake, fake, 6, 1, 900, 37, fake, 1 << 40, None) == BAD_ARG        # cost
    assert f(fake, None, fake, fake, 6, 1, 900, 37, fake, 1 << 40, None) == BAD_ARG        # gt_start
    assert f(fake, fake, None, fake, 6, 1, 900, 37, fake, 1 << 40, None) == BAD_ARG        # matched
    assert f(fake, fake, fake, None, 6, 1, 900, 37, fake, 1 << 40, None) == BAD_ARG        # status
    q(6, 1, 900, 37, ctypes.addressof(n))
    if n.value > 0:
        assert f(fake, fake, fake, fake, 6, 1, 900, 37, None, n.value, None) == BAD_ARG    # workspace missing
        assert f(fake, fake, fake, fake, 6, 1, 900, 37, fake, n.value - 1, None) == BAD_ARG    # too small
        assert f(fake, fake, fake, fake, 6, 1, 900, 37, fake + 2, n.value, None) == BAD_ARG    # misaligned


def test_switch_and_status_check(monkeypatch):
    from vidar_amd.plugin.dense_heads import det_ops as D
    monkeypatch.delenv("VIDAR_DET_ASSIGN", raising=False)
    D.set_assign(None)
    assert D.assign_mode() == "host"                              # off by default
    monkeypatch.setenv("VIDAR_DET_ASSIGN", "device")
    assert D.assign_mode() == "device"
    D.set_assign("host")
    assert D.assign_mode() == "host"                              # the call wins over the environment
    D.set_assign(None)
    monkeypatch.setenv("VIDAR_DET_ASSIGN", "gpu")
    with pytest.raises(ValueError, match="VIDAR_DET_ASSIGN"):
        D.assign_mode()
    with pytest.raises(ValueError):
        D.set_assign("gpu")
    monkeypatch.delenv("VIDAR_DET_ASSIGN")
    D.check_assign_status(torch.zeros(12, dtype=torch.int32))
    D.check_assign_status(None)
    with pytest.raises(ValueError, match="matrix contains invalid numeric entries"):
        D.check_assign_status(torch.tensor([0, 0, 1, 0], dtype=torch.int32))
    with pytest.raises(ValueError, match="cost matrix is infeasible"):
        D.check_assign_status(torch.tensor([0, 2], dtype=torch.int32))
    with pytest.raises(RuntimeError):
        D.assign_device(torch.zeros(1, 6), 1, 1, 3, torch.tensor([0, 2], dtype=torch.int32), 2)     # CPU tensors: no kernel


def test_cpu_tensors_keep_the_host_path_under_the_switch():
    from vidar_amd.plugin.dense_heads import det_ops as D
    cost = torch.from_numpy(case_cost(1, 3, 2, 30, 10, [7, 12]))
    D.set_assign("device")
    try:
        matched, status = D.assign(cost, 3, 2, 30, torch.from_numpy(D.gt_starts([7, 12])), [7, 12])
    finally:
        D.set_assign(None)
    assert status is None and np.array_equal(matched.numpy(), D.solve(cost.numpy(), 3, 30, [7, 12]))
