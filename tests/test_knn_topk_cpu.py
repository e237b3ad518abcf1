"""CPU: the top-K list, the scan and the chunk merge of csrc/knn_topk.h (the bodies of the kernels of
csrc/knn_generic.hip) through the stand-alone host program tests/knn_topk_host.cpp, against the reference's OWN
knn_cpu.cpp build (oracle/_ref): indices and distances bit for bit for every D, K bucket edge and chunk count, with ties,
ragged lengths and K above the cloud size; the workspace query of the built library and the version fall-back of the
wrapper, none of which needs a GPU."""
import ctypes
import os
import struct
import subprocess
import warnings
from pathlib import Path

import numpy as np
import pytest
import torch

from test_knn_generic_cpu import _clouds

ROOT = Path(__file__).resolve().parents[1]
DS = [1, 2, 3, 5, 8]
KS = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32]
CHUNKS = [1, 2, 5, 33]
N, P1, P2 = 2, 57, 33


def build_host_program(directory):
    exe = Path(directory) / "knn_topk_host"
    base = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", f"-I{ROOT / 'vidar_amd' / 'csrc'}",
            str(ROOT / "tests" / "knn_topk_host.cpp"), "-o", str(exe)]
    # a stand-alone program with its own main: the host sanitizers apply when the toolchain ships their runtimes
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.run(base, check=True)
    return exe


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    return build_host_program(tmp_path_factory.mktemp("knn_topk_host"))


def run_host(exe, tmp, a, b, l1, l2, K, chunks):
    """the host program on torch CPU tensors -> (idx int64 [N, P1, K], dist f32 [N, P1, K])"""
    n, p1, d = a.shape
    p2 = b.shape[1]
    blob = (struct.pack("<6i", n, p1, p2, d, K, chunks) + l1.numpy().astype("<i8").tobytes() + l2.numpy().astype("<i8").tobytes()
            + np.ascontiguousarray(a.numpy(), "<f4").tobytes() + np.ascontiguousarray(b.numpy(), "<f4").tobytes())
    src, dst = Path(tmp) / "knn_in.bin", Path(tmp) / "knn_out.bin"
    src.write_bytes(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stderr[-2000:]
    data = dst.read_bytes()
    cnt = n * p1 * K
    assert len(data) == 12 * cnt
    idx = torch.from_numpy(np.frombuffer(data, "<i8", cnt).reshape(n, p1, K).copy())
    dist = torch.from_numpy(np.frombuffer(data, "<f4", cnt, 8 * cnt).reshape(n, p1, K).copy())
    return idx, dist


def ragged(l1, l2, case):
    """one full cloud and one shorter than most K; `empty`: no valid point in cloud 1, no valid row in batch 0"""
    l1, l2 = l1.clone(), l2.clone()
    l2[0] = P2
    l2[1] = 3
    if case == "empty":
        l2[1] = 0
        l1[0] = 0
    return l1, l2


@pytest.mark.parametrize("ties", [False, True], ids=["gaussian", "lattice"])
@pytest.mark.parametrize("D", DS)
def test_lists_and_merge_match_the_reference_build(host_program, tmp_path, ref_modules, D, ties):
    """every K, both ragged cases and every chunk count of one (D, cloud kind): 80 runs of the host program on
    2 x 57 x 33 points"""
    ref = ref_modules("ref_chamferdist_C")
    a, b, l1, l2 = _clouds(D * 100 + int(ties), N, P1, P2, D, ties)
    for K in KS:
        for case in ("short", "empty"):
            m1, m2 = ragged(l1, l2, case)
            ri, rd = ref.knn_points_idx(a, b, m1, m2, K, -1)
            for chunks in CHUNKS:
                oi, od = run_host(host_program, tmp_path, a, b, m1, m2, K, chunks)
                assert torch.equal(oi, ri), (D, K, chunks, case)
                assert torch.equal(od, rd), (D, K, chunks, case)


@pytest.mark.parametrize("K", [1, 5, 32])
def test_identical_points_come_out_in_index_order(host_program, tmp_path, ref_modules, K):
    ref = ref_modules("ref_chamferdist_C")
    a, b, l1, l2 = _clouds(3, N, P1, P2, 3, False)
    b[:] = b[0, 0]                                                # every distance of a row is equal: only the index orders
    l2[0] = P2; l2[1] = 3
    ri, rd = ref.knn_points_idx(a, b, l1, l2, K, -1)
    for chunks in CHUNKS:
        oi, od = run_host(host_program, tmp_path, a, b, l1, l2, K, chunks)
        assert torch.equal(oi, ri) and torch.equal(od, rd)
        for n in range(N):
            kk = min(K, int(l2[n]))
            want = torch.cat([torch.arange(kk), torch.zeros(K - kk, dtype=torch.int64)])
            assert torch.equal(oi[n, :int(l1[n])], want.expand(int(l1[n]), K))


def query(n, p1, p2, d, k, chunks):
    from vidar_amd._lib import lib
    nbytes, used = ctypes.c_int64(123), ctypes.c_int64(123)
    rc = lib().vidar_knn_workspace_bytes(n, p1, p2, d, k, chunks, ctypes.addressof(nbytes), ctypes.addressof(used))
    return rc, nbytes.value, used.value


def test_workspace_query():
    from vidar_amd._lib import BAD_ARG
    # 8 bytes per key, [N, P1, chunks, K] keys
    assert query(2, 57, 33, 3, 5, 4) == (0, 8 * 2 * 57 * 4 * 5, 4)
    assert query(1, 30000, 30000, 8, 32, 7) == (0, 8 * 30000 * 7 * 32, 7)
    one = query(3, 100, 1000, 2, 9, 1)[1]
    for chunks in (2, 5, 33, 1000):                               # linear in chunks
        assert query(3, 100, 1000, 2, 9, chunks) == (0, chunks * one, chunks)
    for p2 in (33, 1000, 30000, 1 << 24):                         # never a function of P1 * P2
        assert query(3, 100, p2, 2, 9, 33) == (0, 33 * one, 33)
    rc, nbytes, used = query(1, 5, 5000, 3, 4, 0)                 # the library's own split: a small P1 against a large P2
    assert rc == 0 and used > 1 and nbytes == 8 * 5 * used * 4
    for d, k in ((9, 1), (1, 33), (0, 1), (1, 0)):
        assert query(2, 57, 33, d, k, 1) == (BAD_ARG, -1, 0)
    assert query(1, 1 << 30, 33, 3, 2, 1) == (BAD_ARG, -1, 0)     # P1 * D beyond a 32-bit element index


def test_zero_extents_return_before_any_gpu_call():
    """no GPU on this machine: a call that reached HIP would not return 0"""
    from vidar_amd._lib import lib
    L = lib()
    for n, p1, p2, k in ((0, 5, 5, 2), (1, 0, 5, 2), (1, 5, 0, 2), (1, 5, 5, 0)):
        assert L.vidar_knn_fwd_f32(None, None, None, None, None, None, None, 0, n, p1, p2, 3, k, 0, None) == 0
        assert L.vidar_knn_bwd_f32(None, None, None, None, None, None, None, None, n, p1, p2, 3, k, None) == 0


def test_an_unfit_version_warns_and_goes_on():
    """version = 3 does not take K = 8 (knn.cu:331-339: a warning, then ChooseVersion): the call goes on to the
    argument check that refuses host tensors"""
    from vidar_amd.third_lib.chamferdist import _C
    a, b, l1, l2 = _clouds(0, 1, 8, 8, 3, False)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with pytest.raises(RuntimeError) as e:
            _C.knn_points_idx(a, b, l1, l2, 8, 3)
    assert "Invalid version" not in str(e.value) and "CUDA tensors" in str(e.value)
    assert any("version 3" in str(x.message) for x in w)
    with warnings.catch_warnings(record=True) as w:               # a version that fits does not warn
        warnings.simplefilter("always")
        with pytest.raises(RuntimeError):
            _C.knn_points_idx(a, b, l1, l2, 4, 3)
    assert not w
