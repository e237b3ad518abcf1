"""`chamferdist._C` -- same callables as the reference's pybind module
(third_lib/chamfer_dist/chamferdist/chamferdist/ext.cpp:5-11), on gfx950 HIP kernels:
  * K = 1, D = 3 (every call site of ViDAR: chamfer.py:77-93) runs vidar_knn1_d3_{fwd,bwd} (csrc/knn.hip);
  * every other (D, K) with 1 <= D <= 8 and 1 <= K <= 32 -- the range of the reference's templated kernels
    (knn.cu:261-295) -- runs vidar_knn_{fwd,bwd}_f32 (csrc/knn_generic.hip): per-lane sorted top-K lists in registers,
    no distance matrix, a workspace proportional to N * P1 * chunks * K;
  * outside that range (D > 8 or K > 32), or with VIDAR_KNN_GENERIC=torch (an A/B switch for tools/kbench.py), a
    chunked torch program ON THE DEVICE of the inputs (`_generic_*` below), not a host fallback: CPU tensors are
    refused exactly like in the hot case.
All three give the results of knn_cpu.cpp:7-58 / :64-106 -- fp32 distances with separately rounded products,
ascending, ties to the lower index, zero rows past `lengths1`, zero slots past `lengths2` -- indices and distances bit
for bit."""
from __future__ import annotations

import ctypes
import os
import warnings

import torch

from ..._lib import lib, check, ptr, stream_of, TIMER
from ... import deterministic


def knn_check_version(version: int, D: int, K: int) -> bool:
    """KnnCheckVersion (knn.cu:269-280): which of the reference's four kernels accepts (D, K).  Every accepted
    combination computes the same result here (see the module docstring for which kernel runs)."""
    if version == 0:
        return True
    if version == 1:
        return 1 <= D <= 32
    if version == 2:
        return 1 <= D <= 8 and 1 <= K <= 32
    if version == 3:
        return 1 <= D <= 8 and 1 <= K <= 4
    return False


def _prep(p1, p2, lengths1, lengths2):
    if not (p1.is_cuda and p2.is_cuda):
        raise RuntimeError("p1/p2 must be CUDA tensors (vidar_amd has no CPU path)")
    if p1.dtype != torch.float32 or p2.dtype != torch.float32:
        raise RuntimeError("p1/p2 must be float32")
    if p1.dim() != 3 or p2.dim() != 3 or p1.shape[2] != p2.shape[2]:
        raise RuntimeError("p1/p2 must be [N, P, D] with the same D")
    if p1.shape[0] != p2.shape[0]:
        raise RuntimeError("batch sizes differ")
    return (p1.contiguous(), p2.contiguous(), lengths1.to(torch.int64).contiguous(),
            lengths2.to(torch.int64).contiguous())


_GENERIC_CHUNK_ELEMS = 1 << 25          # distance-matrix elements per chunk of p1 rows (128 MiB of fp32 + the sort's indices)


def _generic_knn_idx(p1, p2, l1, l2, K):
    """knn_cpu.cpp:7-58 as a tensor program on p1's device: for every valid row of p1 the K nearest valid points of p2,
    squared L2 accumulated over d = 0..D-1 in fp32 with separately rounded products (the CPU build's arithmetic),
    ascending, ties to the lower index (a STABLE sort: the priority queue keeps the first-seen of equal distances and
    pops them in (distance, index) order); rows >= lengths1 and slots >= lengths2 stay zero like `torch::full(.., 0)`."""
    N, P1, D = p1.shape
    P2 = p2.shape[1]
    idx = torch.zeros((N, P1, K), dtype=torch.int64, device=p1.device)
    dist = torch.zeros((N, P1, K), dtype=torch.float32, device=p1.device)
    if N == 0 or P1 == 0 or P2 == 0 or K == 0:
        return idx, dist
    kk = min(K, P2)
    rows = max(1, _GENERIC_CHUNK_ELEMS // P2)
    col = torch.arange(P2, device=p1.device)
    slot = torch.arange(kk, device=p1.device)
    row = torch.arange(P1, device=p1.device)
    for n in range(N):
        col_ok = col < l2[n]                                             # [P2]
        slot_ok = slot < l2[n]                                           # [kk]
        for r0 in range(0, P1, rows):
            a = p1[n, r0:r0 + rows]                                      # [R, D]
            d = None
            for k in range(D):
                diff = a[:, k, None] - p2[n, None, :, k]
                sq = diff * diff
                d = sq if d is None else d + sq
            d = torch.where(col_ok[None], d, torch.full_like(d, float("inf")))
            dv, di = torch.sort(d, dim=1, stable=True)
            keep = slot_ok[None] & (row[r0:r0 + rows, None] < l1[n])     # [R, kk]
            dist[n, r0:r0 + rows, :kk] = torch.where(keep, dv[:, :kk], torch.zeros_like(dv[:, :kk]))
            idx[n, r0:r0 + rows, :kk] = torch.where(keep, di[:, :kk], torch.zeros_like(di[:, :kk]))
    return idx, dist


def _generic_knn_backward(p1, p2, l1, l2, idxs, grad_dists):
    """knn_cpu.cpp:64-106 (== knn.cu:443-544): d dist / d p1 = 2 g (p1 - p2[idx]), scattered with the opposite sign to
    p2[idx]; only rows < lengths1 and slots < min(lengths2, K) contribute."""
    N, P1, D = p1.shape
    K = idxs.shape[2]
    g1 = torch.zeros_like(p1)
    g2 = torch.zeros_like(p2)
    if N == 0 or P1 == 0 or K == 0 or p2.shape[1] == 0:
        return g1, g2
    row_ok = torch.arange(P1, device=p1.device)[None, :, None] < l1[:, None, None]
    slot_ok = torch.arange(K, device=p1.device)[None, None, :] < l2[:, None, None]
    w = torch.where(row_ok & slot_ok, grad_dists, torch.zeros_like(grad_dists))          # [N, P1, K]
    ii = torch.where(row_ok & slot_ok, idxs, torch.zeros_like(idxs))
    nb = p2.gather(1, ii.reshape(N, P1 * K, 1).expand(-1, -1, D)).view(N, P1, K, D)
    diff = 2.0 * w[..., None] * (p1[:, :, None, :] - nb)                                  # [N, P1, K, D]
    g1 = diff.sum(2)
    g2.scatter_add_(1, ii.reshape(N, P1 * K, 1).expand(-1, -1, D), -diff.reshape(N, P1 * K, D))
    return g1, g2


def _kernel_workspace(N, P1, P2, D, K, chunks=0):
    """(bytes, chunks_used) of vidar_knn_fwd_f32, or None where (D, K) or the extents are outside the kernels' range"""
    nbytes, used = ctypes.c_int64(0), ctypes.c_int64(0)
    rc = lib().vidar_knn_workspace_bytes(N, P1, P2, D, K, chunks, ctypes.addressof(nbytes), ctypes.addressof(used))
    return None if rc != 0 or nbytes.value < 0 else (nbytes.value, used.value)


def _use_torch_program():
    return os.environ.get("VIDAR_KNN_GENERIC", "") == "torch"


def knn_points_idx(p1, p2, lengths1, lengths2, K: int = 1, version: int = -1, chunks: int = 0):
    """-> (idx int64 [N,P1,K], dists f32 [N,P1,K]) ; squared L2, ties -> lowest index.  `chunks` (not in the reference's
    signature): the split of p2 the generic kernel takes, 0 = its own choice; the result does not depend on it."""
    K = int(K)
    if version >= 0 and not knn_check_version(version, p1.shape[-1], K):
        # the reference prints a warning and goes on with ChooseVersion(D, K) (knn.cu:331-339); every version computes
        # the same result here
        warnings.warn(f"Requested KNN version {version} is not compatible with D = {p1.shape[-1]}; K = {K}. "
                      f"Falling back to the default version", UserWarning, stacklevel=2)
    p1, p2, l1, l2 = _prep(p1, p2, lengths1, lengths2)
    N, P1, D = p1.shape
    P2 = p2.shape[1]
    if K == 1 and D == 3:
        idx = torch.empty((N, P1, 1), dtype=torch.int64, device=p1.device)
        dist = torch.empty((N, P1, 1), dtype=torch.float32, device=p1.device)
        ws = torch.empty((max(N * P1, 1),), dtype=torch.int64, device=p1.device)
        with TIMER.span("knn1_d3_fwd", 12 * (N * P1 + N * P2) + 12 * N * P1):
          check(lib().vidar_knn1_d3_fwd(ptr(p1), ptr(p2), ptr(l1), ptr(l2), ptr(idx), ptr(dist), ptr(ws),
                                      N, P1, P2, stream_of(p1)), "knn_points_idx")
        return idx, dist
    need = None if _use_torch_program() else _kernel_workspace(N, P1, P2, D, K, chunks)
    if need is None:
        return _generic_knn_idx(p1, p2, l1.to(p1.device), l2.to(p1.device), K)
    if N == 0 or P1 == 0 or P2 == 0:              # nothing to search: the zero fill is the whole result
        return (torch.zeros((N, P1, K), dtype=torch.int64, device=p1.device),
                torch.zeros((N, P1, K), dtype=torch.float32, device=p1.device))
    l1, l2 = l1.to(p1.device), l2.to(p1.device)
    idx = torch.empty((N, P1, K), dtype=torch.int64, device=p1.device)
    dist = torch.empty((N, P1, K), dtype=torch.float32, device=p1.device)
    ws = torch.empty(need[0], dtype=torch.uint8, device=p1.device)
    with TIMER.span("knn_fwd", 4 * D * (N * P1 + N * P2) + 12 * N * P1 * K):
        check(lib().vidar_knn_fwd_f32(ptr(p1), ptr(p2), ptr(l1), ptr(l2), ptr(idx), ptr(dist), ptr(ws), need[0],
                                      N, P1, P2, D, K, chunks, stream_of(p1)), "knn_points_idx")
    return idx, dist


def knn_points_backward(p1, p2, lengths1, lengths2, idxs, grad_dists):
    """-> (grad_p1 [N,P1,D], grad_p2 [N,P2,D])   (knn_cpu.cpp:64-106)"""
    if idxs.shape[-1] != 1 or p1.shape[-1] != 3:
        deterministic.require("knn generic backward")             # before anything touches the GPU
    p1, p2, l1, l2 = _prep(p1, p2, lengths1, lengths2)
    N, P1, D = p1.shape
    P2 = p2.shape[1]
    K = idxs.shape[-1]
    if K != 1 or D != 3:
        idxs, grad_dists = idxs.contiguous(), grad_dists.contiguous().float()
        l1, l2 = l1.to(p1.device), l2.to(p1.device)
        if _use_torch_program() or _kernel_workspace(N, P1, P2, D, K) is None:
            return _generic_knn_backward(p1, p2, l1, l2, idxs, grad_dists)
        if N == 0 or P1 == 0 or P2 == 0:
            return torch.zeros_like(p1), torch.zeros_like(p2)
        g1 = torch.empty_like(p1)
        g2 = torch.empty_like(p2)
        check(lib().vidar_knn_bwd_f32(ptr(p1), ptr(p2), ptr(l1), ptr(l2), ptr(idxs), ptr(grad_dists), ptr(g1), ptr(g2),
                                      N, P1, P2, D, K, stream_of(p1)), "knn_points_backward")
        return g1, g2
    g1 = torch.empty_like(p1)
    g2 = torch.empty_like(p2)
    ws, wsn = None, 0
    if deterministic.sync():                # the fixed-point accumulators of grad_p2
        nbytes = ctypes.c_int64(0)
        check(lib().vidar_knn1_d3_bwd_workspace_bytes(N, P2, ctypes.addressof(nbytes)), "knn_points_backward")
        wsn = nbytes.value
        ws = torch.empty(wsn, dtype=torch.uint8, device=p1.device)
    check(lib().vidar_knn1_d3_bwd_ws(ptr(p1), ptr(p2), ptr(l1), ptr(l2), ptr(idxs.contiguous()),
                                     ptr(grad_dists.contiguous().float()), ptr(g1), ptr(g2), N, P1, P2,
                                     ptr(ws), wsn, stream_of(p1)), "knn_points_backward")
    return g1, g2
