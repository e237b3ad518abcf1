// K nearest neighbours for 1 <= D <= 8, 1 <= K <= 32 (the reference's V2 range, knn.cu:261-264), gfx950.
//
// Replaces (behaviour) third_lib/chamfer_dist/chamferdist/chamferdist/knn.cu:37-255 (the four templated kernels),
// host :297-435, backward :443-544, with the results of the CPU path knn_cpu.cpp:7-58, :64-106 bit for bit: squared L2
// in fp32, every product and sum rounded on its own (-ffp-contract=off), the K smallest by (distance, index) ascending.
// K = 1, D = 3 stays with knn.hip.
//
// Forward, two launches, no distance matrix:
//  * scan: a lane owns one query point and its KB best keys (csrc/knn_topk.h), sorted, in registers; KB is the bucket
//    of K and D a template argument, so every list and coordinate index is a constant.  The p2 point of an iteration is
//    wave-uniform and comes in through the scalar unit, as in knn1_d3_scan_kernel (VIDAR_KNN_P2_LDS=1 stages tiles of
//    p2 in LDS instead: the A/B of profiles/kbench_knn_generic.md).  A candidate costs the D-term distance and one
//    compare with the lane's worst key; the insertion runs only in the lanes that need it.
//    P2 is cut into `chunks` ranges across blockIdx.y so that a small P1 still fills the chip; every (row, chunk) stores
//    its first K keys to the workspace [N, P1, chunks, K].
//  * merge: a lane per row folds the lists of the chunks that hold points of the row's cloud, unpacks the keys and
//    writes all K slots of idx / dist2 (zeros past lengths1 / lengths2).
// The key order is total, so neither `chunks` nor the launch geometry shows in the result.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vidar_hip.h"
#include "vidar_common.h"
#include "det_acc.h"
#include "knn_topk.h"

#ifndef VIDAR_KNN_P2_LDS
#define VIDAR_KNN_P2_LDS 0
#endif

namespace {

using namespace vidar_knn;

constexpr int kThreads = 256;

template <int D, int KB>
__global__ __launch_bounds__(kThreads) void knn_scan_kernel(
    const float* __restrict__ p1, const float* __restrict__ p2, const int64_t* __restrict__ len1,
    const int64_t* __restrict__ len2, uint64_t* __restrict__ lists, int P1, int P2, int K, int chunks) {
  const int n = blockIdx.z, c = blockIdx.y;
  const int l1 = (int)min((int64_t)P1, len1[n]);
  const int l2 = (int)min((int64_t)P2, len2[n]);
  const int j0 = chunk_begin(c, P2, chunks);
  const int j1 = min(chunk_begin(c + 1, P2, chunks), l2);
  // the merge reads neither rows past lengths1 nor chunks that begin past lengths2
  if (j0 >= j1 || (int)blockIdx.x * kThreads >= l1) return;
  const int row = blockIdx.x * kThreads + threadIdx.x;

  float a[D];
  const float* p = p1 + ((size_t)n * P1 + min(row, P1 - 1)) * D;
#pragma unroll
  for (int d = 0; d < D; ++d) a[d] = p[d];
  uint64_t keys[KB];
  list_clear<KB>(keys);
  const float* q = p2 + (size_t)n * P2 * D;
#if VIDAR_KNN_P2_LDS
  constexpr int kTile = 256;                       // p2 points per LDS tile
  __shared__ float tile[kTile * D];
  for (int t0 = j0; t0 < j1; t0 += kTile) {
    const int cnt = min(kTile, j1 - t0);
    __syncthreads();
    for (int e = threadIdx.x; e < cnt * D; e += kThreads) tile[e] = q[(size_t)t0 * D + e];
    __syncthreads();
    list_scan<D, KB>(a, tile, cnt, t0, keys);
  }
#else
  list_scan<D, KB>(a, q + (size_t)j0 * D, j1 - j0, j0, keys);      // q, j0, j1 are wave-uniform: the loads are scalar loads
#endif
  if (row < P1) list_store<KB>(keys, K, lists + (((size_t)n * P1 + row) * chunks + c) * K);
}

template <int KB>
__global__ __launch_bounds__(kThreads) void knn_merge_kernel(
    const uint64_t* __restrict__ lists, const int64_t* __restrict__ len1, const int64_t* __restrict__ len2,
    int64_t* __restrict__ idx, float* __restrict__ dist, int P1, int P2, int K, int chunks) {
  const int n = blockIdx.y;
  const int row = blockIdx.x * kThreads + threadIdx.x;
  if (row >= P1) return;
  const int l2 = (int)min((int64_t)P2, max((int64_t)0, len2[n]));
  const size_t at = (size_t)n * P1 + row;
  row_finish<KB>(lists + at * chunks * K, chunks, K, P2, l2, row < len1[n], idx + at * K, dist + at * K);
}

// grad_p1[n,i,d] = sum_k c, c = (2 g[n,i,k]) (p1[n,i,d] - p2[n,idx[n,i,k],d]) in the order k = 0, 1, .. (a plain store);
// grad_p2[n,idx,d] -= c through the accumulate policy of det_acc.h (knn_cpu.cpp:88-103); the shape of knn1_d3_bwd_body
template <int D, class Acc>
__device__ __forceinline__ void knn_bwd_body(
    const float* __restrict__ p1, const float* __restrict__ p2, const int64_t* __restrict__ len1,
    const int64_t* __restrict__ len2, const int64_t* __restrict__ idx, const float* __restrict__ grad_dist,
    float* __restrict__ grad_p1, float* __restrict__ grad_p2, int P1, int P2, int K, Acc& acc) {
  const int n = blockIdx.y;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= P1) return;
  float a[D], g1[D];
  const float* pa = p1 + ((size_t)n * P1 + i) * D;
#pragma unroll
  for (int d = 0; d < D; ++d) { a[d] = pa[d]; g1[d] = 0.f; }
  if (i < len1[n]) {
    const int kk = (int)min((int64_t)K, max((int64_t)0, len2[n]));
    for (int k = 0; k < kk; ++k) {
      const int64_t j = idx[((size_t)n * P1 + i) * K + k];
      if (j < 0 || j >= P2) continue;              // an index the forward cannot produce: never an address
      const float g2 = 2.0f * grad_dist[((size_t)n * P1 + i) * K + k];
      const float* b = p2 + ((size_t)n * P2 + j) * D;
      float* o = grad_p2 + ((size_t)n * P2 + j) * D;
#pragma unroll
      for (int d = 0; d < D; ++d) {
        const float c = g2 * (a[d] - b[d]);
        g1[d] += c;
        if (g2 != 0.f) acc.add(o + d, -c);         // adding +-0 is the identity; skipping it avoids same-address atomic storms
      }
    }
  }
  if (Acc::kMeasureOnly) return;
  float* o1 = grad_p1 + ((size_t)n * P1 + i) * D;
#pragma unroll
  for (int d = 0; d < D; ++d) o1[d] = g1[d];
}

template <int D>
__global__ __launch_bounds__(kThreads) void knn_bwd_kernel(
    const float* __restrict__ p1, const float* __restrict__ p2, const int64_t* __restrict__ len1,
    const int64_t* __restrict__ len2, const int64_t* __restrict__ idx, const float* __restrict__ grad_dist,
    float* __restrict__ grad_p1, float* __restrict__ grad_p2, int P1, int P2, int K) {
  det::AccAtomic acc;
  knn_bwd_body<D>(p1, p2, len1, len2, idx, grad_dist, grad_p1, grad_p2, P1, P2, K, acc);
}

// the CU count for the automatic split; 256 (an MI355X) where no device answers, so that the query works without one
int cu_count() {
  static const int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) {
      (void)hipGetLastError();
      return 256;
    }
    return n;
  }();
  return cus;
}

// the split of a call, or 0 for arguments outside the kernel range
int chunks_of(int N, int P1, int P2, int D, int K, int chunks) {
  if (!in_range(D, K) || N < 0 || P1 < 0 || P2 < 0 || chunks < 0) return 0;
  if (chunks == 0) chunks = auto_chunks(N, P1, P2, K, cu_count());
  const int most = P2 > 0 ? P2 : 1;                // no range without a point
  chunks = chunks > most ? most : chunks;
  // grid.y / grid.z limits, the element counts of p1 / p2 as int (an index is the low key half), the workspace as int64
  if (chunks > 65535 || N > 65535 || (int64_t)P1 * D > INT32_MAX || (int64_t)P2 * D > INT32_MAX ||
      (int64_t)N * P1 > INT64_MAX / 8 / ((int64_t)chunks * K))
    return 0;
  return chunks;
}

}  // namespace

extern "C" {

int vidar_knn_workspace_bytes(int N, int P1, int P2, int D, int K, int chunks, int64_t* bytes, int64_t* chunks_used) {
  if (bytes) *bytes = -1;
  if (chunks_used) *chunks_used = 0;
  const int c = chunks_of(N, P1, P2, D, K, chunks);
  if (c == 0 || !bytes) return VIDAR_ERR_BAD_ARG;
  *bytes = (int64_t)sizeof(uint64_t) * N * P1 * c * K;
  if (chunks_used) *chunks_used = c;
  return 0;
}

int vidar_knn_fwd_f32(const float* p1, const float* p2, const int64_t* lengths1, const int64_t* lengths2,
                      int64_t* idx, float* dist2, void* workspace, size_t workspace_bytes,
                      int N, int P1, int P2, int D, int K, int chunks, void* stream) {
  if (N < 0 || P1 < 0 || P2 < 0 || K < 0) return VIDAR_ERR_BAD_ARG;
  if (N == 0 || P1 == 0 || P2 == 0 || K == 0) return 0;
  const int c = chunks_of(N, P1, P2, D, K, chunks);
  if (c == 0) return VIDAR_ERR_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (!workspace || workspace_bytes < sizeof(uint64_t) * (size_t)N * P1 * c * K) return VIDAR_ERR_BAD_ARG;
  VIDAR_ENTER();
  uint64_t* lists = (uint64_t*)workspace;
  const int bx = (P1 + kThreads - 1) / kThreads;
  dispatch(D, bucket(K), [&](auto d, auto kb) {
    hipLaunchKernelGGL((knn_scan_kernel<decltype(d)::value, decltype(kb)::value>), dim3(bx, c, N), dim3(kThreads), 0, s,
                       p1, p2, lengths1, lengths2, lists, P1, P2, K, c);
  });
  dispatch(1, bucket(K), [&](auto, auto kb) {          // the merge does not depend on D
    hipLaunchKernelGGL((knn_merge_kernel<decltype(kb)::value>), dim3(bx, N), dim3(kThreads), 0, s, lists, lengths1,
                       lengths2, idx, dist2, P1, P2, K, c);
  });
  return vidar_last_error();
}

int vidar_knn_bwd_f32(const float* p1, const float* p2, const int64_t* lengths1, const int64_t* lengths2,
                      const int64_t* idx, const float* grad_dist2, float* grad_p1, float* grad_p2,
                      int N, int P1, int P2, int D, int K, void* stream) {
  if (N < 0 || P1 < 0 || P2 < 0 || K < 0) return VIDAR_ERR_BAD_ARG;
  if (N == 0 || P1 == 0 || P2 == 0 || K == 0) return 0;
  if (!in_range(D, K) || N > 65535 || (int64_t)P1 * D > INT32_MAX || (int64_t)P2 * D > INT32_MAX) return VIDAR_ERR_BAD_ARG;
  VIDAR_ENTER();
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(grad_p2, 0, sizeof(float) * (size_t)N * P2 * D, s);
  if (e != hipSuccess) return (int)e;
  dispatch(D, 1, [&](auto d, auto) {
    hipLaunchKernelGGL(knn_bwd_kernel<decltype(d)::value>, dim3((P1 + kThreads - 1) / kThreads, N), dim3(kThreads), 0, s,
                       p1, p2, lengths1, lengths2, idx, grad_dist2, grad_p1, grad_p2, P1, P2, K);
  });
  return vidar_last_error();
}

}  // extern "C"
