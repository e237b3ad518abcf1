// Hungarian assignment of the detection loss tail on the device: ALL (layer, sample) problems of a fine-tune step in one
// launch, so that the step's last host read (the cost copy that scipy.optimize.linear_sum_assignment waits for) goes.
// The per-problem body is csrc/det_assign_math.h (algorithm, tie rule, status codes, loop bounds); this file is its
// device Team, the kernel shell and the C entry points.
//
// Kernel notes (gfx950, wave64):
//   * one workgroup per problem (l, b); G_b comes from the device gt_start.  The work is SERIAL in the search step and
//     parallel only in the scan of the long side, a few columns per lane: latency-bound like the rest of this tail
//     (81-89 search steps at G 37, 878 at G 150, 11 625 at G 512 for Q 900), and the NL * B problems are independent.
//   * all solver state stays in LDS (62 KiB of the CU's 160; det_assign_math.h states the extent derived from it).  A
//     column's entries are touched by its own lane only (j % lanes), in 8-byte and 4-byte accesses at consecutive
//     addresses: conflict-free.
//   * the step's minimum: fixed xor-butterfly over the wave on (value, column), lowest column on equal values; one
//     (value, column) per wave to LDS, a barrier, and every thread folds the few wave results in wave order.  The order
//     on (value, column) is total, so any tree gives the same answer.  That barrier is the only one of a search step:
//     the wave results go to two alternating sets of slots, and the closed flag is written by the column's own lane.
//   * with Q > G a row is one ground-truth box over all queries, stride G in the cost block: the pre-pass (which reads the
//     whole block once anyway, for NaN / -inf) writes a transposed copy into the caller's workspace and the scans read
//     consecutive addresses.  -DVIDAR_DET_ASSIGN_STRIDED leaves the block as it is (the A/B of profiles/kbench_det.md).
//   * no atomics, no cross-workgroup traffic: same inputs, same bytes, wherever a problem sits in the grid.
//   * compiled with -ffp-contract=off (build.py pins it): the host program of the tests rounds identically.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "det_assign_math.h"
#include "vidar_common.h"
#include "vidar_hip.h"

#ifndef VIDAR_DET_ASSIGN_THREADS
#define VIDAR_DET_ASSIGN_THREADS 512
#endif

namespace {

using namespace vidar_det_assign;

constexpr int kThreads = VIDAR_DET_ASSIGN_THREADS;
static_assert(kThreads % 64 == 0 && kThreads >= 64 && kThreads <= 1024, "whole waves");
#ifdef VIDAR_DET_ASSIGN_STRIDED
constexpr bool kTranspose = false;
#else
constexpr bool kTranspose = true;
#endif

struct DeviceTeam {
  double* w_val;      // LDS, two sets of one per wave: consecutive argmin() calls alternate, so a wave that is already
  int* w_idx;         // writing the next step's minimum cannot overwrite what a slower wave still reads
  int set;
  double val;
  int idx;
  bool flag;
  __device__ __forceinline__ int lanes() const { return kThreads; }
  template <class F> __device__ __forceinline__ void each(F f) { f((int)threadIdx.x); }
  template <class F> __device__ __forceinline__ void one(F f) { if (threadIdx.x == 0) f(); }
  __device__ __forceinline__ void sync() { __syncthreads(); }
  __device__ __forceinline__ void vote(int, bool b) { flag = b; }
  __device__ __forceinline__ bool any() { return __syncthreads_or(flag ? 1 : 0) != 0; }
  __device__ __forceinline__ void offer(int, double v, int j) { val = v; idx = j; }
  __device__ __forceinline__ void argmin(double* v, int* j) {
    double bv = val;
    int bj = idx;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double ov = __shfl_xor(bv, off, 64);
      const int oj = __shfl_xor(bj, off, 64);
      if (ov < bv || (ov == bv && oj < bj)) {
        bv = ov;
        bj = oj;
      }
    }
    double* wv = w_val + set * (kThreads / 64);
    int* wj = w_idx + set * (kThreads / 64);
    set ^= 1;
    if ((threadIdx.x & 63) == 0) {
      wv[threadIdx.x >> 6] = bv;
      wj[threadIdx.x >> 6] = bj;
    }
    __syncthreads();
    bv = wv[0];
    bj = wj[0];
#pragma unroll
    for (int w = 1; w < kThreads / 64; ++w) {
      const double ov = wv[w];
      const int oj = wj[w];
      if (ov < bv || (ov == bv && oj < bj)) {
        bv = ov;
        bj = oj;
      }
    }
    *v = bv;
    *j = bj;
  }
};

__global__ __launch_bounds__(kThreads) void det_assign_kernel(const float* __restrict__ cost,
                                                              const int32_t* __restrict__ gt_start,
                                                              int32_t* __restrict__ matched,
                                                              int32_t* __restrict__ status, float* tcost, int B, int Q,
                                                              int total_g) {
  __shared__ double s_u[kMaxShort];
  __shared__ double s_v[kMaxLong];
  __shared__ double s_shortest[kMaxLong];
  __shared__ int32_t s_path[kMaxLong];
  __shared__ int32_t s_col4row[kMaxShort];
  __shared__ int32_t s_row4col[kMaxLong];
  __shared__ uint8_t s_closed[kMaxLong];
  __shared__ double s_wval[2 * (kThreads / 64)];
  __shared__ int s_widx[2 * (kThreads / 64)];
  const int p = blockIdx.x, l = p / B, b = p - l * B;
  const int g0 = gt_start[b], G = gt_start[b + 1] - g0;
  int32_t* m = matched + (int64_t)p * Q;
  if (G < 0 || g0 < 0 || g0 + G > total_g) {            // uniform per workgroup: a gt_start that is not one
    for (int q = threadIdx.x; q < Q; q += kThreads) m[q] = -1;
    if (threadIdx.x == 0) status[p] = kExtent;
    return;
  }
  const int64_t off = (int64_t)l * Q * total_g + (int64_t)Q * g0;
  DeviceTeam team{s_wval, s_widx, 0, 0.0, 0, false};
  const State s{s_u, s_v, s_shortest, s_path, s_col4row, s_row4col, s_closed};
  const int32_t st = solve_problem(team, cost + off, tcost ? tcost + off : nullptr, Q, G, s, m);
  if (threadIdx.x == 0) status[p] = st;
}

// 0 fine, 1 unsupported extent, -1 bad argument
int assign_dims(int NL, int B, int Q, int total_g) {
  if (NL < 0 || B < 0 || Q < 0 || total_g < 0 || (int64_t)NL * B > INT32_MAX) return -1;
  const int lng = Q > total_g ? Q : total_g, sht = Q > total_g ? total_g : Q;
  return (lng > kMaxLong || sht > kMaxShort) ? 1 : 0;
}

int64_t assign_workspace(int NL, int B, int Q, int total_g) {
  if (!kTranspose || NL == 0 || B == 0) return 0;
  return (int64_t)NL * Q * total_g * (int64_t)sizeof(float);
}

}  // namespace

extern "C" {

int vidar_det_assign_workspace_bytes(int NL, int B, int Q, int total_g, int64_t* bytes) {
  const int d = assign_dims(NL, B, Q, total_g);
  if (d < 0 || !bytes) return VIDAR_ERR_BAD_ARG;
  *bytes = d == 1 ? -1 : assign_workspace(NL, B, Q, total_g);
  return 0;
}

int vidar_det_assign_f32(const float* cost, const int32_t* gt_start, int32_t* matched, int32_t* status, int NL, int B,
                         int Q, int total_g, void* workspace, size_t workspace_bytes, void* stream) {
  if (assign_dims(NL, B, Q, total_g) != 0) return VIDAR_ERR_BAD_ARG;
  if (NL == 0 || B == 0) return 0;                                  // no problem: no launch
  const int64_t need = assign_workspace(NL, B, Q, total_g);
  if (!gt_start || !status || (Q > 0 && !matched) || ((int64_t)Q * total_g > 0 && !cost) ||
      (need > 0 && (!workspace || ((uintptr_t)workspace & 3) || workspace_bytes < (size_t)need)))
    return VIDAR_ERR_BAD_ARG;
  VIDAR_ENTER();
  hipLaunchKernelGGL(det_assign_kernel, dim3((unsigned)(NL * B)), dim3(kThreads), 0, (hipStream_t)stream, cost, gt_start,
                     matched, status, need > 0 ? (float*)workspace : nullptr, B, Q, total_g);
  return vidar_last_error();
}

}  // extern "C"
