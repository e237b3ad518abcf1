// The 4d-occ ray errors (L1 / AbsRel along the ground-truth rays) of the forecasting metric, for many (sample, frame)
// segments in one call, fp64: the reference's bevformer/utils/eval_utils.py:185-225 with the nearest neighbour it hands
// to chamferdist (knn.cu:21-57, templated on the scalar type, fp64 there).  The per-ray arithmetic is csrc/ray_eval_math.h.
//
// Two launches:
//   * projection: one lane per prediction row writes (theta_hat, phi_hat, d_hat) into the workspace (three planes of P
//     doubles).  The row's segment, hence its origin, is found by bisecting pred_start.  A prediction with d_hat <= 1e-2
//     takes no part: it is parked at theta_hat = +inf, where its squared distance is +inf and the strict `<` never takes it.
//   * match: workgroup (tile, segment), one lane per ground-truth ray.  The segment's (theta_hat, phi_hat) stream through
//     LDS in chunks of kChunk; all lanes of an instruction read the same LDS address (a broadcast: no bank conflict).  The
//     lane keeps (best distance, best row) under a strict `<` while the row counter ascends, so the lowest row wins ties,
//     as in the reference.  It then interpolates, clamps twice and forms its two terms with the header's functions; the
//     workgroup sums (L1, AbsRel, count) in a fixed tree and writes one row of `partial`.  No atomics: the result is a
//     function of the inputs alone.
// The only index formed from data is the loop counter that won the comparison; the starts are clamped to [0, P] / [0, G]
// whatever the device tables hold.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "vidar_hip.h"
#include "vidar_common.h"
#include "ray_eval_math.h"

namespace {

using namespace vidar_ray_eval;

constexpr int kThreads = 256;        // ground-truth rays of a tile
constexpr int kChunk = 1024;         // predictions in LDS at a time: 16 KiB

__global__ __launch_bounds__(kThreads) void ray_eval_project_kernel(const float* __restrict__ pred,
                                                                    const int32_t* __restrict__ pred_start,
                                                                    const float* __restrict__ origin,
                                                                    double* __restrict__ ws, int P, int S) {
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= P) return;
  // the last segment whose start is <= p (empty segments share a start: the last of them is followed by a larger one)
  int lo = 0, hi = S;                // invariant: start[lo] <= p (or lo == 0), start[hi] > p (or hi == S)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (pred_start[mid] <= p) lo = mid; else hi = mid;
  }
  const bool owned = pred_start[lo] <= p && p < pred_start[lo + 1];
  double theta = INFINITY, phi = 0.0, d = 0.0;
  if (owned) {
    spherical((double)pred[p * 3] - (double)origin[lo * 3], (double)pred[p * 3 + 1] - (double)origin[lo * 3 + 1],
              (double)pred[p * 3 + 2] - (double)origin[lo * 3 + 2], &theta, &phi, &d);
    if (!(d > kMinDist)) theta = INFINITY;
  }
  ws[p] = theta;
  ws[(int64_t)P + p] = phi;
  ws[2 * (int64_t)P + p] = d;
}

__global__ __launch_bounds__(kThreads) void ray_eval_match_kernel(
    const int32_t* __restrict__ pred_start, const float* __restrict__ gt, const int32_t* __restrict__ gt_start,
    const float* __restrict__ origin, const double* __restrict__ ws, double* __restrict__ partial,
    int32_t* __restrict__ nn_idx, double* __restrict__ ray_err, double* __restrict__ interp_out, int P, int G, int tiles) {
  __shared__ double s_theta[kChunk];
  __shared__ double s_phi[kChunk];
  __shared__ double s_sum[3][kThreads];
  const int tid = threadIdx.x;
  const int seg = blockIdx.x / tiles, tile = blockIdx.x - seg * tiles;
  const int g0 = min(max(gt_start[seg], 0), G), g1 = min(max(gt_start[seg + 1], g0), G);
  double* row = partial + (int64_t)blockIdx.x * 3;
  if ((int64_t)tile * kThreads >= g1 - g0) {            // beyond the segment: a zero row
    if (tid < 3) row[tid] = 0.0;
    return;
  }
  const int p0 = min(max(pred_start[seg], 0), P), p1 = min(max(pred_start[seg + 1], p0), P);
  const int g = g0 + tile * kThreads + tid;
  const bool have = g < g1;
  const double o[3] = {origin[seg * 3], origin[seg * 3 + 1], origin[seg * 3 + 2]};
  double pt[3] = {0.0, 0.0, 0.0}, theta = 0.0, phi = 0.0, d = 0.0;
  if (have) {
    for (int a = 0; a < 3; ++a) pt[a] = gt[(int64_t)g * 3 + a];
    spherical(pt[0] - o[0], pt[1] - o[1], pt[2] - o[2], &theta, &phi, &d);
  }
  const bool counted = have && d > kMinDist;

  double best = INFINITY;
  int best_row = -1;
  for (int c0 = p0; c0 < p1; c0 += kChunk) {
    const int n = min(kChunk, p1 - c0);
    __syncthreads();                                    // the previous chunk has been read by everyone
    for (int j = tid; j < n; j += kThreads) {
      s_theta[j] = ws[c0 + j];
      s_phi[j] = ws[(int64_t)P + c0 + j];
    }
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < n; ++j) {
      const double d2 = angular_d2(theta, phi, s_theta[j], s_phi[j]);
      if (d2 < best) {
        best = d2;
        best_row = c0 + j;
      }
    }
  }

  double l1 = 0.0, absrel = 0.0, ip[3] = {NAN, NAN, NAN};
  if (counted) {
    if (best_row < 0) {                                 // no kept prediction in the segment: the reference would raise
      l1 = absrel = NAN;
    } else {
      interpolate(pt, o, ws[2 * (int64_t)P + best_row], ip);
      error_terms(pt, ip, o, &l1, &absrel);
    }
  }
  if (have) {
    if (nn_idx != nullptr) nn_idx[g] = counted && best_row >= 0 ? best_row - p0 : -1;
    if (ray_err != nullptr) {
      ray_err[(int64_t)g * 2] = l1;
      ray_err[(int64_t)g * 2 + 1] = absrel;
    }
    if (interp_out != nullptr)
      for (int a = 0; a < 3; ++a) interp_out[(int64_t)g * 3 + a] = ip[a];
  }

  // fixed tree: lane t adds lane t + s for s = 128, 64, ..., 1
  s_sum[0][tid] = l1;
  s_sum[1][tid] = absrel;
  s_sum[2][tid] = counted ? 1.0 : 0.0;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (tid < s)
      for (int k = 0; k < 3; ++k) s_sum[k][tid] += s_sum[k][tid + s];
    __syncthreads();
  }
  if (tid < 3) row[tid] = s_sum[tid][0];
}

}  // namespace

extern "C" {

int vidar_ray_eval_workspace_bytes(int P, int64_t* bytes) {
  if (P < 0 || !bytes) return VIDAR_ERR_BAD_ARG;
  *bytes = (int64_t)P * 3 * (int64_t)sizeof(double);
  return 0;
}

int vidar_ray_eval_f64(const float* pred, const int32_t* pred_start, const float* gt, const int32_t* gt_start,
                       const float* origin, void* partial, int32_t* nn_idx, void* ray_err, void* interp, int P, int G,
                       int S, int max_gt, void* workspace, size_t workspace_bytes, void* stream) {
  VIDAR_ENTER();
  if (P < 0 || G < 0 || S < 0 || max_gt < 0) return VIDAR_ERR_BAD_ARG;
  if (S == 0 || G == 0) return 0;                       // nothing to score: no launch (partial has no row to write)
  const int64_t tiles = ((int64_t)max_gt + kThreads - 1) / kThreads;
  if (max_gt == 0 || tiles * S > INT_MAX || !pred_start || !gt || !gt_start || !origin || !partial || (P > 0 && !pred) ||
      (P > 0 && (!workspace || workspace_bytes < (size_t)P * 3 * sizeof(double))) || ((uintptr_t)workspace & 7u) != 0)
    return VIDAR_ERR_BAD_ARG;
  if (P > 0)
    hipLaunchKernelGGL(ray_eval_project_kernel, dim3((unsigned)(((int64_t)P + kThreads - 1) / kThreads)), dim3(kThreads),
                       0, (hipStream_t)stream, pred, pred_start, origin, (double*)workspace, P, S);
  hipLaunchKernelGGL(ray_eval_match_kernel, dim3((unsigned)(tiles * S)), dim3(kThreads), 0, (hipStream_t)stream, pred_start,
                     gt, gt_start, origin, (const double*)workspace, (double*)partial, nn_idx, (double*)ray_err,
                     (double*)interp, P, G, (int)tiles);
  return vidar_last_error();
}

}  // extern "C"
