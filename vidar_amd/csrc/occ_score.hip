// Score of a predicted occupancy evidence grid against a measured one, for many (sample, frame) segments in one call:
// the counts behind IoU / precision / recall per threshold, the Brier sum and a reliability histogram.  The per-voxel
// decisions are csrc/occ_score_math.h (fp32, every operation rounded on its own: -ffp-contract=off).
//
// Two launches, no floating-point atomics, no atomics at all:
//   * tiles: workgroup (tile, segment) reads its kTile voxels of the four planes once, 16 B per voxel.  Every column but
//     brier is a COUNT: a wave counts a predicate with one ballot and a population count, in integers, so the counts are
//     exact whatever the order.  A lane adds its brier terms (fp64) in voxel order; the wave sums the lanes in a fixed
//     butterfly, the workgroup its waves in wave order.  One row of `partial` [S, tiles, columns] f64 per workgroup.
//   * sum: wave (column, segment) adds the tiles in a fixed order -- lane l the tiles l, l + 64, ... in tile order, then
//     the lanes in the same butterfly -- and writes table [S, columns] f64.
// Counts stay below 2^31 and are exact in fp64; brier is a function of the inputs alone: equal inputs give equal bits.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "vidar_hip.h"
#include "vidar_common.h"
#include "occ_score_math.h"

namespace {

using namespace vidar_occ;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPerThread = 16;
constexpr int kTile = kThreads * kPerThread;      // voxels of a workgroup
constexpr int kMaxColumns = kFixedColumns + 3 * kMaxThresholds + 2 * kMaxBins;

struct ScoreArgs {
  float th[kMaxThresholds];
  float min_pred, min_meas, min_hits;
  int T, B;
};

__device__ __forceinline__ uint32_t wave_count(bool p) { return (uint32_t)__popcll(__ballot(p)); }

__global__ __launch_bounds__(kThreads) void occ_score_tile_kernel(const float* __restrict__ pred,
                                                                  const float* __restrict__ meas,
                                                                  double* __restrict__ partial, int V, int tiles,
                                                                  ScoreArgs a) {
  __shared__ double s_cols[kWaves][kMaxColumns];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile = blockIdx.x, seg = blockIdx.y;
  const float* hp = pred + (size_t)seg * 2 * (size_t)V;
  const float* fp = hp + V;
  const float* hm = meas + (size_t)seg * 2 * (size_t)V;
  const float* fm = hm + V;
  // wave-uniform counters; the loops below are fully unrolled, so every index is a constant
  uint32_t n_pred = 0, n_meas = 0, n_both = 0, n_occ = 0;
  uint32_t tp[kMaxThresholds] = {}, fpos[kMaxThresholds] = {}, fneg[kMaxThresholds] = {};
  uint32_t cnt[kMaxBins] = {}, pos[kMaxBins] = {};
  double brier = 0.0;
  const int64_t base = (int64_t)tile * kTile;
#pragma unroll 4
  for (int i = 0; i < kPerThread; ++i) {
    const int64_t idx = base + (int64_t)i * kThreads + tid;
    const bool in = idx < V;
    Voxel x{false, false, false, false, false, 0.f};
    if (in) x = classify(hp[idx], fp[idx], hm[idx], fm[idx], a.min_pred, a.min_meas, a.min_hits);
    n_pred += wave_count(x.pred);
    n_meas += wave_count(x.meas);
    n_both += wave_count(x.both);
    n_occ += wave_count(x.both && x.y);
    if (x.both) brier += brier_term(x.o_p, x.y);
#pragma unroll
    for (int j = 0; j < kMaxThresholds; ++j) {
      if (j < a.T) {
        const bool yhat = x.o_p >= a.th[j];
        tp[j] += wave_count(x.both && yhat && x.y);
        fpos[j] += wave_count(x.both && yhat && !x.y);
        fneg[j] += wave_count(x.both && !yhat && x.y);
      }
    }
    const int bin = x.both && a.B > 0 ? bin_of(x.o_p, a.B) : -1;
#pragma unroll
    for (int b = 0; b < kMaxBins; ++b) {
      if (b < a.B) {
        cnt[b] += wave_count(bin == b);
        pos[b] += wave_count(bin == b && x.y);
      }
    }
  }
  // lanes of a wave: a fixed butterfly, the same additions in every run
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) brier += __shfl_xor(brier, m, 64);
  if (lane == 0) {
    double* c = s_cols[wave];
    c[0] = n_pred; c[1] = n_meas; c[2] = n_both; c[3] = n_occ; c[4] = brier;
#pragma unroll
    for (int j = 0; j < kMaxThresholds; ++j)
      if (j < a.T) { c[5 + 3 * j] = tp[j]; c[6 + 3 * j] = fpos[j]; c[7 + 3 * j] = fneg[j]; }
#pragma unroll
    for (int b = 0; b < kMaxBins; ++b)
      if (b < a.B) { c[5 + 3 * a.T + 2 * b] = cnt[b]; c[6 + 3 * a.T + 2 * b] = pos[b]; }
  }
  __syncthreads();
  const int ncols = columns(a.T, a.B);
  if (tid < ncols) {
    double s = s_cols[0][tid];
    for (int w = 1; w < kWaves; ++w) s += s_cols[w][tid];
    partial[((size_t)seg * tiles + tile) * ncols + tid] = s;
  }
}

// wave (column, segment): lane l adds tiles l, l + 64, ... in tile order, the wave its lanes in the fixed butterfly -- the
// order is a function of the tile count alone (a single thread walking the tiles waits out one memory latency per tile)
__global__ __launch_bounds__(64) void occ_score_sum_kernel(const double* __restrict__ partial, double* __restrict__ table,
                                                           int tiles, int ncols) {
  const int c = blockIdx.x, seg = blockIdx.y, lane = threadIdx.x;
  const double* p = partial + (size_t)seg * tiles * ncols + c;
  double s = 0.0;
  for (int t = lane; t < tiles; t += 64) s += p[(size_t)t * ncols];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
  if (lane == 0) table[(size_t)seg * ncols + c] = s;
}

inline int64_t score_tiles(int V) { return ((int64_t)V + kTile - 1) / kTile; }
inline bool score_bad(int S, int V, int T, int B) {
  return S < 0 || V < 0 || T < 1 || T > kMaxThresholds || B < 0 || B > kMaxBins || S > 65535;
}

}  // namespace

extern "C" {

int vidar_occ_score_workspace_bytes(int S, int V, int T, int B, int64_t* bytes) {
  if (!bytes || score_bad(S, V, T, B)) return VIDAR_ERR_BAD_ARG;
  *bytes = (int64_t)S * score_tiles(V) * columns(T, B) * (int64_t)sizeof(double);
  return 0;
}

int vidar_occ_score_f32(const float* pred, const float* meas, const float* thresholds, void* table, int S, int V, int T,
                        int B, float min_pred_evidence, float min_meas_evidence, float min_hits, void* workspace,
                        size_t workspace_bytes, void* stream) {
  VIDAR_ENTER();
  if (score_bad(S, V, T, B) || !thresholds) return VIDAR_ERR_BAD_ARG;
  ScoreArgs a{};
  for (int j = 0; j < T; ++j) {
    if (thresholds[j] != thresholds[j]) return VIDAR_ERR_BAD_ARG;
    a.th[j] = thresholds[j];
  }
  if (min_pred_evidence != min_pred_evidence || min_meas_evidence != min_meas_evidence || min_hits != min_hits)
    return VIDAR_ERR_BAD_ARG;
  if (S == 0 || V == 0) return 0;                         // nothing to score: no launch (table has no voxel to count)
  const int64_t tiles = score_tiles(V);
  const int ncols = columns(T, B);
  if (!pred || !meas || !table || !workspace || ((uintptr_t)workspace & 7u) != 0 || ((uintptr_t)table & 7u) != 0 ||
      workspace_bytes < (size_t)S * (size_t)tiles * (size_t)ncols * sizeof(double))
    return VIDAR_ERR_BAD_ARG;
  a.min_pred = min_pred_evidence; a.min_meas = min_meas_evidence; a.min_hits = min_hits;
  a.T = T; a.B = B;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(occ_score_tile_kernel, dim3((unsigned)tiles, (unsigned)S), dim3(kThreads), 0, s, pred, meas,
                     (double*)workspace, V, (int)tiles, a);
  hipLaunchKernelGGL(occ_score_sum_kernel, dim3((unsigned)ncols, (unsigned)S), dim3(64), 0, s,
                     (const double*)workspace, (double*)table, (int)tiles, ncols);
  return vidar_last_error();
}

}  // extern "C"
