// Matching step of the nuScenes detection metric (mAP / NDS): greedy, confidence-ordered nearest-centre matching of the
// predictions against the annotations, for every distance threshold at once.  The reference hands the whole metric to
// the nuScenes devkit (datasets/nuscnes_eval.py:628-676), which walks it as nested Python loops once per (class,
// threshold); the semantics below are RECALLED from the devkit's `accumulate` (it is not part of the reference tree).
//
// Ownership rule: a match only interacts with other matches of the same (sample, class, threshold) -- the devkit's
// `taken` set is keyed by the sample and a pass has one class.  So ONE WAVE owns one (segment, threshold), segment =
// (sample, class): waves never share state, there is no atomic, no barrier and no LDS, and the result is a function of
// the inputs alone.
//
// Kernel notes (gfx950, wave64):
//   * the wave walks its segment's predictions in processing order (prepared by the caller: score descending, equal
//     scores with the later input index first).  Predictions are fetched 64 at a time, one per lane, and broadcast one
//     after the other with v_readlane (the loop counter is wave-uniform); every lane keeps the verdict of "its"
//     prediction in a register, so `match` is written 64 rows at a time and the five errors of the true-positive
//     threshold are evaluated by 64 lanes in parallel after the sequential part.
//   * the lanes hold the segment's annotations: lane l owns rows l, l + 64, ...  Up to 256 rows (1 or 4 chunks) stay in
//     registers with their taken flags as bits of one register; larger segments are streamed from memory with the
//     taken state kept in `gt_match` (a lane only ever reads back the flags it wrote itself).  Any count works.
//   * per prediction: squared centre distance in fp32 to the untaken rows (dx*dx + dy*dy, no contraction: this file is
//     built with -ffp-contract=off), wave minimum of the 64-bit key (distance bits << 32 | row) by an unsigned butterfly
//     -- distances are non-negative, so the integer order is the float order and the lowest row wins ties.  The nearest
//     untaken row is chosen FIRST and only then tested against the threshold (strictly), as in the devkit: a prediction
//     whose nearest untaken row is too far is a false positive even when a taken one is nearer.
//   * a NaN distance never matches (its key is above every finite one and fails the `<`).
//   * empty segments cost two loads per wave; a segment without annotations writes its -1 rows 64 at a time.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "vidar_hip.h"
#include "vidar_common.h"
#include "det_eval_math.h"

namespace {

using namespace vidar_det_eval;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxT = 8;             // distance thresholds per call

struct Ths {
  float th2[kMaxT];                  // squared thresholds
};

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(v, off, 64);
    v = o < v ? o : v;
  }
  return v;
}

__device__ __forceinline__ float bcast(float v, int src_lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src_lane));
}

// CH > 0: the segment's n <= 64 * CH annotations in CH register chunks; CH == 0: streamed from memory, any n.
// match_t / gtm_t: this threshold's rows of match / gt_match; err: non-NULL in the wave of the true-positive threshold.
template <int CH>
__device__ __forceinline__ void walk_segment(const float* __restrict__ pred_box, const int32_t* __restrict__ pred_attr,
                                             const float* __restrict__ gt_box, const int32_t* __restrict__ gt_attr,
                                             int32_t* match_t, int32_t* gtm_t, float* err, int p0, int p1, int g0, int n,
                                             float th2, bool half_period, int lane) {
  constexpr int R = CH > 0 ? CH : 1;
  float gx[R], gy[R];
  uint32_t taken = 0;                // bit c: row c * 64 + lane is matched (or does not exist)
  if (CH > 0) {
#pragma unroll
    for (int c = 0; c < R; ++c) {
      const int g = c * 64 + lane;
      gx[c] = gy[c] = 0.0f;
      if (g < n) {
        gx[c] = gt_box[(int64_t)(g0 + g) * kBox];
        gy[c] = gt_box[(int64_t)(g0 + g) * kBox + 1];
      } else {
        taken |= 1u << c;
      }
    }
  }
  for (int g = lane; g < n; g += 64) gtm_t[g0 + g] = -1;
  for (int pb = p0; pb < p1; pb += 64) {
    const int p = pb + lane;
    const bool have = p < p1;
    const float px_l = have ? pred_box[(int64_t)p * kBox] : 0.0f;
    const float py_l = have ? pred_box[(int64_t)p * kBox + 1] : 0.0f;
    const int nb = min(64, p1 - pb);
    int mine = -1;
    for (int j = 0; j < nb; ++j) {
      const float px = bcast(px_l, j), py = bcast(py_l, j);
      unsigned long long best = ~0ull;
      if (CH > 0) {
#pragma unroll
        for (int c = 0; c < R; ++c)
          if (!((taken >> c) & 1u)) {
            const unsigned long long key =
                ((unsigned long long)__float_as_uint(centre_d2(px, py, gx[c], gy[c])) << 32) | (uint32_t)(c * 64 + lane);
            best = key < best ? key : best;
          }
      } else {
        for (int g = lane; g < n; g += 64)
          if (gtm_t[g0 + g] < 0) {
            const float* b = gt_box + (int64_t)(g0 + g) * kBox;
            const unsigned long long key =
                ((unsigned long long)__float_as_uint(centre_d2(px, py, b[0], b[1])) << 32) | (uint32_t)g;
            best = key < best ? key : best;
          }
      }
      best = wave_min_u64(best);
      const int idx = (int)(uint32_t)best;
      const bool hit = best != ~0ull && __uint_as_float((uint32_t)(best >> 32)) < th2;     // wave-uniform
      if (hit) {
        if ((idx & 63) == lane) {
          if (CH > 0) taken |= 1u << (idx >> 6);
          gtm_t[g0 + idx] = pb + j;
        }
        if (lane == j) mine = g0 + idx;
      }
    }
    if (have) {
      match_t[p] = mine;
      if (err != nullptr) {
        float e[kErr];
        if (mine >= 0) {
          pair_errors(gt_box + (int64_t)mine * kBox, gt_attr ? gt_attr[mine] : -1, pred_box + (int64_t)p * kBox,
                      pred_attr ? pred_attr[p] : -1, half_period, e);
        } else {
#pragma unroll
          for (int k = 0; k < kErr; ++k) e[k] = NAN;
        }
#pragma unroll
        for (int k = 0; k < kErr; ++k) err[(int64_t)p * kErr + k] = e[k];
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void det_eval_match_kernel(
    const float* __restrict__ pred_box, const int32_t* __restrict__ pred_attr, const int32_t* __restrict__ pred_start,
    const float* __restrict__ gt_box, const int32_t* __restrict__ gt_attr, const int32_t* __restrict__ gt_start,
    int32_t* match, int32_t* gt_match, float* err, Ths ths, int P, int G, int NS, int NT, int tp_index, int num_classes,
    int barrier_class) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (w >= (int64_t)NS * NT) return;
  const int seg = (int)(w / NT), t = (int)(w - (int64_t)seg * NT);
  // the starts come from the device: whatever they hold, no access leaves [0, P) / [0, G)
  const int p0 = min(max(pred_start[seg], 0), P), p1 = min(max(pred_start[seg + 1], p0), P);
  const int g0 = min(max(gt_start[seg], 0), G), g1 = min(max(gt_start[seg + 1], g0), G);
  const int n = g1 - g0;
  if (p1 == p0 && n == 0) return;
  int32_t* match_t = match + (int64_t)t * P;
  int32_t* gtm_t = gt_match + (int64_t)t * G;
  float* err_t = t == tp_index ? err : nullptr;
  if (n == 0) {                      // nothing to match against: every prediction is a false positive
    for (int p = p0 + lane; p < p1; p += 64) {
      match_t[p] = -1;
      if (err_t != nullptr)
        for (int k = 0; k < kErr; ++k) err_t[(int64_t)p * kErr + k] = NAN;
    }
    return;
  }
  const bool half_period = seg % num_classes == barrier_class;
  const float th2 = ths.th2[t];
  if (n <= 64)
    walk_segment<1>(pred_box, pred_attr, gt_box, gt_attr, match_t, gtm_t, err_t, p0, p1, g0, n, th2, half_period, lane);
  else if (n <= 256)
    walk_segment<4>(pred_box, pred_attr, gt_box, gt_attr, match_t, gtm_t, err_t, p0, p1, g0, n, th2, half_period, lane);
  else
    walk_segment<0>(pred_box, pred_attr, gt_box, gt_attr, match_t, gtm_t, err_t, p0, p1, g0, n, th2, half_period, lane);
}

}  // namespace

extern "C" {

int vidar_det_eval_match_f32(const float* pred_box, const int32_t* pred_attr, const int32_t* pred_start,
                             const float* gt_box, const int32_t* gt_attr, const int32_t* gt_start, const float* dist_ths,
                             int32_t* match, int32_t* gt_match, float* err, int P, int G, int NS, int NT, int tp_index,
                             int num_classes, int barrier_class, void* stream) {
  VIDAR_ENTER();
  if (P < 0 || G < 0 || NS < 0 || NT < 0 || NT > kMaxT || num_classes <= 0 || tp_index < -1 || tp_index >= max(NT, 1) ||
      (int64_t)NS * max(NT, 1) > (int64_t)INT_MAX * kWaves)
    return VIDAR_ERR_BAD_ARG;
  if (NS == 0 || NT == 0 || (P == 0 && G == 0)) return 0;      // nothing to write: no launch on an empty grid
  if (!pred_start || !gt_start || !dist_ths || (P > 0 && (!pred_box || !match)) || (G > 0 && (!gt_box || !gt_match)) ||
      (P > 0 && tp_index >= 0 && !err))
    return VIDAR_ERR_BAD_ARG;
  Ths ths;
  for (int t = 0; t < kMaxT; ++t) ths.th2[t] = t < NT ? dist_ths[t] * dist_ths[t] : 0.0f;
  const int64_t waves = (int64_t)NS * NT;
  hipLaunchKernelGGL(det_eval_match_kernel, dim3((unsigned)((waves + kWaves - 1) / kWaves)), dim3(kThreads), 0,
                     (hipStream_t)stream, pred_box, pred_attr, pred_start, gt_box, gt_attr, gt_start, match, gt_match,
                     err, ths, P, G, NS, NT, tp_index, num_classes, barrier_class);
  return vidar_last_error();
}

}  // extern "C"
