// The five true-positive errors of the nuScenes detection metric for ONE matched (ground truth, prediction) pair, fp32.
//
// Plain C++ on purpose: det_eval.hip evaluates them per lane, and tests/det_eval_host.cpp compiles the very same text
// with g++ so that the CPU test-suite can compare them with the fp64 restatement in tests/det_eval_cases.py on a machine
// without a GPU.  Compile with -ffp-contract=off: every operation rounds on its own.
//
// Semantics RECALLED from the nuScenes devkit (eval/common/utils.py: center_distance, velocity_l2, scale_iou, yaw_diff /
// angle_diff, attr_acc; eval/detection/algo.py: accumulate) -- the devkit is not part of the reference tree and is not
// installable here, so none of this is pinned to it; the reference only calls it (datasets/nuscnes_eval.py:628-676).
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define VIDAR_DET_EVAL_FN __host__ __device__ __forceinline__
#else
#define VIDAR_DET_EVAL_FN inline
#endif

namespace vidar_det_eval {

constexpr int kBox = 9;   // x, y, z, three sizes, yaw, vx, vy
constexpr int kErr = 5;   // trans_err, vel_err, scale_err, orient_err, attr_err -- the column order of err[P, 5]
constexpr float kPi = 3.14159265358979323846f;

// squared centre distance on x and y: what the matcher compares (and takes the root of for trans_err)
VIDAR_DET_EVAL_FN float centre_d2(float px, float py, float gx, float gy) {
  const float dx = px - gx, dy = py - gy;
  return dx * dx + dy * dy;
}

VIDAR_DET_EVAL_FN float trans_err(const float* gt, const float* pr) { return sqrtf(centre_d2(pr[0], pr[1], gt[0], gt[1])); }

// L2 of the velocity differences; a NaN ground-truth (or predicted) velocity gives NaN
VIDAR_DET_EVAL_FN float vel_err(const float* gt, const float* pr) {
  const float dx = pr[7] - gt[7], dy = pr[8] - gt[8];
  return sqrtf(dx * dx + dy * dy);
}

// 1 - IoU of the two boxes aligned at a corner with equal orientation
VIDAR_DET_EVAL_FN float scale_err(const float* gt, const float* pr) {
  const float va = gt[3] * gt[4] * gt[5], vr = pr[3] * pr[4] * pr[5];
  const float inter = fminf(gt[3], pr[3]) * fminf(gt[4], pr[4]) * fminf(gt[5], pr[5]);
  return 1.0f - inter / (va + vr - inter);
}

// |((yg - yp + T/2) mod T) - T/2| with the floored modulo (result in [0, T)); T = pi for barriers (a barrier turned by
// pi is the same barrier), 2 pi otherwise
VIDAR_DET_EVAL_FN float orient_err(const float* gt, const float* pr, bool half_period) {
  const float T = half_period ? kPi : 2.0f * kPi;
  float r = fmodf(gt[6] - pr[6] + 0.5f * T, T);
  if (r < 0.0f) r += T;
  float d = r - 0.5f * T;
  if (d > kPi) d -= 2.0f * kPi;
  return fabsf(d);
}

// 1 - (the attribute ids agree); NaN where the ground truth carries no attribute (id < 0)
VIDAR_DET_EVAL_FN float attr_err(int32_t gt_attr, int32_t pr_attr) {
  return gt_attr < 0 ? NAN : (gt_attr == pr_attr ? 0.0f : 1.0f);
}

VIDAR_DET_EVAL_FN void pair_errors(const float* gt, int32_t gt_attr, const float* pr, int32_t pr_attr, bool half_period,
                                   float* out /*[kErr]*/) {
  out[0] = trans_err(gt, pr);
  out[1] = vel_err(gt, pr);
  out[2] = scale_err(gt, pr);
  out[3] = orient_err(gt, pr, half_period);
  out[4] = attr_err(gt_attr, pr_attr);
}

}  // namespace vidar_det_eval
