// Per-ray and per-voxel arithmetic of the occupancy score: the measured evidence of a sweep (ray_march.hip,
// sweep_evidence_body) and the comparison of a predicted with a measured evidence grid (occ_score.hip).
//
// Plain C++ on purpose, like det_eval_math.h and ray_eval_math.h: the kernels evaluate it per lane, and
// tests/occ_score_host.cpp compiles the very same text with g++ so that the CPU suite can hold it against a torch
// restatement on a machine without a GPU.  Compile with -ffp-contract=off: every fp32 operation rounds on its own, as
// torch's do, so both sides take the same decision on every voxel -- also on one that sits exactly on a floor.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define VIDAR_OCC_FN __host__ __device__ __forceinline__
#else
#define VIDAR_OCC_FN inline
#endif

namespace vidar_occ {

constexpr int kMaxThresholds = 8;
constexpr int kMaxBins = 16;
constexpr int kFixedColumns = 5;   // n_pred, n_meas, n_both, n_occ, brier

// columns of a table row: 5 + 3 T + 2 B
VIDAR_OCC_FN int columns(int T, int B) { return kFixedColumns + 3 * T + 2 * B; }

// ---- the measured side: a beam of length L (voxel units) that returned ------------------------------------------------
// a_k: how much of the step behind waypoint k (at (k + 0.5) step from the origin) the beam had behind it when it
// returned: 1 well before the return, 0 from the return on, a ramp in between -- continuous in L and in the waypoint.
VIDAR_OCC_FN float beam_weight(float L, int k, float step) {
  const float a = (L - ((float)k + 0.5f) * step) / step;
  return a < 0.f ? 0.f : (a > 1.f ? 1.f : a);            // NaN (step == 0 at the return) falls through as NaN
}
// Waypoints to march: a_k == 0 for every k >= L / step - 0.5, so min(K, ceil(L / step + 0.5)) leaves out none that adds
// (a whole waypoint of slack against the rounding of the quotient).  L finite and > 0.
VIDAR_OCC_FN int beam_trips(float L, float step, int K) {
  const float t = ceilf(L / step + 0.5f);
  if (!(t < (float)K)) return K;                          // also NaN, +inf
  return t > 0.f ? (int)t : 0;
}

// ---- the comparison: one voxel, fp32, every operation rounded on its own ----------------------------------------------
struct Voxel {
  bool finite;   // all four planes finite; a voxel that is not takes part in no column
  bool pred;     // the predicted evidence reaches its floor
  bool meas;     // the measured evidence reaches its floor
  bool both;
  bool y;        // a return was measured in this cell (whatever the free evidence says)
  float o_p;     // predicted occupancy hit_p / ev_p; only meaningful under `both`
};

VIDAR_OCC_FN bool finite_f(float v) { return v - v == 0.f; }

VIDAR_OCC_FN Voxel classify(float hit_p, float free_p, float hit_m, float free_m, float min_pred_evidence,
                            float min_meas_evidence, float min_hits) {
  Voxel x;
  x.finite = finite_f(hit_p) && finite_f(free_p) && finite_f(hit_m) && finite_f(free_m);
  const float ev_p = hit_p + free_p, ev_m = hit_m + free_m;
  x.o_p = hit_p / ev_p;
  x.pred = x.finite && ev_p >= min_pred_evidence;
  x.meas = x.finite && ev_m >= min_meas_evidence;
  x.both = x.pred && x.meas;
  x.y = hit_m >= min_hits;
  return x;
}

// reliability bin of o_p: min(int(o_p * B), B - 1); an o_p below 0 or NaN (0 / 0 under a floor of 0) goes to bin 0
VIDAR_OCC_FN int bin_of(float o_p, int B) {
  const float s = o_p * (float)B;
  if (!(s >= 0.f)) return 0;
  return s < (float)B ? (int)s : B - 1;
}

// the voxel's term of the Brier sum, fp64
VIDAR_OCC_FN double brier_term(float o_p, bool y) {
  const double d = (double)o_p - (y ? 1.0 : 0.0);
  return d * d;
}

}  // namespace vidar_occ
