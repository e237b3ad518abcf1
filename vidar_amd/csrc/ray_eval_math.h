// Per-ray arithmetic of the 4d-occ ray errors (L1 / AbsRel along the ground-truth rays), fp64: the reference's
// bevformer/utils/eval_utils.py:21-225 (inside_volume, clamp / _clamp, spherical_projection, compute_ray_errors) for ONE
// ray, with its operation order.
//
// Plain C++ on purpose: ray_eval.hip evaluates it per lane, and tests/ray_eval_host.cpp compiles the very same text with
// g++ so that the CPU test-suite can compare it with the reference's own numpy results (tests/golden/ray_eval_cases.npz)
// on a machine without a GPU.  Compile with -ffp-contract=off: every operation rounds on its own, as numpy's do.
//
// What the reference does per ray and this header restates:
//   * spherical_projection (:177-182): azimuth atan2(x, y), elevation atan2(z, y) -- y in both --, d = sqrt(x*x + y*y +
//     z*z) summed left to right.
//   * clamp (:39-78): a point inside the closed PC_RANGE box is left alone.  Otherwise _clamp (:81-174): the ray
//     origin -> point is cut to the box widened by 0.02 ("the volume").  A plane distance is (bound - start) / dir, 1e8
//     where |dir| <= 1e-8 (np.isclose against 0); a plane qualifies iff t + 1e-4 >= 0 and start + t * dir lies in the
//     volume.  The reference walks the six planes in ascending t and stops at the first that qualifies, i.e. takes the
//     minimum qualifying t (equal t give the same point: no sort is needed).  Stage 1 (origin outside the volume) moves
//     the ray origin to the entry point, or declares the ray invalid (everything +inf) when it misses; a point in front
//     of the entry (t > l) becomes the entry point.  Stage 2 (point outside the volume) moves the point back along the
//     ray to the first qualifying plane.
//   * compute_ray_errors (:185-225): interp = origin + d_hat[nn] * unit(gt - origin); both the ground truth and the
//     interpolated point are clamped (the second one's invalid flag is ignored); rays whose clamped ground truth is
//     invalid, or whose clamped length is <= 0.01, contribute nothing.
// PC_RANGE is the metric's own (:11), not the model's.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define VIDAR_RAY_EVAL_FN __host__ __device__ __forceinline__
#else
#define VIDAR_RAY_EVAL_FN inline
#endif

namespace vidar_ray_eval {

constexpr double kMinDist = 1e-2;      // rays (predicted and ground truth) at most this long take no part (:191-192)
constexpr double kMinClamped = 0.01;   // clamped ground-truth rays at most this long contribute nothing (:217)
constexpr double kShell = 0.02;        // the volume is the box widened by this (:24)
constexpr double kMaxValue = 1e8;      // plane distance of a ray parallel to the plane (:12)

VIDAR_RAY_EVAL_FN double box_lo(int a) { return a == 2 ? -4.5 : -70.0; }
VIDAR_RAY_EVAL_FN double box_hi(int a) { return a == 2 ? 4.5 : 70.0; }

// sqrt(x*x + y*y + z*z), left to right: every length of the metric
VIDAR_RAY_EVAL_FN double norm3(double x, double y, double z) { return sqrt(x * x + y * y + z * z); }

// (azimuth, elevation, distance) of a point relative to its origin
VIDAR_RAY_EVAL_FN void spherical(double x, double y, double z, double* theta, double* phi, double* d) {
  *d = norm3(x, y, z);
  *theta = atan2(x, y);
  *phi = atan2(z, y);
}

// squared angular distance the nearest-neighbour search compares; the reference's third coordinate (1 against 1) adds 0
VIDAR_RAY_EVAL_FN double angular_d2(double theta, double phi, double theta_hat, double phi_hat) {
  const double dt = theta - theta_hat, dp = phi - phi_hat;
  return dt * dt + dp * dp;
}

VIDAR_RAY_EVAL_FN bool in_box(const double* p) {
  bool in = true;
  for (int a = 0; a < 3; ++a) in = in && box_lo(a) <= p[a] && p[a] <= box_hi(a);
  return in;
}

VIDAR_RAY_EVAL_FN bool in_volume(const double* p) {
  bool in = true;
  for (int a = 0; a < 3; ++a) in = in && box_lo(a) - kShell <= p[a] && p[a] <= box_hi(a) + kShell;
  return in;
}

VIDAR_RAY_EVAL_FN double plane_t(double bound, double start, double dir) {
  return fabs(dir) <= 1e-8 ? kMaxValue : (bound - start) / dir;
}

// the qualifying plane crossing of the ray start + t * dir with the smallest t; false when no plane qualifies
VIDAR_RAY_EVAL_FN bool first_hit(const double* start, const double* dir, double* hit, double* t_hit) {
  bool found = false;
  double best = 0.0;
  for (int k = 0; k < 6; ++k) {
    const int a = k >> 1;
    const double t = plane_t((k & 1) ? box_hi(a) : box_lo(a), start[a], dir[a]);
    if (!(t + 1e-4 >= 0.0)) continue;
    double p[3];
    for (int b = 0; b < 3; ++b) p[b] = start[b] + t * dir[b];
    if (in_volume(p) && (!found || t < best)) {
      found = true;
      best = t;
      for (int b = 0; b < 3; ++b) hit[b] = p[b];
    }
  }
  *t_hit = best;
  return found;
}

// clamp(point, origin) for one ray: `point` is rewritten, `ray_origin` written; -> the ray is invalid
VIDAR_RAY_EVAL_FN bool clamp_ray(double* point, const double* origin, double* ray_origin) {
  for (int a = 0; a < 3; ++a) ray_origin[a] = origin[a];
  if (in_box(point)) return false;
  double v[3], dir[3];
  for (int a = 0; a < 3; ++a) v[a] = point[a] - origin[a];
  const double l = norm3(v[0], v[1], v[2]);
  for (int a = 0; a < 3; ++a) dir[a] = v[a] / l;
  if (!in_volume(origin)) {
    double hit[3], t;
    if (!first_hit(origin, dir, hit, &t)) {
      for (int a = 0; a < 3; ++a) point[a] = ray_origin[a] = INFINITY;
      return true;
    }
    for (int a = 0; a < 3; ++a) ray_origin[a] = hit[a];
    if (t > l)
      for (int a = 0; a < 3; ++a) point[a] = hit[a];
  }
  if (!in_volume(point)) {
    double back[3], hit[3], t;
    for (int a = 0; a < 3; ++a) back[a] = -dir[a];
    if (first_hit(point, back, hit, &t))      // the reference asserts that one exists
      for (int a = 0; a < 3; ++a) point[a] = hit[a];
  }
  return (isinf(point[0]) && isinf(point[1]) && isinf(point[2])) || (isnan(point[0]) && isnan(point[1]) && isnan(point[2]));
}

// origin + d_hat * unit(gt - origin): the prediction moved onto the ground-truth ray
VIDAR_RAY_EVAL_FN void interpolate(const double* gt, const double* origin, double d_hat, double* out) {
  double v[3];
  for (int a = 0; a < 3; ++a) v[a] = gt[a] - origin[a];
  const double n = norm3(v[0], v[1], v[2]);
  for (int a = 0; a < 3; ++a) out[a] = origin[a] + d_hat * (v[a] / n);
}

// the L1 and AbsRel terms of one counted ground-truth ray; -> false (both 0) when the ray is invalid or too short
// after clamping
VIDAR_RAY_EVAL_FN bool error_terms(const double* gt, const double* interp, const double* origin, double* l1,
                                   double* absrel) {
  double g[3], p[3], g_origin[3], p_origin[3];
  for (int a = 0; a < 3; ++a) {
    g[a] = gt[a];
    p[a] = interp[a];
  }
  const bool invalid = clamp_ray(g, origin, g_origin);
  clamp_ray(p, origin, p_origin);
  *l1 = *absrel = 0.0;
  if (invalid) return false;
  const double dc = norm3(g[0] - g_origin[0], g[1] - g_origin[1], g[2] - g_origin[2]);
  if (!(dc > kMinClamped)) return false;
  const double e = norm3(g[0] - p[0], g[1] - p[1], g[2] - p[2]);
  *l1 = e;
  *absrel = e / dc;
  return true;
}

}  // namespace vidar_ray_eval
