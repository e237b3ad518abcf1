// Per-waypoint weights of the occupancy query (ray_march.hip, point_occupancy_body): how much of waypoint k's stretch of
// a ray lies inside, and how much beyond, the stretch a query at length L owns.
//
// Plain C++ on purpose, like cam_ray.h and occ_score_math.h: the kernels evaluate it per lane, and tests/occ_at_host.cpp
// compiles the very same text with g++ (under the address and undefined-behaviour sanitizers) and holds it against fp64.
// Compile with -ffp-contract=off: every fp32 operation rounds on its own, so the listed and the per-voxel form, the
// register and the streamed form give the same bits.
#pragma once
#include <math.h>

#ifdef __HIPCC__
#define VIDAR_OCC_AT_FN __host__ __device__ __forceinline__
#else
#define VIDAR_OCC_AT_FN inline
#endif

namespace vidar_occ_at {

// Waypoint k owns [k step, (k + 1) step) of the ray.  How much of that stretch lies before `edge`, as a fraction of it:
// 0 while the edge is at or before the stretch, 1 once it is past it, a ramp inside -- continuous in the edge.
VIDAR_OCC_AT_FN float covered(float edge, int k, float step) {
  const float a = (edge - (float)k * step) / step;
  return a < 0.f ? 0.f : (a > 1.f ? 1.f : a);              // NaN falls through as NaN
}

struct Weights {
  float hit;    // fraction of the stretch inside the query's [L - extent/2, L + extent/2]
  float free;   // fraction beyond it: a return there means the ray passed the query
};

// hit + free = 1 - covered(L - extent/2): what is left is the part of the stretch BEFORE the query.  Both are >= 0 (the
// far edge is never before the near one, and the clamp is monotonic), and free is formed from the far edge alone, never
// as 1 - (before + hit).
VIDAR_OCC_AT_FN Weights weights(float L, float extent, int k, float step) {
  const float half = extent / 2.f;
  const float c_near = covered(L - half, k, step), c_far = covered(L + half, k, step);
  return Weights{c_far - c_near, 1.f - c_far};
}

// extent must be a finite length > 0
VIDAR_OCC_AT_FN bool bad_extent(float extent) { return !(extent > 0.f) || !(extent - extent == 0.f); }

}  // namespace vidar_occ_at
