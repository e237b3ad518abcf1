// csrc/occ_at_math.h on the host: the weights of the occupancy query held against the same formula in fp64.
// A stand-alone program (tests/test_voxel_occupancy_cpu.py builds it with g++ -ffp-contract=off, under the address and
// undefined-behaviour sanitizers where the toolchain has them) -- it prints what it measured and returns 1 on a miss.
//
// Tolerance, from the number format alone: with M = max(L + extent/2, K step), each of {L -+ extent/2, k step, their
// difference} carries at most 2^-24 M, the quotient by step one more relative 2^-24, so an edge's coverage is within
// tol_c = (3 M / step + 1) 2^-24 of its fp64 value; hit is a difference of two of them, free one against 1.
#include <math.h>
#include <stdio.h>

#include "occ_at_math.h"

namespace {

int g_failures = 0;

void expect(bool ok, const char* what, double a, double b, double c) {
  if (ok) return;
  ++g_failures;
  if (g_failures <= 20) printf("MISS %s: %.9g %.9g %.9g\n", what, a, b, c);
}

double clamp01(double a) { return a < 0.0 ? 0.0 : (a > 1.0 ? 1.0 : a); }

struct Ref { double before, hit, free; };

Ref ref(float L, float extent, int k, float step) {
  const double half = (double)extent / 2.0, lo = (double)k * (double)step;
  const double c_near = clamp01(((double)L - half - lo) / (double)step), c_far = clamp01(((double)L + half - lo) / (double)step);
  return Ref{c_near, c_far - c_near, 1.0 - c_far};
}

// every waypoint of one query: the weights against fp64, their signs, partition of unity; returns sum_k hit in fp64 of
// the fp32 weights
double sweep(float L, float extent, float step, int K, double* max_err, int* nonzero_hits) {
  const double eps = ldexp(1.0, -24);
  const double M = fmax((double)L + (double)extent / 2.0, (double)K * (double)step);
  const double tol_c = (3.0 * M / (double)step + 1.0) * eps, tol = 2.0 * tol_c + 2.0 * eps;
  double sum_hit = 0.0;
  *nonzero_hits = 0;
  for (int k = 0; k < K; ++k) {
    const vidar_occ_at::Weights w = vidar_occ_at::weights(L, extent, k, step);
    const float before = vidar_occ_at::covered(L - extent / 2.f, k, step);
    const Ref r = ref(L, extent, k, step);
    const double eh = fabs((double)w.hit - r.hit), ef = fabs((double)w.free - r.free);
    if (eh > *max_err) *max_err = eh;
    if (ef > *max_err) *max_err = ef;
    expect(eh <= tol && ef <= tol, "weight against fp64 (k, err hit, err free)", k, eh, ef);
    expect(w.hit >= 0.f && w.free >= 0.f && w.hit <= 1.f && w.free <= 1.f, "range (k, hit, free)", k, w.hit, w.free);
    expect(fabs((double)before + (double)w.hit + (double)w.free - 1.0) <= 4.0 * eps, "partition of unity (k, hit, free)", k,
           w.hit, w.free);
    sum_hit += (double)w.hit;
    *nonzero_hits += w.hit != 0.f;
  }
  return sum_hit;
}

}  // namespace

int main() {
  double max_err = 0.0;
  int nz = 0;
  const float steps[] = {1.f, 0.2f, 0.5f, 0.25f, 0.125f, 3.f};
  const float extents[] = {0.3f, 1.f, 2.5f};
  const int Ks[] = {512, 512, 64, 65, 1026, 5};
  int queries = 0;
  for (int s = 0; s < 6; ++s)
    for (float extent : extents)
      for (int i = 0; i < 400; ++i) {
        const float L = 0.013f + 0.2371f * (float)i;                   // 0.013 .. 94.6: before, inside and beyond K step
        const float step = steps[s];
        const int K = Ks[s];
        const double sum_hit = sweep(L, extent, step, K, &max_err, &nz);
        // the query's stretch, clipped to the marched range [0, K step], in units of step
        const double lo = fmax((double)L - (double)extent / 2.0, 0.0), hi = fmin((double)L + (double)extent / 2.0, (double)K * step);
        const double want = fmax(hi - lo, 0.0) / (double)step;
        const double M = fmax((double)L + extent, (double)K * step);
        expect(fabs(sum_hit - want) <= 8.0 * (3.0 * M / step + 1.0) * ldexp(1.0, -24), "sum of hit (L, got, want)", L, sum_hit,
               want);
        ++queries;
      }
  printf("weights against fp64: %d queries, max error %.3g\n", queries, max_err);

  // L < extent/2: the near edge lies behind the origin -- nothing is `before`, waypoint 0 is hit from its start
  {
    const float L = 0.3f, extent = 1.f, step = 0.25f;
    for (int k = 0; k < 8; ++k) {
      expect(vidar_occ_at::covered(L - extent / 2.f, k, step) == 0.f, "near edge behind the origin (k)", k, 0, 0);
      const vidar_occ_at::Weights w = vidar_occ_at::weights(L, extent, k, step);
      expect(w.hit == (k < 3 ? 1.f : 0.f) || k == 3, "L < extent/2: waypoints 0..2 are wholly hit (k, hit)", k, w.hit, 0);
      expect(k < 4 || w.free == 1.f, "L < extent/2: beyond the far edge all is free (k, free)", k, w.free, 0);
    }
    const double sum_hit = sweep(L, extent, step, 8, &max_err, &nz);
    expect(fabs(sum_hit - 0.8 / 0.25) <= 1e-5, "L < extent/2: the hit stretch is L + extent/2 (got, want)", sum_hit, 3.2, 0);
  }
  // L - extent/2 >= K step: every marched waypoint lies before the query -- exact zeros
  {
    const float step = 0.25f, extent = 1.f;
    const int K = 65;                                                  // K step = 16.25
    const float Ls[] = {16.75f, 17.f, 40.f, 3e30f};
    for (float L : Ls)
      for (int k = 0; k < K; ++k) {
        const vidar_occ_at::Weights w = vidar_occ_at::weights(L, extent, k, step);
        expect(w.hit == 0.f && w.free == 0.f, "beyond the marched range (L, k, hit)", L, k, w.hit);
      }
    const vidar_occ_at::Weights last = vidar_occ_at::weights(16.625f, extent, K - 1, step);   // half a waypoint earlier
    expect(last.hit == 0.5f && last.free == 0.f, "just inside the marched range (hit, free)", last.hit, last.free, 0);
  }
  // step > extent: the query is shorter than a waypoint's stretch -- at most two waypoints see it, extent / step in all
  {
    const float step = 3.f, extent = 1.f;
    for (int i = 0; i < 60; ++i) {
      const float L = 2.f + 0.25f * (float)i;
      const double sum_hit = sweep(L, extent, step, 8, &max_err, &nz);
      expect(nz >= 1 && nz <= 2, "step > extent: waypoints that see the query (L, n)", L, nz, 0);
      expect(fabs(sum_hit - 1.0 / 3.0) <= 1e-5, "step > extent: extent / step in all (L, got)", L, sum_hit, 0);
    }
  }
  // the extent check of the entry points
  {
    const float bad[] = {0.f, -1.f, NAN, INFINITY, -INFINITY};
    for (float e : bad) expect(vidar_occ_at::bad_extent(e), "bad extent", e, 0, 0);
    const float good[] = {1e-30f, 0.3f, 1.f, 3e38f};
    for (float e : good) expect(!vidar_occ_at::bad_extent(e), "good extent", e, 0, 0);
  }
  printf("%d checks missed\n", g_failures);
  return g_failures ? 1 : 0;
}
