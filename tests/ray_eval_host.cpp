// TEST INFRASTRUCTURE.  Compiles vidar_amd/csrc/ray_eval_math.h (the per-ray arithmetic the kernels of ray_eval.hip
// evaluate per lane) with g++ into a stand-alone program, so that it can be compared with the reference's own numpy
// results (tests/golden/ray_eval_cases.npz) on a machine without a GPU (tests/test_ray_eval_cpu.py), under the host
// sanitizers when the toolchain has them.  The loops around the header restate what the kernels do with it: park the
// short predictions, search with a strict `<` in index order, sum the terms.  Never used by the product.
//
//   ray_eval_host IN OUT
// IN : int32 n_cases, then per case { int32 P, G; float origin[3]; float pred[P][3]; float gt[G][3]; }
// OUT: per case { double clamp_origin[G][3]; double clamp_point[G][3]; int32 invalid[G]; int32 nn[G];
//                 double interp[G][3]; double terms[G][2]; double l1, absrel; int32 count; }
//      clamp_* / invalid: clamp(gt) of every ray; nn: the row of pred, -1 for an uncounted ray; interp: NaN for an
//      uncounted ray; terms: (L1, AbsRel), 0 where the ray contributes nothing; l1 / absrel: their sums over count
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>

#include "ray_eval_math.h"

using namespace vidar_ray_eval;

template <typename T>
static bool put(FILE* f, const std::vector<T>& v) {
  return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 3;
  int32_t n_cases = 0;
  if (fread(&n_cases, sizeof n_cases, 1, in) != 1 || n_cases < 0) return 4;
  for (int32_t c = 0; c < n_cases; ++c) {
    int32_t dims[2];
    float o32[3];
    if (fread(dims, sizeof(int32_t), 2, in) != 2 || dims[0] < 0 || dims[1] < 0 || fread(o32, sizeof(float), 3, in) != 3)
      return 4;
    const size_t P = (size_t)dims[0], G = (size_t)dims[1];
    std::vector<float> pred(P * 3), gt(G * 3);
    if ((P && fread(pred.data(), sizeof(float), P * 3, in) != P * 3) || (G && fread(gt.data(), sizeof(float), G * 3, in) != G * 3))
      return 4;
    const double origin[3] = {o32[0], o32[1], o32[2]};
    std::vector<double> th(P), ph(P), dh(P);
    for (size_t p = 0; p < P; ++p) {
      spherical((double)pred[p * 3] - origin[0], (double)pred[p * 3 + 1] - origin[1], (double)pred[p * 3 + 2] - origin[2],
                &th[p], &ph[p], &dh[p]);
      if (!(dh[p] > kMinDist)) th[p] = INFINITY;          // parked: the strict `<` below never takes it
    }
    std::vector<double> co(G * 3), cp(G * 3), interp(G * 3, NAN), terms(G * 2, 0.0);
    std::vector<int32_t> invalid(G), nn(G, -1);
    double sum_l1 = 0.0, sum_ar = 0.0;
    int32_t count = 0;
    for (size_t g = 0; g < G; ++g) {
      const double pt[3] = {gt[g * 3], gt[g * 3 + 1], gt[g * 3 + 2]};
      double q[3] = {pt[0], pt[1], pt[2]};
      invalid[g] = clamp_ray(q, origin, &co[g * 3]);
      for (int a = 0; a < 3; ++a) cp[g * 3 + a] = q[a];
      double theta, phi, d;
      spherical(pt[0] - origin[0], pt[1] - origin[1], pt[2] - origin[2], &theta, &phi, &d);
      if (!(d > kMinDist)) continue;
      ++count;
      double best = INFINITY;
      for (size_t p = 0; p < P; ++p) {
        const double d2 = angular_d2(theta, phi, th[p], ph[p]);
        if (d2 < best) {
          best = d2;
          nn[g] = (int32_t)p;
        }
      }
      if (nn[g] < 0) {                                   // no kept prediction: the reference would raise
        terms[g * 2] = terms[g * 2 + 1] = NAN;
      } else {
        interpolate(pt, origin, dh[(size_t)nn[g]], &interp[g * 3]);
        error_terms(pt, &interp[g * 3], origin, &terms[g * 2], &terms[g * 2 + 1]);
      }
      sum_l1 += terms[g * 2];
      sum_ar += terms[g * 2 + 1];
    }
    const double res[2] = {sum_l1 / count, sum_ar / count};
    if (!put(out, co) || !put(out, cp) || !put(out, invalid) || !put(out, nn) || !put(out, interp) || !put(out, terms) ||
        fwrite(res, sizeof(double), 2, out) != 2 || fwrite(&count, sizeof count, 1, out) != 1)
      return 6;
  }
  fclose(in);
  fclose(out);
  printf("%d cases\n", n_cases);
  return 0;
}
