// TEST INFRASTRUCTURE.  Compiles vidar_amd/csrc/occ_score_math.h (the per-voxel decisions of occ_score.hip and the
// per-ray weight of ray_march.hip's sweep_evidence_body) with g++ into a stand-alone program, so that they can be compared
// with the torch restatement of tests/occ_score_cases.py / tests/sweep_evidence_cases.py on a machine without a GPU
// (tests/test_occ_score_cpu.py), under the host sanitizers when the toolchain has them.  Never used by the product.
//
//   occ_score_host IN OUT
// IN : int32 V, T, B, R, K; float min_pred, min_meas, min_hits, step; float th[T]; float planes[4][V] (hit_p, free_p,
//      hit_m, free_m); float L[R]
// OUT: double table[5 + 3T + 2B] of the V voxels as ONE segment, summed in voxel order;
//      int32 flags[V] (bit 0 pred, 1 meas, 2 both, 3 y, 4 finite); float o_p[V];
//      float a[R][K] (beam_weight); int32 trips[R] (beam_trips)
#include <stdint.h>
#include <stdio.h>
#include <vector>

#include "occ_score_math.h"

using namespace vidar_occ;

template <class T>
static bool read_n(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}
template <class T>
static bool write_n(FILE* f, const std::vector<T>& v) {
  return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 3;
  int32_t dims[5];
  float scal[4];
  if (fread(dims, sizeof dims, 1, in) != 1 || fread(scal, sizeof scal, 1, in) != 1) return 4;
  const int V = dims[0], T = dims[1], B = dims[2], R = dims[3], K = dims[4];
  if (V < 0 || T < 1 || T > kMaxThresholds || B < 0 || B > kMaxBins || R < 0 || K < 0) return 4;
  std::vector<float> th, planes, L;
  if (!read_n(in, th, (size_t)T) || !read_n(in, planes, (size_t)4 * V) || !read_n(in, L, (size_t)R)) return 4;
  fclose(in);

  std::vector<double> table((size_t)columns(T, B), 0.0);
  std::vector<int32_t> flags((size_t)V);
  std::vector<float> o_p((size_t)V);
  for (int i = 0; i < V; ++i) {
    const Voxel x = classify(planes[i], planes[(size_t)V + i], planes[(size_t)2 * V + i], planes[(size_t)3 * V + i],
                             scal[0], scal[1], scal[2]);
    flags[i] = (int)x.pred | (int)x.meas << 1 | (int)x.both << 2 | (int)x.y << 3 | (int)x.finite << 4;
    o_p[i] = x.o_p;
    table[0] += x.pred; table[1] += x.meas; table[2] += x.both; table[3] += x.both && x.y;
    if (!x.both) continue;
    table[4] += brier_term(x.o_p, x.y);
    for (int j = 0; j < T; ++j) {
      const bool yhat = x.o_p >= th[j];
      table[5 + 3 * j] += yhat && x.y;
      table[6 + 3 * j] += yhat && !x.y;
      table[7 + 3 * j] += !yhat && x.y;
    }
    if (B > 0) {
      const int b = bin_of(x.o_p, B);
      table[5 + 3 * T + 2 * b] += 1.0;
      table[6 + 3 * T + 2 * b] += x.y;
    }
  }
  std::vector<float> a((size_t)R * K);
  std::vector<int32_t> trips((size_t)R);
  for (int r = 0; r < R; ++r) {
    trips[r] = beam_trips(L[r], scal[3], K);
    for (int k = 0; k < K; ++k) a[(size_t)r * K + k] = beam_weight(L[r], k, scal[3]);
  }

  FILE* o = fopen(argv[2], "wb");
  if (!o) return 5;
  if (!write_n(o, table) || !write_n(o, flags) || !write_n(o, o_p) || !write_n(o, a) || !write_n(o, trips)) return 6;
  fclose(o);
  printf("%d voxels, %d rays\n", V, R);
  return 0;
}
