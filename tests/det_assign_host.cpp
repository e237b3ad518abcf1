// TEST INFRASTRUCTURE.  Compiles vidar_amd/csrc/det_assign_math.h (the per-problem body of the assignment kernel of
// det_assign.hip) with g++ into a stand-alone program: the Team's lane loop is a plain `for`, the state arrays are heap
// vectors of exactly the problem's size, so the CPU test-suite (tests/test_det_assign_cpu.py) can compare the solver
// with SciPy on a machine without a GPU, under the host sanitizers when the toolchain has them, and the GPU tests can
// ask the kernel for the same bytes.  Never used by the product.
//
//   det_assign_host IN OUT LANES [transpose]
// IN : int32 NL, B, Q, total_g; int32 gt_start[B + 1]; float cost[NL * Q * total_g] in the layout of
//      vidar_det_match_cost_f32 (sample b's [Q, G_b] block of a layer's row at Q * gt_start[b])
// OUT: int32 matched[NL * B * Q]; int32 status[NL * B]
// LANES: the team width (any value >= 1 gives the same bytes).  transpose = 1: solve Q > G problems on a transposed copy,
// as the kernel does.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "det_assign_math.h"

using namespace vidar_det_assign;

struct HostTeam {
  int n;
  std::vector<double> val;
  std::vector<int> idx;
  std::vector<char> flag;
  explicit HostTeam(int lanes) : n(lanes), val((size_t)lanes), idx((size_t)lanes), flag((size_t)lanes) {}
  int lanes() const { return n; }
  template <class F> void each(F f) { for (int lane = 0; lane < n; ++lane) f(lane); }
  template <class F> void one(F f) { f(); }
  void sync() {}
  void vote(int lane, bool b) { flag[(size_t)lane] = b; }
  bool any() const {
    bool r = false;
    for (int lane = 0; lane < n; ++lane) r = r || flag[(size_t)lane];
    return r;
  }
  void offer(int lane, double v, int j) { val[(size_t)lane] = v; idx[(size_t)lane] = j; }
  void argmin(double* v, int* j) const {
    double bv = val[0];
    int bj = idx[0];
    for (int lane = 1; lane < n; ++lane)
      if (val[(size_t)lane] < bv || (val[(size_t)lane] == bv && idx[(size_t)lane] < bj)) {
        bv = val[(size_t)lane];
        bj = idx[(size_t)lane];
      }
    *v = bv;
    *j = bj;
  }
};

int main(int argc, char** argv) {
  if (argc != 4 && argc != 5) {
    fprintf(stderr, "usage: %s IN OUT LANES [transpose]\n", argv[0]);
    return 2;
  }
  const int lanes = atoi(argv[3]);
  const bool transpose = argc == 5 && atoi(argv[4]) != 0;
  if (lanes < 1) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 3;
  int32_t hdr[4];
  if (fread(hdr, sizeof(int32_t), 4, in) != 4) return 4;
  const int NL = hdr[0], B = hdr[1], Q = hdr[2], total_g = hdr[3];
  if (NL < 0 || B < 0 || Q < 0 || total_g < 0) return 4;
  std::vector<int32_t> start((size_t)B + 1);
  if (fread(start.data(), sizeof(int32_t), start.size(), in) != start.size()) return 4;
  std::vector<float> cost((size_t)NL * Q * total_g);
  if (!cost.empty() && fread(cost.data(), sizeof(float), cost.size(), in) != cost.size()) return 4;
  fclose(in);

  std::vector<int32_t> matched((size_t)NL * B * Q, -7), status((size_t)NL * B, -7);
  HostTeam team(lanes);
  for (int l = 0; l < NL; ++l)
    for (int b = 0; b < B; ++b) {
      const int g0 = start[(size_t)b], G = start[(size_t)b + 1] - g0;
      int32_t* m = matched.data() + ((size_t)l * B + b) * Q;
      if (G < 0 || g0 < 0 || g0 + G > total_g) {
        for (int q = 0; q < Q; ++q) m[q] = -1;
        status[(size_t)l * B + b] = kExtent;
        continue;
      }
      const int N = Q > G ? G : Q, M = Q > G ? Q : G;
      std::vector<double> u((size_t)N), v((size_t)M), shortest((size_t)M);
      std::vector<int32_t> path((size_t)M), col4row((size_t)N), row4col((size_t)M);
      std::vector<uint8_t> closed((size_t)M);
      std::vector<float> t(transpose && Q > G ? (size_t)Q * G : 0);
      State s{u.data(), v.data(), shortest.data(), path.data(), col4row.data(), row4col.data(), closed.data()};
      // a block of its own, exactly Q * G long, so that a read beyond it is seen
      std::vector<float> blk(cost.begin() + ((size_t)l * Q * total_g + (size_t)Q * g0),
                             cost.begin() + ((size_t)l * Q * total_g + (size_t)Q * (g0 + G)));
      status[(size_t)l * B + b] = solve_problem(team, blk.data(), t.empty() ? nullptr : t.data(), Q, G, s, m);
    }
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 5;
  if (!matched.empty() && fwrite(matched.data(), sizeof(int32_t), matched.size(), o) != matched.size()) return 6;
  if (!status.empty() && fwrite(status.data(), sizeof(int32_t), status.size(), o) != status.size()) return 6;
  fclose(o);
  printf("%d problems\n", NL * B);
  return 0;
}
