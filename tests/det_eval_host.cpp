// TEST INFRASTRUCTURE.  Compiles vidar_amd/csrc/det_eval_math.h (the five true-positive errors the matcher kernel of
// det_eval.hip evaluates per lane) with g++ into a stand-alone program, so that the formulas can be compared with the
// fp64 restatement of tests/det_eval_cases.py on a machine without a GPU (tests/test_det_eval_cpu.py), under the host
// sanitizers when the toolchain has them.  Never used by the product.
//
//   det_eval_host IN OUT
// IN : int32 n, then n records of { float gt[9]; float pred[9]; int32 gt_attr, pred_attr, half_period; }
// OUT: n records of float err[5] (trans_err, vel_err, scale_err, orient_err, attr_err)
#include <stdint.h>
#include <stdio.h>
#include <vector>

#include "det_eval_math.h"

using namespace vidar_det_eval;

struct Record {
  float gt[kBox];
  float pred[kBox];
  int32_t gt_attr, pred_attr, half_period;
};

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 3;
  int32_t n = 0;
  if (fread(&n, sizeof n, 1, in) != 1 || n < 0) return 4;
  std::vector<Record> rec((size_t)n);
  if (n > 0 && fread(rec.data(), sizeof(Record), (size_t)n, in) != (size_t)n) return 4;
  fclose(in);
  std::vector<float> out((size_t)n * kErr);
  for (int32_t i = 0; i < n; ++i)
    pair_errors(rec[i].gt, rec[i].gt_attr, rec[i].pred, rec[i].pred_attr, rec[i].half_period != 0, out.data() + (size_t)i * kErr);
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 5;
  if (n > 0 && fwrite(out.data(), sizeof(float), out.size(), o) != out.size()) return 6;
  fclose(o);
  printf("%d pairs\n", n);
  return 0;
}
