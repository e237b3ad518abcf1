// TEST INFRASTRUCTURE.  Compiles vidar_amd/csrc/knn_topk.h (the per-lane top-K list, the scan and the chunk merge of
// the kernels of knn_generic.hip) with g++ into a stand-alone program: lanes and chunks are plain loops, every buffer is
// a heap vector of exactly its size, so the CPU test-suite (tests/test_knn_topk_cpu.py) can compare the lists with the
// reference's knn_cpu.cpp build on a machine without a GPU, under the host sanitizers when the toolchain has them.
// Never used by the product.
//
//   knn_topk_host IN OUT
// IN : int32 N, P1, P2, D, K, chunks; int64 lengths1[N], lengths2[N]; float p1[N * P1 * D], p2[N * P2 * D]
// OUT: int64 idx[N * P1 * K]; float dist[N * P1 * K]
// The outputs start as -7 / NaN, the workspace as a pattern no key has: what the functions do not write shows.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "knn_topk.h"

using namespace vidar_knn;

template <int D, int KB>
static void run(const std::vector<float>& p1, const std::vector<float>& p2, const std::vector<int64_t>& len1,
                const std::vector<int64_t>& len2, int N, int P1, int P2, int K, int chunks, std::vector<int64_t>& idx,
                std::vector<float>& dist) {
  std::vector<uint64_t> lists((size_t)N * P1 * chunks * K, 0x0badbadbadbadbadull);
  for (int n = 0; n < N; ++n) {
    const int l1 = (int)(len1[(size_t)n] < P1 ? len1[(size_t)n] : P1);
    const int l2 = (int)(len2[(size_t)n] < P2 ? (len2[(size_t)n] < 0 ? 0 : len2[(size_t)n]) : P2);
    // the cloud as a block of its own, exactly l2 points long, so that a read beyond lengths2 is seen
    std::vector<float> q(p2.begin() + (size_t)n * P2 * D, p2.begin() + ((size_t)n * P2 + l2) * D);
    for (int c = 0; c < chunks; ++c) {               // the scan launch: one (row, chunk) per lane
      const int j0 = chunk_begin(c, P2, chunks);
      const int j1 = chunk_begin(c + 1, P2, chunks) < l2 ? chunk_begin(c + 1, P2, chunks) : l2;
      if (j0 >= j1) continue;
      for (int row = 0; row < l1; ++row) {
        float a[D];
        for (int d = 0; d < D; ++d) a[d] = p1[((size_t)n * P1 + row) * D + d];
        uint64_t keys[KB];
        list_clear<KB>(keys);
        list_scan<D, KB>(a, q.data() + (size_t)j0 * D, j1 - j0, j0, keys);
        list_store<KB>(keys, K, lists.data() + (((size_t)n * P1 + row) * chunks + c) * K);
      }
    }
    for (int row = 0; row < P1; ++row) {             // the merge launch: one row per lane
      const size_t at = (size_t)n * P1 + row;
      row_finish<KB>(lists.data() + at * chunks * K, chunks, K, P2, l2, row < len1[(size_t)n], idx.data() + at * K,
                     dist.data() + at * K);
    }
  }
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 3;
  int32_t hdr[6];
  if (fread(hdr, sizeof(int32_t), 6, in) != 6) return 4;
  const int N = hdr[0], P1 = hdr[1], P2 = hdr[2], D = hdr[3], K = hdr[4], chunks = hdr[5];
  if (N < 0 || P1 < 0 || P2 < 0 || !in_range(D, K) || chunks < 1 || chunks > (P2 > 0 ? P2 : 1)) return 4;
  std::vector<int64_t> len1((size_t)N), len2((size_t)N);
  std::vector<float> p1((size_t)N * P1 * D), p2((size_t)N * P2 * D);
  if (N && (fread(len1.data(), sizeof(int64_t), len1.size(), in) != len1.size() ||
            fread(len2.data(), sizeof(int64_t), len2.size(), in) != len2.size()))
    return 4;
  if (!p1.empty() && fread(p1.data(), sizeof(float), p1.size(), in) != p1.size()) return 4;
  if (!p2.empty() && fread(p2.data(), sizeof(float), p2.size(), in) != p2.size()) return 4;
  fclose(in);

  std::vector<int64_t> idx((size_t)N * P1 * K, -7);
  std::vector<float> dist((size_t)N * P1 * K, NAN);
  dispatch(D, bucket(K), [&](auto d, auto kb) {
    run<decltype(d)::value, decltype(kb)::value>(p1, p2, len1, len2, N, P1, P2, K, chunks, idx, dist);
  });
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 5;
  if (!idx.empty() && fwrite(idx.data(), sizeof(int64_t), idx.size(), o) != idx.size()) return 6;
  if (!dist.empty() && fwrite(dist.data(), sizeof(float), dist.size(), o) != dist.size()) return 6;
  fclose(o);
  printf("%d rows\n", N * P1);
  return 0;
}
