// K nearest neighbours for any (D, K) of the kernel range: the per-lane top-K list, the scan of a range of p2 and the
// merge of a row's chunk lists (knn_cpu.cpp:7-58 as a bounded list instead of a priority queue).
//
// ONE body for the kernels of knn_generic.hip and the host test: tests/knn_topk_host.cpp walks lanes and chunks in plain
// loops over the same functions.  Compile with -ffp-contract=off: every product and every sum of a distance rounds on
// its own, as in the reference's CPU build, so the kernel, the host program and the reference give the same bytes.
//
// Order.  A squared distance is a sum of squares: never negative, so its fp32 bit pattern orders like its value, and
//   key = dist_bits << 32 | index
// is a TOTAL order equal to the lexicographic (dist, index) of the reference's max-heap of (float, int) tuples.  The K
// smallest keys of a row are therefore one well-defined set whatever the order they are met in: the result depends
// neither on the number of chunks nor on the launch geometry.  A list is KB keys ascending, KB the bucket of K (1, 2, 4,
// 8, 16, 32); slots that hold no point yet are kEmpty (all ones), which is larger than every real key because an index
// stays below 2^31.  All list indices are compile-time constants after unrolling: the list lives in registers.
//
// NaN coordinates are outside the contract; they cannot move an index out of [0, P2) (an index is only ever a loop
// counter of the scan) and no loop depends on a value: a NaN distance is just a bit pattern that sorts high.
#pragma once
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define VIDAR_KNN_FN __host__ __device__ __forceinline__
#else
#define VIDAR_KNN_FN inline
#endif

namespace vidar_knn {

constexpr int kMaxD = 8;       // the reference's V2 range (knn.cu:261-264)
constexpr int kMaxK = 32;
constexpr uint64_t kEmpty = ~0ull;

VIDAR_KNN_FN bool in_range(int D, int K) { return D >= 1 && D <= kMaxD && K >= 1 && K <= kMaxK; }

// smallest of 1, 2, 4, 8, 16, 32 that holds K
VIDAR_KNN_FN int bucket(int K) {
  int b = 1;
  while (b < K) b *= 2;
  return b;
}

VIDAR_KNN_FN uint32_t float_bits(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __float_as_uint(x);
#else
  uint32_t u;
  memcpy(&u, &x, sizeof u);
  return u;
#endif
}
VIDAR_KNN_FN float bits_float(uint32_t u) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __uint_as_float(u);
#else
  float x;
  memcpy(&x, &u, sizeof x);
  return x;
#endif
}

VIDAR_KNN_FN uint64_t make_key(float dist, int index) { return ((uint64_t)float_bits(dist) << 32) | (uint32_t)index; }
VIDAR_KNN_FN int key_index(uint64_t key) { return (int)(uint32_t)key; }
VIDAR_KNN_FN float key_dist(uint64_t key) { return bits_float((uint32_t)(key >> 32)); }

// chunk c of `chunks` covers p2 indices [chunk_begin(c), chunk_begin(c + 1)): non-empty for every c when chunks <= P2
VIDAR_KNN_FN int chunk_begin(int c, int P2, int chunks) { return (int)((int64_t)c * P2 / chunks); }

// How many chunks the library takes when the caller leaves it open.  Every chunk starts with an empty list, and a wave
// runs the insertion whenever ANY of its 64 lanes needs it -- for about the first 64 KB points of a range always -- so
// more chunks buy parallelism with list upkeep, and the larger K is the dearer.  Measured on an MI355X
// (profiles/kbench_knn_generic.md, the sweep over `chunks`): the best split has about 32 / KB workgroups of 256 rows
// per CU (16 at most, 1 at least) and no range shorter than 384 points or 16 lists.
VIDAR_KNN_FN int auto_chunks(int N, int P1, int P2, int K, int cus) {
  const int64_t blocks = (int64_t)N * ((P1 + 255) / 256);
  const int KB = bucket(K);
  const int min_len = 16 * KB > 384 ? 16 * KB : 384;
  const int per_cu = 32 / KB > 16 ? 16 : (32 / KB < 1 ? 1 : 32 / KB);
  int64_t s = (per_cu * (int64_t)cus + blocks - 1) / (blocks > 0 ? blocks : 1);
  const int64_t most = (P2 + min_len - 1) / min_len;
  s = s > most ? most : s;
  return (int)(s < 1 ? 1 : s);
}

// dist = 0; for d: diff = a[d] - b[d]; dist += diff * diff   (knn_cpu.cpp:36-40)
template <int D>
VIDAR_KNN_FN float sqdist(const float (&a)[D], const float* b) {
  float dist = 0.f;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const float diff = a[d] - b[d];
    dist += diff * diff;
  }
  return dist;
}

template <int KB>
VIDAR_KNN_FN void list_clear(uint64_t (&keys)[KB]) {
#pragma unroll
  for (int i = 0; i < KB; ++i) keys[i] = kEmpty;
}

// keep the KB smallest of keys + {key}, ascending: one compare-and-shift step per slot, from the top down
template <int KB>
VIDAR_KNN_FN void list_insert(uint64_t (&keys)[KB], uint64_t key) {
#pragma unroll
  for (int i = KB - 1; i > 0; --i) {
    const uint64_t below = keys[i - 1];
    keys[i] = key < below ? below : (key < keys[i] ? key : keys[i]);
  }
  keys[0] = key < keys[0] ? key : keys[0];
}

// `count` points at `q` ([count, D]; their indices are first, first + 1, ..) against the query `a`, into the list
template <int D, int KB>
VIDAR_KNN_FN void list_scan(const float (&a)[D], const float* q, int count, int first, uint64_t (&keys)[KB]) {
#pragma unroll 4
  for (int j = 0; j < count; ++j) {
    const float dist = sqdist<D>(a, q + (size_t)j * D);
    // the index rises, so on equal distance the new key is the larger one: `key < worst` is `dist_bits < worst's`
    if (float_bits(dist) < (uint32_t)(keys[KB - 1] >> 32)) list_insert<KB>(keys, make_key(dist, first + j));
  }
}

// the `chunks` lists of one row (`lists`: [chunks, K] keys, each ascending, kEmpty-padded) into one
template <int KB>
VIDAR_KNN_FN void list_merge(const uint64_t* lists, int chunks, int K, uint64_t (&keys)[KB]) {
  // one flat loop with one list_insert body: with an early exit per list the compiler holds a second copy of the list
  // and knn_merge_kernel<32> no longer fits four waves per SIMD
  for (int e = 0; e < chunks * K; ++e) {
    const uint64_t key = lists[e];
    if (key < keys[KB - 1]) list_insert<KB>(keys, key);
  }
}

// the first K keys of a (row, chunk) list to its place in the workspace
template <int KB>
VIDAR_KNN_FN void list_store(const uint64_t (&keys)[KB], int K, uint64_t* out) {
#pragma unroll
  for (int k = 0; k < KB; ++k)
    if (k < K) out[k] = keys[k];
}

// One row's result from its `chunks` lists (`lists`: [chunks, K]).  l2 = the cloud's valid points, 0 .. P2; live = the
// row is below lengths1.  The scan writes only the chunks that begin below l2, so only those are read.  All K slots of
// idx / dist are written: zero for a row that is not live and beyond min(K, l2), like the reference's
// torch::full(.., 0) (knn_cpu.cpp:18-19).
template <int KB>
VIDAR_KNN_FN void row_finish(const uint64_t* lists, int chunks, int K, int P2, int l2, bool live, int64_t* idx,
                             float* dist) {
  uint64_t keys[KB];
  list_clear<KB>(keys);
  if (live && l2 > 0) {
    int written = 0;
    while (written < chunks && chunk_begin(written, P2, chunks) < l2) ++written;
    list_merge<KB>(lists, written, K, keys);
  }
#pragma unroll
  for (int k = 0; k < KB; ++k)
    if (k < K) {
      const bool filled = live && k < l2 && keys[k] != kEmpty;
      idx[k] = filled ? (int64_t)key_index(keys[k]) : 0;
      dist[k] = filled ? key_dist(keys[k]) : 0.f;
    }
}

// f(D, KB as integral constants) for the run-time (D, KB) of the kernel range
template <int V> struct Int { static constexpr int value = V; };
template <int D, class F>
inline void dispatch_k(int KB, F&& f) {
  switch (KB) {
    case 1: f(Int<D>{}, Int<1>{}); break;
    case 2: f(Int<D>{}, Int<2>{}); break;
    case 4: f(Int<D>{}, Int<4>{}); break;
    case 8: f(Int<D>{}, Int<8>{}); break;
    case 16: f(Int<D>{}, Int<16>{}); break;
    default: f(Int<D>{}, Int<32>{}); break;
  }
}
template <class F>
inline void dispatch(int D, int KB, F&& f) {
  switch (D) {
    case 1: dispatch_k<1>(KB, f); break;
    case 2: dispatch_k<2>(KB, f); break;
    case 3: dispatch_k<3>(KB, f); break;
    case 4: dispatch_k<4>(KB, f); break;
    case 5: dispatch_k<5>(KB, f); break;
    case 6: dispatch_k<6>(KB, f); break;
    case 7: dispatch_k<7>(KB, f); break;
    default: dispatch_k<8>(KB, f); break;
  }
}

}  // namespace vidar_knn
