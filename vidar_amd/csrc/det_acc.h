// Order-independent accumulation for the scatter backwards (the deterministic mode).
//
// fp32 atomic adds round after every add, so a scattered sum depends on the order in which its contributions arrive.
// Integer adds are associative.  In the deterministic mode a scatter kernel therefore runs twice over the same body:
//
//   measure   every contribution v only updates M = max |v| (AccMeasure: the maximum of the bit patterns of |v|, which
//             orders non-negative floats and puts inf and every NaN above all finite values; a maximum is itself
//             independent of order);
//   fixed     every contribution adds q = llrint(v / delta) with a 64-bit integer atomic into an int64 accumulator
//             (AccFixed), and a finalising kernel writes out[i] = (float)((double)acc[i] * delta).
//
// The quantum.  E = exponent_above(M) is an exponent with 2^E >= M (and 2^E <= 2 M for a normal M).  n is a bound on the
// number of contributions of the call that the host knows, h = ceil(log2(max(n, 1))), and
//     delta = 2^(E - (62 - h)).
// v / delta is a scaling by a power of two, exact in double (|exponent| <= 149 + 62 + 63), so the only rounding of a
// contribution is the llrint:  |q - v / delta| <= 1/2  and  |q| <= 2^(62 - h).
// No overflow: |sum q| <= n * 2^(62 - h) <= 2^h * 2^(62 - h) = 2^62 < 2^63.
//
// Error bound.  For an address with N_a contributions and exact sum S_a the accumulator holds an integer A with
//     |A * delta - S_a| <= N_a * delta / 2,
// and the finalising step rounds A * delta (a double product, exact to 2^-53 relative: far below the next term) once to
// fp32.  So
//     |out - S_a| <= N_a * delta / 2  +  2^-24 * |out|         (round to nearest; the tests allow 2^-23 * |S_a|)
// and with N_a <= n <= 2^h, 2^E <= 2 M:   N_a * delta / 2 <= 2^h * 2^(E - 62 + h) / 2 <= M * 2^(2h - 62).
// (For a denormal M, 2^E = 2^-126 may exceed 2 M; the bound then holds with 2^-127 in place of M.)
//
// Edge cases, by contract:
//   M == 0          every contribution is +-0: delta = 0, the output is exact zeros.
//   M not finite    (an inf or NaN contribution) the WHOLE output tensor is NaN.  The fp32-atomic form poisons only the
//                   addresses the non-finite contributions touch; the fixed-point form cannot represent them per
//                   address, and a result that is loudly wrong everywhere is the safer of the two possible answers.
//
// The result is a function of the multiset of contributions alone: not of arrival order, launch geometry, the order of
// the items or the kernel variant that produced them.
//
// This header holds the arithmetic only and compiles for the host too (tests/det_acc_host.cpp); the device policies are
// under __HIPCC__, the host shell of a deterministic scatter is det_scatter.h.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define DET_HD __host__ __device__ __forceinline__
#else
#define DET_HD inline
#endif

namespace det {

DET_HD uint32_t abs_bits(float v) {
#ifdef __HIP_DEVICE_COMPILE__
  return __float_as_uint(v) & 0x7fffffffu;
#else
  uint32_t b; memcpy(&b, &v, 4); return b & 0x7fffffffu;
#endif
}
DET_HD bool finite_bits(uint32_t mbits) { return (mbits >> 23) < 0xffu; }

// ceil(log2(max(n, 1)))
DET_HD int headroom_bits(uint64_t n) {
  int h = 0;
  while (h < 63 && ((uint64_t)1 << h) < n) ++h;
  return h;
}

// E with 2^E >= M for the finite M > 0 whose bit pattern is `mbits`; 2^E <= 2 M for a normal M
DET_HD int exponent_above(uint32_t mbits) {
  const int be = (int)(mbits >> 23);
  return be == 0 ? -126 : be - 126;
}

// 2^e as a double, -1022 <= e <= 1023
DET_HD double pow2(int e) {
  const uint64_t b = (uint64_t)(e + 1023) << 52;
#ifdef __HIP_DEVICE_COMPILE__
  return __longlong_as_double((long long)b);
#else
  double d; memcpy(&d, &b, 8); return d;
#endif
}

// delta and 1 / delta of a call with max word `mbits` and headroom h; both 0 for M == 0 and for a non-finite M (the
// finalising step answers those two cases on its own)
struct Quantum { double delta, inv; };
DET_HD Quantum quantum(uint32_t mbits, int h) {
  if (mbits == 0 || !finite_bits(mbits)) return Quantum{0.0, 0.0};
  const int e = exponent_above(mbits) - (62 - h);
  return Quantum{pow2(e), pow2(-e)};
}

DET_HD int64_t quantise(float v, double inv_delta) { return (int64_t)llrint((double)v * inv_delta); }

DET_HD float finalise(int64_t acc, uint32_t mbits, double delta) {
  if (!finite_bits(mbits)) return NAN;
  return (float)((double)acc * delta);
}

}  // namespace det

#ifdef __HIPCC__
namespace det {

// The accumulate policies of a scatter body: `acc.add(p, v)` stands where the body adds v to the output element *p.
// All three have one shape, so a kernel is written once, as a template over Acc that takes a `typename Acc::Param` per
// gradient output:   Acc acc(out, param);  body(..., acc);  acc.flush();     (out: the float output the body addresses)

// fp32 atomic, the default mode: exactly the instruction the bodies used before they took a policy
struct AccAtomic {
  static constexpr bool kMeasureOnly = false;
  struct Param {};
  __device__ __forceinline__ AccAtomic() {}
  __device__ __forceinline__ explicit AccAtomic(const float*, Param = {}) {}
  __device__ __forceinline__ void add(float* p, float v) const { unsafeAtomicAdd(p, v); }
  __device__ __forceinline__ void flush() const {}
};

// first pass of the deterministic mode: M = max |v| of everything the body would add
struct AccMeasure {
  static constexpr bool kMeasureOnly = true;   // a body may skip its plain stores in this pass
  struct Param { uint32_t* word; };
  uint32_t* word;
  uint32_t m = 0;
  AccMeasure() = default;   // on the host a policy object is only a tag (det_scatter.h)
  __device__ __forceinline__ AccMeasure(const float*, Param p) : word(p.word) {}
  __device__ __forceinline__ void add(float*, float v) { m = max(m, abs_bits(v)); }
  // Per wave, then one atomicMax per workgroup.  THE CONTRACT OF A BODY: flush holds workgroup barriers, so every thread
  // of a workgroup that runs the body calls it, once per accumulator -- a thread that had returned from the kernel would
  // deadlock the others.  A body is therefore an inlined function whose early `return`s leave the body, never the
  // kernel; a kernel that carries its body inline keeps, under this policy, every thread on the way to the flush.
  __device__ __forceinline__ void flush() const {
    __shared__ uint32_t wave_max[16];
    uint32_t v = m;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, s, 64));
    const int tid = threadIdx.x + blockDim.x * (threadIdx.y + blockDim.y * threadIdx.z);
    const int nwaves = (blockDim.x * blockDim.y * blockDim.z + 63) / 64;
    __syncthreads();   // a kernel with two outputs flushes twice through the same LDS words
    if (tid % 64 == 0) wave_max[tid / 64] = v;
    __syncthreads();
    if (tid == 0) {
#pragma unroll 1
      for (int w = 1; w < nwaves; ++w) v = max(v, wave_max[w]);
      if (v != 0) atomicMax(word, v);
    }
  }
};

// second pass: 64-bit fixed point.  `base` is the float output the body addresses, `acc` its int64 accumulator volume.
struct AccFixed {
  static constexpr bool kMeasureOnly = false;
  struct Param { long long* acc; const uint32_t* word; int h; };
  const float* base;
  unsigned long long* acc;
  double inv_delta;
  AccFixed() = default;
  __device__ __forceinline__ AccFixed(const float* base_, Param p)
      : base(base_), acc((unsigned long long*)p.acc), inv_delta(quantum(*p.word, p.h).inv) {}
  __device__ __forceinline__ void add(float* p, float v) const {
    atomicAdd(acc + (p - base), (unsigned long long)quantise(v, inv_delta));
  }
  __device__ __forceinline__ void flush() const {}
};

}  // namespace det
#endif
