// Host program for tests/test_deterministic_cpu.py: the arithmetic of vidar_amd/csrc/det_acc.h compiled by g++.
// Prints one "name ok" line per check and exits non-zero at the first failure.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "det_acc.h"

static int fail(const char* what) {
  std::printf("FAILED %s\n", what);
  return 1;
}

static uint32_t bits_of(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

// what a deterministic scatter does for ONE address: measure, quantise and add, finalise
static float det_sum(const std::vector<float>& v, uint64_t n_bound, uint32_t* mbits_out = nullptr, int* h_out = nullptr) {
  uint32_t mbits = 0;
  for (float x : v) mbits = std::max(mbits, det::abs_bits(x));
  const int h = det::headroom_bits(n_bound);
  const det::Quantum q = det::quantum(mbits, h);
  uint64_t acc = 0;                       // the device adds with an unsigned 64-bit atomic: wrap-around two's complement
  for (float x : v) acc += (uint64_t)det::quantise(x, q.inv);
  if (mbits_out) *mbits_out = mbits;
  if (h_out) *h_out = h;
  return det::finalise((int64_t)acc, mbits, q.delta);
}

// `det_acc_host small n v0 v1 ...`: the header's own numbers for one address that receives v0, v1, ... in a call with
// at most n contributions, for the test to compare with exact rationals:
//   "h <h> delta_exp <e> acc <A> out <float bits>"   (delta = 2^e)
static int small(int argc, char** argv) {
  const uint64_t n = std::strtoull(argv[2], nullptr, 10);
  std::vector<float> v;
  for (int i = 3; i < argc; ++i) v.push_back(std::strtof(argv[i], nullptr));
  uint32_t mbits = 0;
  for (float x : v) mbits = std::max(mbits, det::abs_bits(x));
  const int h = det::headroom_bits(n);
  const det::Quantum q = det::quantum(mbits, h);
  int64_t acc = 0;
  for (float x : v) acc += det::quantise(x, q.inv);
  int e = 0;
  std::frexp(q.delta, &e);                                   // delta = 0.5 * 2^e
  std::printf("h %d delta_exp %d acc %lld out %u\n", h, e - 1, (long long)acc, bits_of(det::finalise(acc, mbits, q.delta)));
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 3 && std::string(argv[1]) == "small") return small(argc, argv);
  std::mt19937_64 rng(12345);

  // 1. 10^5 contributions spanning 12 decades: the same bits under 20 random permutations, and within the documented
  //    bound of the exact sum
  {
    const int n = 100000;
    std::vector<float> v(n);
    std::uniform_real_distribution<double> expo(-6.0, 6.0), mant(1.0, 10.0);
    for (int i = 0; i < n; ++i) v[i] = (float)((rng() & 1 ? 1.0 : -1.0) * mant(rng) * std::pow(10.0, expo(rng)));
    uint32_t mbits; int h;
    const float first = det_sum(v, n, &mbits, &h);
    for (int rep = 0; rep < 20; ++rep) {
      std::shuffle(v.begin(), v.end(), rng);
      if (bits_of(det_sum(v, n)) != bits_of(first)) return fail("permutation");
    }
    long double exact = 0.0L;             // ascending magnitudes in a 64-bit mantissa: good to ~1e-7, the bound is ~1e-2
    std::vector<float> sorted(v);
    std::sort(sorted.begin(), sorted.end(), [](float a, float b) { return std::fabs(a) < std::fabs(b); });
    for (float x : sorted) exact += (long double)x;
    float M; memcpy(&M, &mbits, 4);
    const long double bound = (long double)M * std::pow(2.0L, 2 * h - 62) + std::pow(2.0L, -23) * std::fabs(exact);
    const long double tight = (long double)n * det::quantum(mbits, h).delta / 2 + std::pow(2.0L, -23) * std::fabs(exact);
    const long double err = std::fabs((long double)first - exact);
    std::printf("sum %.9g exact %.12Lg err %.3Lg tight bound %.3Lg bound %.3Lg h %d\n", first, exact, err, tight, bound, h);
    if (!(err <= tight) || !(tight <= bound)) return fail("error bound");
    std::printf("permutation ok\nerror bound ok\n");
  }

  // 2. no overflow with n = 2^31 contributions all equal to +M (and to -M): the accumulator of one address is
  //    n * q(M), computed here as the repeated add would leave it
  {
    const uint64_t n = 1ull << 31;
    for (float M : {1.0f, 3.0e38f, 1.0e-38f, 0.75f, 1.9999999f}) {
      for (float sgn : {1.0f, -1.0f}) {
        const uint32_t mbits = det::abs_bits(M);
        const int h = det::headroom_bits(n);
        const det::Quantum q = det::quantum(mbits, h);
        const int64_t one = det::quantise(sgn * M, q.inv);
        if (std::llabs(one) > (1ll << (62 - h))) return fail("quantum magnitude");
        const __int128 total = (__int128)one * (__int128)n;
        if (total > (__int128)1 << 62 || total < -((__int128)1 << 62)) return fail("overflow");
        const float out = det::finalise((int64_t)total, mbits, q.delta);
        const double want = (double)sgn * (double)M * (double)n;
        const float want_f = (float)want;   // may be inf for the largest M: then the finite accumulator says inf too
        if (std::isfinite(want_f) ? std::fabs((double)out - want) > std::ldexp(std::fabs(want), -22) : out != want_f)
          return fail("sum of n equal terms");
      }
    }
    if (det::headroom_bits(0) != 0 || det::headroom_bits(1) != 0 || det::headroom_bits(2) != 1 ||
        det::headroom_bits(3) != 2 || det::headroom_bits((1ull << 31) + 1) != 32)
      return fail("headroom_bits");
    std::printf("overflow ok\n");
  }

  // 3. the contract of the edge cases
  {
    std::vector<float> zeros(100, 0.0f);
    zeros[3] = -0.0f;
    if (bits_of(det_sum(zeros, 100)) != 0) return fail("M == 0");
    for (float bad : {INFINITY, -INFINITY, NAN}) {
      std::vector<float> v = {1.0f, 2.0f, bad, -3.0f};
      if (!std::isnan(det_sum(v, 4))) return fail("non-finite M");
    }
    // a denormal M still has a valid quantum
    std::vector<float> tiny = {1.0e-44f, 2.0e-44f, -1.0e-44f};
    if (det_sum(tiny, 3) != 2.0e-44f) return fail("denormal M");
    std::printf("edge cases ok\n");
  }

  // 4. one value alone comes back exactly: M = |x|, whose 24 significant bits end at 2^(E - 24), a multiple of
  //    delta = 2^(E - 62 + h) for h <= 38
  {
    std::uniform_real_distribution<float> u(-1000.f, 1000.f);
    for (int i = 0; i < 1000; ++i) {
      const float x = u(rng);
      if (det_sum({x}, 1u << 20) != x) return fail("identity");
    }
    std::printf("identity ok\n");
  }
  return 0;
}
