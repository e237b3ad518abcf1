// Private copies for the scatter backwards (ray_march.hip, dvr_family.hip, latent_render.hip).
//
// Every ray of a frame starts at the sensor origin (latent render: at the BEV centre), so the first waypoints of all
// rays scatter onto the same few voxels and the fp32 atomics on those addresses serialise.  The backward kernels
// therefore add into kCopies private copies of the gradient volume (workgroup i -> copy i mod kCopies; neighbouring
// workgroups are neighbouring rays) kept in the CALLER's workspace, and sum_copies_kernel adds the copies up in a fixed
// order: kCopies times fewer atomics per hot address for the same total number.  Without a usable workspace the
// kernels add straight into the outputs.  Measured on MI355X, memset and sum included
// (profiles/r04_staged_variants_kernel_times.log): ray_ce_bwd 0.69 -> 0.41 ms, ray_gumbel_bwd 0.41 -> 0.29 ms,
// lr_prob_bwd 0.66 -> 0.48 ms, lr_gather_bwd 1.32 -> 1.08 ms.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vidar_common.h"

namespace {   // internal linkage: every translation unit that scatters carries its own sum_copies_kernel

constexpr int kScatterCopies = 8;

// workspace for `volumes` gradient volumes of n floats each
inline size_t scatter_workspace_bytes(size_t n, int volumes) { return sizeof(float) * n * kScatterCopies * volumes; }

// the private copy this workgroup adds into (ncopies == 1: the output itself)
__device__ __forceinline__ size_t scatter_copy_of_block(int ncopies) { return blockIdx.x % ncopies; }

__device__ __forceinline__ void scatter_acc(float& a, float v) { a += v; }
__device__ __forceinline__ void scatter_acc(float4& a, const float4& v) { a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; }

// out = copy 0 + copy 1 + ... + copy 7, n elements of T per copy
template <class T>
__global__ __launch_bounds__(256) void sum_copies_kernel(const T* __restrict__ copies, T* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  T a = copies[i];
  for (int c = 1; c < kScatterCopies; ++c) scatter_acc(a, copies[(size_t)c * n + i]);
  out[i] = a;
}

// The host side of a scatter backward with one gradient output (out1 == nullptr) of n0 floats or two, of n0 and n1
// floats; T is the element type of the copy sum (n0 and n1 are multiples of its width).
//   * copies are used iff the workspace is non-NULL, holds 8 copies of every output and -- only where T is wider than
//     float -- workspace and outputs are aligned to T;
//   * the accumulators (the copies, else the outputs) are zeroed;
//   * `launch(acc0, acc1, ncopies)` enqueues the scatter kernel: copy c of volume v starts at acc_v + c * n_v;
//   * the copies are summed into the outputs.  An `empty` launch (no rays) skips the kernel and leaves zeroed outputs.
template <class T = float, class Launch>
int scatter_with_copies(float* out0, float* out1, size_t n0, size_t n1, bool empty, void* workspace,
                        size_t workspace_bytes, hipStream_t s, Launch launch) {
  if (!out1) n1 = 0;
  const size_t need = scatter_workspace_bytes(n0 + n1, 1);
  const bool aligned =
      sizeof(T) == sizeof(float) || (((uintptr_t)workspace | (uintptr_t)out0 | (uintptr_t)out1) % sizeof(T)) == 0;
  const bool copies = workspace != nullptr && workspace_bytes >= need && aligned;
  float* acc0 = copies ? (float*)workspace : out0;
  float* acc1 = !out1 ? nullptr : copies ? (float*)workspace + n0 * kScatterCopies : out1;
  const auto zero_outputs = [&] {
    hipError_t e = hipMemsetAsync(out0, 0, sizeof(float) * n0, s);
    if (e == hipSuccess && out1) e = hipMemsetAsync(out1, 0, sizeof(float) * n1, s);
    return e;
  };
  const hipError_t e = copies ? hipMemsetAsync(workspace, 0, need, s) : zero_outputs();
  if (e != hipSuccess) return (int)e;
  if (empty) return copies ? (int)zero_outputs() : 0;
  launch(acc0, acc1, copies ? kScatterCopies : 1);
  if (copies) {
    const auto sum = [&](const float* acc, float* out, size_t n) {
      const size_t nt = n * sizeof(float) / sizeof(T);
      hipLaunchKernelGGL(sum_copies_kernel<T>, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, s, (const T*)acc, (T*)out,
                         nt);
    };
    sum(acc0, out0, n0);
    if (out1) sum(acc1, out1, n1);
  }
  return vidar_last_error();
}
// ... of n floats each
template <class T = float, class Launch>
int scatter_with_copies(float* out0, float* out1, size_t n, bool empty, void* workspace, size_t workspace_bytes,
                        hipStream_t s, Launch launch) {
  return scatter_with_copies<T>(out0, out1, n, n, empty, workspace, workspace_bytes, s, launch);
}

}  // namespace
