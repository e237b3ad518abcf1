// Host shell of a scatter backward in the deterministic mode (det_acc.h has the arithmetic, DESIGN 4f the policy).
//
// The caller's workspace holds one int64 accumulator per output element and, behind them, the max word of every
// output: det_workspace_bytes.  det_scatter zeroes it, enqueues the body's measure form and then its fixed-point form,
// and finalises into the float outputs; nothing is allocated and the host never waits for the device (the fixed-point
// kernels read the max word the measure kernel left in the workspace).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "det_acc.h"
#include "scatter_copies.h"
#include "vidar_hip.h"
#include "vidar_common.h"

namespace {   // internal linkage, like scatter_copies.h

inline bool det_mode() { return vidar_get_deterministic() != 0; }

// workspace for outputs of n floats in all: 8 B per element + one 8-byte slot per output for its max word
inline size_t det_workspace_bytes(size_t n, int outputs = 1) { return 8 * (n + (size_t)outputs); }

__global__ __launch_bounds__(256) void det_finalise_kernel(const long long* __restrict__ acc,
                                                           const uint32_t* __restrict__ word, float* __restrict__ out,
                                                           size_t n, int h) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t mbits = *word;
  out[i] = det::finalise(acc[i], mbits, det::quantum(mbits, h).delta);
}

// One gradient output (out1 == nullptr) of n0 floats or two, of n0 and n1 floats; `contributions` bounds the number of
// adds of the whole call.  `launch(tag, p0, p1)` enqueues the body's kernel for the policy `decltype(tag)` (first
// det::AccMeasure, then det::AccFixed) with p_v the policy's Param of output v: one generic lambda that launches
// kernel<decltype(tag)>, on the same grid and with the same arguments in both passes.  An `empty` call only zeroes the
// outputs.
// VIDAR_ERR_BAD_ARG without a workspace of det_workspace_bytes: the mode never falls back to float atomics.
template <class Launch>
int det_scatter(float* out0, float* out1, size_t n0, size_t n1, uint64_t contributions, bool empty, void* workspace,
                size_t workspace_bytes, hipStream_t s, Launch launch) {
  if (!out1) n1 = 0;
  if (empty || n0 + n1 == 0) {          // nothing to add: zeros, and no workspace is needed
    hipError_t e = n0 ? hipMemsetAsync(out0, 0, sizeof(float) * n0, s) : hipSuccess;
    if (e == hipSuccess && n1) e = hipMemsetAsync(out1, 0, sizeof(float) * n1, s);
    return (int)e;
  }
  const int outputs = out1 ? 2 : 1;
  const size_t need = det_workspace_bytes(n0 + n1, outputs);
  if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 7)) return VIDAR_ERR_BAD_ARG;
  const int h = det::headroom_bits(contributions);
  long long* acc0 = (long long*)workspace;
  long long* acc1 = out1 ? acc0 + n0 : nullptr;
  uint32_t* word0 = (uint32_t*)(acc0 + n0 + n1);
  uint32_t* word1 = out1 ? word0 + 2 : nullptr;
  const hipError_t e = hipMemsetAsync(workspace, 0, need, s);
  if (e != hipSuccess) return (int)e;
  launch(det::AccMeasure{}, det::AccMeasure::Param{word0}, det::AccMeasure::Param{word1});
  launch(det::AccFixed{}, det::AccFixed::Param{acc0, word0, h}, det::AccFixed::Param{acc1, word1, h});
  if (n0)
    hipLaunchKernelGGL(det_finalise_kernel, dim3((unsigned)((n0 + 255) / 256)), dim3(256), 0, s, acc0, word0, out0, n0, h);
  if (n1)
    hipLaunchKernelGGL(det_finalise_kernel, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, s, acc1, word1, out1, n1, h);
  return vidar_last_error();
}

// The host side of a backward whose default mode scatters into private copies (scatter_copies.h): the one place where
// such an entry forks on the mode.  `default_launch(acc0, acc1, ncopies)` is scatter_with_copies' callable (T: the element
// type of its copy sum), `det_launch(tag, p0, p1)` det_scatter's.
template <class T = float, class DefaultLaunch, class DetLaunch>
int scatter_backward(float* out0, float* out1, size_t n0, size_t n1, uint64_t contributions, bool empty, void* workspace,
                     size_t workspace_bytes, hipStream_t s, DefaultLaunch default_launch, DetLaunch det_launch) {
  if (det_mode())
    return det_scatter(out0, out1, n0, n1, contributions, empty, workspace, workspace_bytes, s, det_launch);
  return scatter_with_copies<T>(out0, out1, n0, n1, empty, workspace, workspace_bytes, s, default_launch);
}
// ... and its workspace, for `outputs` gradient outputs of n floats in all
inline size_t scatter_backward_workspace_bytes(size_t n, int outputs) {
  return det_mode() ? det_workspace_bytes(n, outputs) : scatter_workspace_bytes(n, 1);
}

}  // namespace
