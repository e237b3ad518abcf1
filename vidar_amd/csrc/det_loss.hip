// Detection loss tail of the BEVFormer fine-tune step (bevformer/dense_heads/bevformer_head.py:215-393,
// core/bbox/assigners/hungarian_assigner_3d.py:106-123, core/bbox/match_costs/match_cost.py), for ALL decoder layers
// and ALL samples of a step at once:
//   * det_match_cost_kernel: the Hungarian cost matrices (focal classification cost + L1 over the first 8 box code
//     dims), one launch; the host then makes ONE device->host copy and solves the NL*B assignment problems;
//   * det_loss_fwd_kernel / det_loss_sum_kernel: sigmoid focal loss against the assigned labels and the
//     code-weighted L1 of the matched queries, reduced to [NL, 2] sums;
//   * det_loss_bwd_kernel: d cls / d box written in full, no targets tensor.
// The reference runs this as ~6 x batch x (sigmoid, two logs, two pows, gather, cdist, add, .cpu()) and then
// 6 x (scatter targets, focal loss, normalize_bbox, isfinite, masked L1): several hundred launches of a few KB and
// 6*B + 12 host syncs.  Nothing here is bandwidth: at NL 6, B 1, Q 900, C 10 the operands are 0.43 MB and the largest
// cost matrix (G 150) 3.2 MB.  These kernels are LATENCY-bound (a few hundred workgroups, one short dependent chain
// each); what they buy is the launch count and, first of all, the host-sync count.
//
// Kernel notes (gfx950, wave64):
//   * workgroup = 256 threads = 4 waves, one workgroup per (layer, tile of consecutive (sample, query) rows); every
//     global access is one dword per lane at consecutive addresses, so a wave touches 256 contiguous bytes.  The box
//     rows are 10 floats = 40 B, only 8-byte aligned: a 16-byte load per lane would straddle rows and be misaligned for
//     three rows out of four, and a dwordx2 mapping gains nothing over the dword-per-lane mapping, which is already
//     fully coalesced -- so no vector loads here, on purpose.
//   * reductions are deterministic: lane values -> fixed shuffle tree per wave -> the 4 wave sums added in wave order
//     -> one partial per workgroup in the caller's workspace -> det_loss_sum_kernel adds the partials of a layer in
//     tile order (one wave, strided, then the same tree).  No floating-point atomics anywhere: same inputs, same bits.
//     The terms are fp32; they are ADDED in fp64 (54 000 terms per layer: an fp32 running sum would carry more rounding
//     than the terms themselves; the fp64 adds are free in a latency-bound kernel) and the total is rounded to fp32 once.
//   * compiled with -ffp-contract=off like the rest of the library: the operation order below is what is evaluated.
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include "vidar_hip.h"
#include "vidar_common.h"

namespace {

constexpr int kCode = 10;        // box code size (cx, cy, log w, log l, cz, log h, sin, cos, vx, vy)
constexpr int kCostDims = 8;     // the assigner's L1 cost leaves the velocity out (hungarian_assigner_3d.py:113)
constexpr int kMaxC = 64;        // classes staged per query in LDS
constexpr int kCostTQ = 16;      // queries per workgroup of the cost kernel
constexpr int kLossTR = 64;      // (sample, query) rows per workgroup of the loss kernels
constexpr int kThreads = 256;

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float powg(float x, float gamma) { return gamma == 2.0f ? x * x : powf(x, gamma); }

// sample of the flattened row r = b * Q + q is r / Q; gt_start[b] .. gt_start[b + 1] are its ground-truth rows
__global__ __launch_bounds__(kThreads) void det_match_cost_kernel(
    const float* __restrict__ cls, const float* __restrict__ box, const float* __restrict__ gt_box,
    const int32_t* __restrict__ gt_label, const int32_t* __restrict__ gt_start, float* __restrict__ cost, float alpha,
    float gamma, float cls_w, float reg_w, int B, int Q, int C, int total_g) {
  __shared__ float s_cls[kCostTQ][kMaxC];
  __shared__ float s_box[kCostTQ][kCostDims];
  const int tiles = (Q + kCostTQ - 1) / kCostTQ;
  const int tile = blockIdx.x % tiles, b = blockIdx.x / tiles, l = blockIdx.y;
  const int g0 = gt_start[b], G = gt_start[b + 1] - g0;
  if (G <= 0 || g0 < 0 || g0 + G > total_g) return;          // uniform per workgroup
  const int q0 = tile * kCostTQ;
  const int nq = min(kCostTQ, Q - q0);
  const int64_t row0 = ((int64_t)l * B + b) * Q + q0;
  for (int e = threadIdx.x; e < nq * C; e += kThreads) {
    const float p = sigmoidf_(cls[row0 * C + e]);
    const float pos = -alpha * powg(1.0f - p, gamma) * logf(p + 1e-12f);
    const float neg = -(1.0f - alpha) * powg(p, gamma) * logf(1.0f - p + 1e-12f);
    s_cls[e / C][e % C] = (pos - neg) * cls_w;
  }
  for (int e = threadIdx.x; e < nq * kCostDims; e += kThreads)
    s_box[e / kCostDims][e % kCostDims] = box[(row0 + e / kCostDims) * kCode + e % kCostDims];
  __syncthreads();
  // [Q, G] row-major block of sample b inside layer l's row of the output
  float* out = cost + (int64_t)l * Q * total_g + (int64_t)Q * g0 + (int64_t)q0 * G;
  for (int e = threadIdx.x; e < nq * G; e += kThreads) {
    const int ql = e / G, g = e - ql * G;
    const float* t = gt_box + (int64_t)(g0 + g) * kCode;
    float reg = 0.0f;
#pragma unroll
    for (int k = 0; k < kCostDims; ++k) reg += fabsf(s_box[ql][k] - t[k]);
    int c = gt_label[g0 + g];
    c = c < 0 ? 0 : (c >= C ? C - 1 : c);                     // never index outside, whatever the labels hold (the head checks host labels)
    out[e] = s_cls[ql][c] + reg * reg_w;
  }
}

// fixed-order sum over the workgroup; valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* s_wave) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) s_wave[wave] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < kThreads / 64; ++w) t += s_wave[w];
  __syncthreads();
  return t;
}

// per row of the tile: offset of the matched ground-truth row (in floats) or -1 when the query is unmatched or its
// target has a non-finite entry (bevformer_head.py:383)
__device__ __forceinline__ void stage_targets(int* s_tgt, const int32_t* __restrict__ matched,
                                              const float* __restrict__ gt_box, const int32_t* __restrict__ gt_start,
                                              int64_t row0, int r0, int nr, int Q, int total_g) {
  if ((int)threadIdx.x < nr) {
    const int b = (r0 + threadIdx.x) / Q;
    const int g0 = gt_start[b], G = gt_start[b + 1] - g0;
    const int m = matched[row0 + threadIdx.x];
    int off = -1;
    if (m >= 0 && m < G && g0 >= 0 && g0 + G <= total_g) {
      off = (g0 + m) * kCode;
      bool finite = true;
      for (int k = 0; k < kCode; ++k) finite = finite && isfinite(gt_box[off + k]);
      if (!finite) off = -1;
    }
    s_tgt[threadIdx.x] = off;
  }
  __syncthreads();
}

__global__ __launch_bounds__(kThreads) void det_loss_fwd_kernel(
    const float* __restrict__ cls, const float* __restrict__ box, const int32_t* __restrict__ labels,
    const int32_t* __restrict__ matched, const float* __restrict__ gt_box, const int32_t* __restrict__ gt_start,
    const float* __restrict__ code_w, double* __restrict__ partial, float alpha, float gamma, int R, int Q, int C,
    int total_g) {
  __shared__ int s_tgt[kLossTR];
  __shared__ int s_lab[kLossTR];
  __shared__ double s_wave[kThreads / 64];
  const int tile = blockIdx.x, l = blockIdx.y;
  const int r0 = tile * kLossTR;
  const int nr = min(kLossTR, R - r0);
  const int64_t row0 = (int64_t)l * R + r0;
  if ((int)threadIdx.x < nr) s_lab[threadIdx.x] = labels[row0 + threadIdx.x];
  stage_targets(s_tgt, matched, gt_box, gt_start, row0, r0, nr, Q, total_g);
  double a_cls = 0.0, a_box = 0.0;
  for (int e = threadIdx.x; e < nr * C; e += kThreads) {
    const int rl = e / C, c = e - rl * C;
    const float p = sigmoidf_(cls[row0 * C + e]);
    a_cls += (s_lab[rl] == c) ? -alpha * powg(1.0f - p, gamma) * logf(fmaxf(p, FLT_MIN))
                              : -(1.0f - alpha) * powg(p, gamma) * logf(fmaxf(1.0f - p, FLT_MIN));
  }
  for (int e = threadIdx.x; e < nr * kCode; e += kThreads) {
    const int rl = e / kCode, k = e - rl * kCode;
    const int off = s_tgt[rl];
    if (off >= 0) a_box += code_w[k] * fabsf(box[row0 * kCode + e] - gt_box[off + k]);
  }
  const double t_cls = block_sum(a_cls, s_wave);
  const double t_box = block_sum(a_box, s_wave);
  if (threadIdx.x == 0) {
    double* o = partial + ((int64_t)l * gridDim.x + tile) * 2;
    o[0] = t_cls;
    o[1] = t_box;
  }
}

// one wave per layer: partial[l, 0 .. tiles) -> sums[l, 2]
__global__ __launch_bounds__(64) void det_loss_sum_kernel(const double* __restrict__ partial, float* __restrict__ sums,
                                                          int tiles) {
  const int l = blockIdx.x;
  double a = 0.0, b = 0.0;
  for (int t = threadIdx.x; t < tiles; t += 64) {
    a += partial[((int64_t)l * tiles + t) * 2];
    b += partial[((int64_t)l * tiles + t) * 2 + 1];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_down(a, off, 64);
    b += __shfl_down(b, off, 64);
  }
  if (threadIdx.x == 0) {
    sums[l * 2] = (float)a;
    sums[l * 2 + 1] = (float)b;
  }
}

__global__ __launch_bounds__(kThreads) void det_loss_bwd_kernel(
    const float* __restrict__ cls, const float* __restrict__ box, const int32_t* __restrict__ labels,
    const int32_t* __restrict__ matched, const float* __restrict__ gt_box, const int32_t* __restrict__ gt_start,
    const float* __restrict__ code_w, const float* __restrict__ d_sums, float* __restrict__ d_cls,
    float* __restrict__ d_box, float alpha, float gamma, int R, int Q, int C, int total_g) {
  __shared__ int s_tgt[kLossTR];
  __shared__ int s_lab[kLossTR];
  const int tile = blockIdx.x, l = blockIdx.y;
  const int r0 = tile * kLossTR;
  const int nr = min(kLossTR, R - r0);
  const int64_t row0 = (int64_t)l * R + r0;
  if ((int)threadIdx.x < nr) s_lab[threadIdx.x] = labels[row0 + threadIdx.x];
  stage_targets(s_tgt, matched, gt_box, gt_start, row0, r0, nr, Q, total_g);
  const float dc = d_sums[l * 2], db = d_sums[l * 2 + 1];
  for (int e = threadIdx.x; e < nr * C; e += kThreads) {
    const int rl = e / C, c = e - rl * C;
    const float p = sigmoidf_(cls[row0 * C + e]);
    float g;
    if (s_lab[rl] == c)          // d/dx of -alpha (1-p)^gamma log p
      g = -alpha * powg(1.0f - p, gamma) * (1.0f - p - gamma * p * logf(fmaxf(p, FLT_MIN)));
    else                         // d/dx of -(1-alpha) p^gamma log(1-p)
      g = -(1.0f - alpha) * powg(p, gamma) * (gamma * (1.0f - p) * logf(fmaxf(1.0f - p, FLT_MIN)) - p);
    d_cls[row0 * C + e] = g * dc;
  }
  for (int e = threadIdx.x; e < nr * kCode; e += kThreads) {
    const int rl = e / kCode, k = e - rl * kCode;
    const int off = s_tgt[rl];
    float g = 0.0f;
    if (off >= 0) {
      const float d = box[row0 * kCode + e] - gt_box[off + k];
      g = code_w[k] * (d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f)) * db;
    }
    d_box[row0 * kCode + e] = g;
  }
}

bool bad_dims(int NL, int B, int Q, int C, int total_g) {
  return NL < 0 || B < 0 || Q < 0 || C <= 0 || C > kMaxC || total_g < 0 || (int64_t)B * Q > INT32_MAX / 16 ||
         (int64_t)total_g * kCode > INT32_MAX || NL > 65535;
}

}  // namespace

extern "C" {

int vidar_det_match_cost_f32(const float* cls, const float* box, const float* gt_box_norm, const int32_t* gt_label,
                             const int32_t* gt_start, float* cost, float alpha, float gamma, float cls_weight,
                             float reg_weight, int NL, int B, int Q, int C, int total_g, void* stream) {
  VIDAR_ENTER();
  if (bad_dims(NL, B, Q, C, total_g)) return VIDAR_ERR_BAD_ARG;
  if (NL == 0 || B == 0 || Q == 0 || total_g == 0) return 0;            // nothing to match: no launch on an empty grid
  if (!cls || !box || !gt_box_norm || !gt_label || !gt_start || !cost) return VIDAR_ERR_BAD_ARG;
  const int tiles = (Q + kCostTQ - 1) / kCostTQ;
  hipLaunchKernelGGL(det_match_cost_kernel, dim3((unsigned)(tiles * B), (unsigned)NL), dim3(kThreads), 0,
                     (hipStream_t)stream, cls, box, gt_box_norm, gt_label, gt_start, cost, alpha, gamma, cls_weight,
                     reg_weight, B, Q, C, total_g);
  return vidar_last_error();
}

size_t vidar_det_loss_workspace_bytes(int NL, int B, int Q) {
  if (NL <= 0 || B <= 0 || Q <= 0) return 0;
  const int64_t tiles = ((int64_t)B * Q + kLossTR - 1) / kLossTR;
  return (size_t)(NL * tiles * 2 * sizeof(double));
}

int vidar_det_loss_fwd_f32(const float* cls, const float* box, const int32_t* labels, const int32_t* matched_gt,
                           const float* gt_box_norm, const int32_t* gt_start, const float* code_weights, float* sums,
                           float alpha, float gamma, int NL, int B, int Q, int C, int total_g, void* workspace,
                           size_t workspace_bytes, void* stream) {
  VIDAR_ENTER();
  if (bad_dims(NL, B, Q, C, total_g)) return VIDAR_ERR_BAD_ARG;
  if (NL == 0) return 0;
  if (!sums) return VIDAR_ERR_BAD_ARG;
  if (B == 0 || Q == 0) {
    return (int)hipMemsetAsync(sums, 0, (size_t)NL * 2 * sizeof(float), (hipStream_t)stream);
  }
  if (!cls || !box || !labels || !matched_gt || !gt_start || !code_weights || (total_g > 0 && !gt_box_norm) ||
      !workspace || ((uintptr_t)workspace & 7) || workspace_bytes < vidar_det_loss_workspace_bytes(NL, B, Q))
    return VIDAR_ERR_BAD_ARG;
  const int R = B * Q, tiles = (R + kLossTR - 1) / kLossTR;
  hipLaunchKernelGGL(det_loss_fwd_kernel, dim3((unsigned)tiles, (unsigned)NL), dim3(kThreads), 0, (hipStream_t)stream,
                     cls, box, labels, matched_gt, gt_box_norm, gt_start, code_weights, (double*)workspace, alpha, gamma,
                     R, Q, C, total_g);
  hipLaunchKernelGGL(det_loss_sum_kernel, dim3((unsigned)NL), dim3(64), 0, (hipStream_t)stream,
                     (const double*)workspace, sums, tiles);
  return vidar_last_error();
}

int vidar_det_loss_bwd_f32(const float* cls, const float* box, const int32_t* labels, const int32_t* matched_gt,
                           const float* gt_box_norm, const int32_t* gt_start, const float* code_weights,
                           const float* grad_sums, float* grad_cls, float* grad_box, float alpha, float gamma, int NL,
                           int B, int Q, int C, int total_g, void* stream) {
  VIDAR_ENTER();
  if (bad_dims(NL, B, Q, C, total_g)) return VIDAR_ERR_BAD_ARG;
  if (NL == 0 || B == 0 || Q == 0) return 0;
  if (!cls || !box || !labels || !matched_gt || !gt_start || !code_weights || (total_g > 0 && !gt_box_norm) ||
      !grad_sums || !grad_cls || !grad_box)
    return VIDAR_ERR_BAD_ARG;
  const int R = B * Q, tiles = (R + kLossTR - 1) / kLossTR;
  hipLaunchKernelGGL(det_loss_bwd_kernel, dim3((unsigned)tiles, (unsigned)NL), dim3(kThreads), 0, (hipStream_t)stream,
                     cls, box, labels, matched_gt, gt_box_norm, gt_start, code_weights, grad_sums, grad_cls, grad_box,
                     alpha, gamma, R, Q, C, total_g);
  return vidar_last_error();
}

}  // extern "C"
