// Fused LatentRendering ray-march for gfx950.
//
// Replaces the PyTorch op chain of
//   projects/mmdet3d_plugin/bevformer/modules/ray_operations/latent_rendering.py:96-150
// (3x F.grid_sample over [bs,16,Q,257] + sigmoid + cumprod + masked normalisation + reductions,
//  ~5 GB of intermediates per call at Q = 200x200) with two gather kernels and their adjoints that
// keep every intermediate in registers:
//   stage 1 (":102-129")  path_prob[b,q,z] = prod_{k<G, |n_k|<|n_q|} (1 - act(occ(n_k)))  * act(occ(n_q))
//   stage 2 (":131-150")  feat[b,q,z]      = sum_k a(n_k) m_k / (sum_k m_k + eps),  m_k = path_prob(n_k) [|n_k| < bound_q]
// where n_k = 2 * rhat_q * (k + 0.5) * step are the G waypoints of the ray from the BEV centre
// through cell q (normalised [-1,1] coordinates), sampled bilinearly with zero padding and
// align_corners=False.  z runs over the Z = pred_height height bins (1 .. 64); stage 2 carries A = Z * J <= 256 LoRA
// channels and weights channel ch with the path probability of bin ch / J (the reference's view(bs, pred_height, -1, ..)).
//
// Layout in HBM: all maps are channel-last [bs, h*w, Z or A] f32 -- exactly what the producing
// nn.Linear emits -- so one bilinear corner of all channels is one contiguous segment (64 bytes at 16 channels).
// Mapping: one wave per BEV cell; forward lane = (waypoint slot, float4 of channels) -- at 16 channels (k mod 16,
// quarter of the 16 bins) -- the ray is walked 64 / (channel lanes) waypoints per iteration and reduced over the
// waypoint slots with xor shuffles.  Rows that are no multiple of 4 floats take one channel per lane.  Cells are
// assigned to workgroups in row-major order, 4 cells per 256-thread workgroup.
// Backward kernels recompute the forward samples and scatter with fp32 hardware atomics, with the
// lane map (waypoint slot, channel) -- at 16 channels (k mod 4, height bin) -- so that one atomic instruction covers a
// corner's contiguous bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include <type_traits>

#include "vidar_hip.h"
#include "vidar_common.h"
#include "scatter_copies.h"
#include "det_scatter.h"

namespace {

constexpr int kMaxZ = 64;    // height bins
constexpr int kMaxA = 256;   // LoRA channels
constexpr int kThreads = 256;
constexpr int kCellsPerBlock = kThreads / 64;

// Every ray starts at the BEV centre, so the first waypoints of all H*W rays scatter onto the same few cells: the
// backward kernels add into private copies of the gradient maps (scatter_copies.h; the kernels were serialised on the
// hot addresses, not bound by the atomic rate).
// which private copy this workgroup adds into, as an offset in units of [Q, channels] maps (0 when the variant is off)
__device__ __forceinline__ size_t copy_of_block(int ncopies) { return scatter_copy_of_block(ncopies) * gridDim.y; }

struct Geo {
  int H, W, G;
  float step;   // grid_step / (min(H,W)//2), rounded to f32 (latent_rendering.py:102-104)
  int act;      // 0 = sigmoid, 1 = exp
  float eps;
};

struct Cell {
  float rnx, rny;   // unit direction (nan_to_num'ed)
  float ncx, ncy;   // the cell itself in [-1,1]
  float len_c;      // |n_cell|
  float bound;      // min(1/|rnx|, 1/|rny|)
};

__device__ __forceinline__ Cell make_cell(int q, const Geo& g) {
  const int i = q / g.W, j = q % g.W;
  const float gx = (j + 0.5f) / g.W, gy = (i + 0.5f) / g.H;
  const float rx = gx - 0.5f, ry = gy - 0.5f;
  const float nrm = sqrtf(rx * rx + ry * ry);
  Cell c;
  c.rnx = rx / nrm; c.rny = ry / nrm;
  if (c.rnx != c.rnx) c.rnx = 0.f;
  if (c.rny != c.rny) c.rny = 0.f;
  c.ncx = gx * 2.f - 1.f; c.ncy = gy * 2.f - 1.f;
  c.len_c = sqrtf(c.ncx * c.ncx + c.ncy * c.ncy);
  c.bound = fminf(1.f / fabsf(c.rnx), 1.f / fabsf(c.rny));
  return c;
}

struct Tap {        // one bilinear footprint
  int o[4];         // cell index of the 4 corners or -1
  float w[4];
};

__device__ __forceinline__ Tap make_tap(float nx, float ny, const Geo& g) {
  const float ix = ((nx + 1.f) * g.W - 1.f) / 2.f;
  const float iy = ((ny + 1.f) * g.H - 1.f) / 2.f;
  const float fx = floorf(ix), fy = floorf(iy);
  const int x0 = (int)fx, y0 = (int)fy, x1 = x0 + 1, y1 = y0 + 1;
  const float ax = ix - fx, ay = iy - fy;
  Tap t;
  t.w[0] = (1.f - ax) * (1.f - ay); t.w[1] = ax * (1.f - ay);
  t.w[2] = (1.f - ax) * ay;         t.w[3] = ax * ay;
  const bool l = x0 >= 0 && x0 < g.W, r = x1 >= 0 && x1 < g.W;
  const bool u = y0 >= 0 && y0 < g.H, d = y1 >= 0 && y1 < g.H;
  t.o[0] = (l && u) ? y0 * g.W + x0 : -1;
  t.o[1] = (r && u) ? y0 * g.W + x1 : -1;
  t.o[2] = (l && d) ? y1 * g.W + x0 : -1;
  t.o[3] = (r && d) ? y1 * g.W + x1 : -1;
  return t;
}

// V channels of one lane: V = 4 is read and written as one float4 (rows of a multiple of 4 floats), V = 1 as a scalar
template <int V>
struct Vec {
  float e[V];
};
template <int V>
__device__ __forceinline__ Vec<V> vec_fill(float x) {
  Vec<V> v;
#pragma unroll
  for (int i = 0; i < V; ++i) v.e[i] = x;
  return v;
}
template <int V>
__device__ __forceinline__ Vec<V> vec_load(const float* __restrict__ p) {
  Vec<V> v;
  if constexpr (V == 4) {
    const float4 f = *reinterpret_cast<const float4*>(p);
    v.e[0] = f.x; v.e[1] = f.y; v.e[2] = f.z; v.e[3] = f.w;
  } else {
    v.e[0] = *p;
  }
  return v;
}
template <int V>
__device__ __forceinline__ void vec_store(float* __restrict__ p, const Vec<V>& v) {
  if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(v.e[0], v.e[1], v.e[2], v.e[3]);
  else *p = v.e[0];
}

// bilinear sample of channels ch .. ch+V-1 of a channel-last map with C channels
template <int V>
__device__ __forceinline__ Vec<V> tap_load(const float* __restrict__ map, const Tap& t, int C, int ch) {
  Vec<V> acc = vec_fill<V>(0.f);
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    if (t.o[c] >= 0) {
      const Vec<V> v = vec_load<V>(map + (size_t)t.o[c] * C + ch);
#pragma unroll
      for (int i = 0; i < V; ++i) acc.e[i] += t.w[c] * v.e[i];
    }
  }
  return acc;
}
// `acc`: the accumulate policy of det_acc.h (fp32 atomic / measure / fixed point) of the map
template <class Acc>
__device__ __forceinline__ void tap_scatter1(float* __restrict__ map, const Tap& t, int C, int ch, float g, Acc& acc) {
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if (t.o[c] >= 0) acc.add(map + (size_t)t.o[c] * C + ch, t.w[c] * g);
}
// stage 2: the path probability that weights LoRA channels ch .. ch+V-1, i.e. of the bins (ch+i) / J
template <int V>
__device__ __forceinline__ Vec<V> tap_load_bins(const float* __restrict__ pm, const Tap& t, int Z, int ch, int J) {
  if (J == 1) return tap_load<V>(pm, t, Z, ch);
  Vec<V> m;
  int prev = -1;
#pragma unroll
  for (int i = 0; i < V; ++i) {
    const int bin = (ch + i) / J;
    m.e[i] = (i > 0 && bin == prev) ? m.e[i > 0 ? i - 1 : 0] : tap_load<1>(pm, t, Z, bin).e[0];
    prev = bin;
  }
  return m;
}

__device__ __forceinline__ float act_f(float x, int act) {
  if (act == 0) return 1.f / (1.f + expf(-x));
  return 1.f - expf(-fmaxf(x, 0.f));
}
// d act / dx expressed with p = act(x)
__device__ __forceinline__ float act_d(float x, float p, int act) {
  if (act == 0) return p * (1.f - p);
  return x > 0.f ? (1.f - p) : 0.f;
}

// Lane map of every kernel: lane = (waypoint slot, channel lane); LPW = lanes per waypoint, 1 / 4 / 16 / 64, that covers
// the channels (or 64 with a loop over channel chunks), the remaining 64 / LPW lane bits walk the ray.
// reduce over the waypoint slots (lane bits log2(LPW) .. 5); every lane ends with the full result
template <int LPW, int V>
__device__ __forceinline__ Vec<V> kprod(Vec<V> v) {
#pragma unroll
  for (int m = LPW; m < 64; m <<= 1) {
#pragma unroll
    for (int i = 0; i < V; ++i) v.e[i] *= __shfl_xor(v.e[i], m, 64);
  }
  return v;
}
template <int LPW, int V>
__device__ __forceinline__ Vec<V> ksum(Vec<V> v) {
#pragma unroll
  for (int m = LPW; m < 64; m <<= 1) {
#pragma unroll
    for (int i = 0; i < V; ++i) v.e[i] += __shfl_xor(v.e[i], m, 64);
  }
  return v;
}
// stage 2 backward: sum over the lanes of this waypoint slot that follow in the same height bin (`ahead` of them, a
// contiguous run), so that the first lane of a bin holds the bin's sum.  Every lane of the slot takes part.
template <int LPW>
__device__ __forceinline__ float group_sum(float v, int ahead) {
#pragma unroll
  for (int d = 1; d < LPW; d <<= 1) {
    const float o = __shfl_down(v, d, 64);
    if (d <= ahead) v += o;
  }
  return v;
}

__device__ __forceinline__ void waypoint(const Cell& c, const Geo& g, int k, float& nx, float& ny,
                                         float& len) {
  const float s = (k + 0.5f) * g.step;
  const float ux = 0.5f + c.rnx * s, uy = 0.5f + c.rny * s;
  nx = ux * 2.f - 1.f; ny = uy * 2.f - 1.f;
  len = sqrtf(nx * nx + ny * ny);
}

// ---------------------------------------------------------------------------------------------
// All four kernel bodies: one wave per BEV cell.  ZC != 0 states the channel counts at compile time (the released 16 / 16
// shape); ZC == 0 takes them from the launch.  Channel lanes past the channel count neither load nor scatter.
// stage 1 forward: occ [bs,Q,Z] -> path_prob [bs,Q,Z]; lane = (waypoint slot, V bins)
// ---------------------------------------------------------------------------------------------
template <int LPW, int V, int ZC>
__device__ __forceinline__ void lr_prob_fwd(const float* __restrict__ occ, float* __restrict__ prob, int Q, int Zr,
                                            const Geo& g) {
  const int Z = ZC ? ZC : Zr;
  const int b = blockIdx.y;
  const int q = blockIdx.x * kCellsPerBlock + threadIdx.x / 64;
  if (q >= Q) return;
  const int lane = threadIdx.x & 63, z = (lane & (LPW - 1)) * V, ks = lane / LPW;
  const bool on = z < Z;
  const float* map = occ + (size_t)b * Q * Z;
  const Cell c = make_cell(q, g);
  Vec<V> pr = vec_fill<V>(1.f);
  for (int k = ks; k < g.G; k += 64 / LPW) {
    float nx, ny, len;
    waypoint(c, g, k, nx, ny, len);
    if (len < c.len_c && on) {
      const Vec<V> x = tap_load<V>(map, make_tap(nx, ny, g), Z, z);
#pragma unroll
      for (int i = 0; i < V; ++i) pr.e[i] *= 1.f - act_f(x.e[i], g.act);
    }
  }
  pr = kprod<LPW>(pr);
  if (ks == 0 && on) {
    const Vec<V> xc = tap_load<V>(map, make_tap(c.ncx, c.ncy, g), Z, z);
    Vec<V> out;
#pragma unroll
    for (int i = 0; i < V; ++i) out.e[i] = pr.e[i] * act_f(xc.e[i], g.act);
    vec_store<V>(prob + ((size_t)b * Q + q) * Z + z, out);
  }
}

// stage 1 backward: grad_prob [bs,Q,Z] -> grad_occ [bs,Q,Z] (pre-zeroed, atomics); lane = (waypoint slot, bin): one
// atomic instruction covers the contiguous bytes of a tap corner (atomics cost per instruction x line, see msda.hip)
// (Acc: the accumulate policy of det_acc.h; the early `return`s of the two backward bodies are held to the contract at its
// AccMeasure::flush.)
template <int LPW, int ZC, class Acc>
__device__ __forceinline__ void lr_prob_bwd(const float* __restrict__ occ, const float* __restrict__ grad_prob,
                                            float* __restrict__ grad_occ, int Q, int Zr, const Geo& g, int ncopies,
                                            Acc& acc) {
  const int Z = ZC ? ZC : Zr;
  const int b = blockIdx.y;
  const int q = blockIdx.x * kCellsPerBlock + threadIdx.x / 64;
  if (q >= Q) return;
  const int lane = threadIdx.x & 63, z = lane & (LPW - 1), ks = lane / LPW;
  const bool on = z < Z;
  const float* map = occ + (size_t)b * Q * Z;
  float* gmap = grad_occ + (copy_of_block(ncopies) + b) * Q * Z;
  const Cell c = make_cell(q, g);
  // pass 1: the transmittance product
  Vec<1> pr = vec_fill<1>(1.f);
  for (int k = ks; k < g.G; k += 64 / LPW) {
    float nx, ny, len;
    waypoint(c, g, k, nx, ny, len);
    if (len < c.len_c && on) pr.e[0] *= 1.f - act_f(tap_load<1>(map, make_tap(nx, ny, g), Z, z).e[0], g.act);
  }
  pr = kprod<LPW>(pr);
  if (!on) return;
  const Tap tc = make_tap(c.ncx, c.ncy, g);
  const float xc = tap_load<1>(map, tc, Z, z).e[0];
  const float pc = act_f(xc, g.act);
  const float go = grad_prob[((size_t)b * Q + q) * Z + z];
  // d/d(1-p_k) of prod * pc  = prod/(1-p_k) * pc ; guarded against (1-p_k) == 0
  const float gp = go * pr.e[0] * pc;
  for (int k = ks; k < g.G; k += 64 / LPW) {
    float nx, ny, len;
    waypoint(c, g, k, nx, ny, len);
    if (len < c.len_c) {
      const Tap t = make_tap(nx, ny, g);
      const float x = tap_load<1>(map, t, Z, z).e[0];
      const float p = act_f(x, g.act);
      const float gs = (1.f - p) > 0.f ? -gp / (1.f - p) * act_d(x, p, g.act) : 0.f;
      tap_scatter1(gmap, t, Z, z, gs, acc);
    }
  }
  if (ks == 0) tap_scatter1(gmap, tc, Z, z, go * pr.e[0] * act_d(xc, pc, g.act), acc);
}

// ---------------------------------------------------------------------------------------------
// stage 2 forward: prob [bs,Q,Z], a [bs,Q,A] -> feat [bs,Q,A], msum [bs,Q,Z] (= sum_k m_k); A = Z * J and LoRA
// channel ch is weighted by bin ch / J.  lane = (waypoint slot, V channels); A > LPW * V is walked in chunks.
// ---------------------------------------------------------------------------------------------
template <int LPW, int V, int ZC>
__device__ __forceinline__ void lr_gather_fwd(const float* __restrict__ prob, const float* __restrict__ a,
                                              float* __restrict__ feat, float* __restrict__ msum, int Q, int Zr, int Ar,
                                              const Geo& g) {
  const int Z = ZC ? ZC : Zr, A = ZC ? ZC : Ar, J = ZC ? 1 : Ar / Zr;
  const int b = blockIdx.y;
  const int q = blockIdx.x * kCellsPerBlock + threadIdx.x / 64;
  if (q >= Q) return;
  const int lane = threadIdx.x & 63, cl = (lane & (LPW - 1)) * V, ks = lane / LPW;
  const float* pm = prob + (size_t)b * Q * Z;
  const float* am = a + (size_t)b * Q * A;
  const Cell c = make_cell(q, g);
  for (int c0 = 0; c0 < A; c0 += LPW * V) {
    const int ch = c0 + cl;
    const bool on = ch < A;
    Vec<V> M = vec_fill<V>(0.f), Nn = M;
    for (int k = ks; k < g.G; k += 64 / LPW) {
      float nx, ny, len;
      waypoint(c, g, k, nx, ny, len);
      if (len < c.bound && on) {
        const Tap t = make_tap(nx, ny, g);
        const Vec<V> m = tap_load_bins<V>(pm, t, Z, ch, J);
        const Vec<V> av = tap_load<V>(am, t, A, ch);
#pragma unroll
        for (int i = 0; i < V; ++i) { M.e[i] += m.e[i]; Nn.e[i] += av.e[i] * m.e[i]; }
      }
    }
    M = ksum<LPW>(M); Nn = ksum<LPW>(Nn);
    if (ks == 0 && on) {
      Vec<V> f;
#pragma unroll
      for (int i = 0; i < V; ++i) f.e[i] = Nn.e[i] / (M.e[i] + g.eps);
      vec_store<V>(feat + ((size_t)b * Q + q) * A + ch, f);
      float* mrow = msum + ((size_t)b * Q + q) * Z;
      if (J == 1) {
        vec_store<V>(mrow + ch, M);
      } else {
#pragma unroll
        for (int i = 0; i < V; ++i)
          if ((ch + i) % J == 0) mrow[(ch + i) / J] = M.e[i];
      }
    }
  }
}

// stage 2 backward: grad_feat [bs,Q,A] -> grad_prob [bs,Q,Z], grad_a [bs,Q,A] (pre-zeroed, atomics); lane = (waypoint
// slot, channel), A > LPW is walked in chunks.  grad_prob of a bin is summed over the bin's channels inside the wave
// and added by the bin's first lane of the chunk.
template <int LPW, int ZC, class Acc>
__device__ __forceinline__ void lr_gather_bwd(
    const float* __restrict__ prob, const float* __restrict__ a, const float* __restrict__ feat,
    const float* __restrict__ msum, const float* __restrict__ grad_feat,
    float* __restrict__ grad_prob, float* __restrict__ grad_a, int Q, int Zr, int Ar, const Geo& g, int ncopies,
    Acc& acc_prob, Acc& acc_a) {
  const int Z = ZC ? ZC : Zr, A = ZC ? ZC : Ar, J = ZC ? 1 : Ar / Zr;
  const int b = blockIdx.y;
  const int q = blockIdx.x * kCellsPerBlock + threadIdx.x / 64;
  if (q >= Q) return;
  const int lane = threadIdx.x & 63, cl = lane & (LPW - 1), ks = lane / LPW;
  const float* pm = prob + (size_t)b * Q * Z;
  const float* am = a + (size_t)b * Q * A;
  float* gpm = grad_prob + (copy_of_block(ncopies) + b) * Q * Z;
  float* gam = grad_a + (copy_of_block(ncopies) + b) * Q * A;
  const Cell c = make_cell(q, g);
  for (int c0 = 0; c0 < A; c0 += LPW) {
    const int ch = c0 + cl;
    const bool on = ch < A;
    const int bin = on ? ch / J : 0;
    // lanes after this one in the same slot, chunk and bin; the lane that adds the bin's sum
    const int ahead = on ? min(min(J - 1 - ch % J, LPW - 1 - cl), A - 1 - ch) : 0;
    const bool first = on && (cl == 0 || ch % J == 0);
    const float f = on ? feat[((size_t)b * Q + q) * A + ch] : 0.f;
    const float s = on ? grad_feat[((size_t)b * Q + q) * A + ch] / (msum[((size_t)b * Q + q) * Z + bin] + g.eps) : 0.f;
    for (int k = ks; k < g.G; k += 64 / LPW) {
      float nx, ny, len;
      waypoint(c, g, k, nx, ny, len);
      if (len < c.bound) {
        const Tap t = make_tap(nx, ny, g);
        float gp = 0.f;
        if (on) {
          const float m = tap_load<1>(pm, t, Z, bin).e[0];
          const float av = tap_load<1>(am, t, A, ch).e[0];
          tap_scatter1(gam, t, A, ch, s * m, acc_a);
          gp = s * (av - f);
        }
        if (J > 1) gp = group_sum<LPW>(gp, ahead);
        if (first) tap_scatter1(gpm, t, Z, bin, gp, acc_prob);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// The kernels: the released shape under the names it has always had, every other shape as `_any`
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void lr_prob_fwd_kernel(const float* __restrict__ occ, float* __restrict__ prob,
                                                               int Q, Geo g) {
  lr_prob_fwd<4, 4, 16>(occ, prob, Q, 16, g);
}
__global__ __launch_bounds__(kThreads) void lr_prob_bwd_kernel(const float* __restrict__ occ,
                                                               const float* __restrict__ grad_prob,
                                                               float* __restrict__ grad_occ, int Q, Geo g, int ncopies) {
  det::AccAtomic acc;
  lr_prob_bwd<16, 16>(occ, grad_prob, grad_occ, Q, 16, g, ncopies, acc);
}
__global__ __launch_bounds__(kThreads) void lr_gather_fwd_kernel(const float* __restrict__ prob,
                                                                 const float* __restrict__ a, float* __restrict__ feat,
                                                                 float* __restrict__ msum, int Q, Geo g) {
  lr_gather_fwd<4, 4, 16>(prob, a, feat, msum, Q, 16, 16, g);
}
__global__ __launch_bounds__(kThreads) void lr_gather_bwd_kernel(
    const float* __restrict__ prob, const float* __restrict__ a, const float* __restrict__ feat,
    const float* __restrict__ msum, const float* __restrict__ grad_feat,
    float* __restrict__ grad_prob, float* __restrict__ grad_a, int Q, Geo g, int ncopies) {
  det::AccAtomic acc;
  lr_gather_bwd<16, 16>(prob, a, feat, msum, grad_feat, grad_prob, grad_a, Q, 16, 16, g, ncopies, acc, acc);
}
template <int LPW, int V>
__global__ __launch_bounds__(kThreads) void lr_prob_fwd_any_kernel(const float* __restrict__ occ,
                                                                   float* __restrict__ prob, int Q, int Z, Geo g) {
  lr_prob_fwd<LPW, V, 0>(occ, prob, Q, Z, g);
}
template <int LPW>
__global__ __launch_bounds__(kThreads) void lr_prob_bwd_any_kernel(const float* __restrict__ occ,
                                                                   const float* __restrict__ grad_prob,
                                                                   float* __restrict__ grad_occ, int Q, int Z, Geo g,
                                                                   int ncopies) {
  det::AccAtomic acc;
  lr_prob_bwd<LPW, 0>(occ, grad_prob, grad_occ, Q, Z, g, ncopies, acc);
}
template <int LPW, int V>
__global__ __launch_bounds__(kThreads) void lr_gather_fwd_any_kernel(const float* __restrict__ prob,
                                                                     const float* __restrict__ a,
                                                                     float* __restrict__ feat, float* __restrict__ msum,
                                                                     int Q, int Z, int A, Geo g) {
  lr_gather_fwd<LPW, V, 0>(prob, a, feat, msum, Q, Z, A, g);
}
template <int LPW>
__global__ __launch_bounds__(kThreads) void lr_gather_bwd_any_kernel(
    const float* __restrict__ prob, const float* __restrict__ a, const float* __restrict__ feat,
    const float* __restrict__ msum, const float* __restrict__ grad_feat,
    float* __restrict__ grad_prob, float* __restrict__ grad_a, int Q, int Z, int A, Geo g, int ncopies) {
  det::AccAtomic acc;
  lr_gather_bwd<LPW, 0>(prob, a, feat, msum, grad_feat, grad_prob, grad_a, Q, Z, A, g, ncopies, acc, acc);
}

// Deterministic mode (det_acc.h): the shape-generic bodies under the measure policy, then under the fixed-point policy,
// adding straight into the accumulator volumes (no private copies).
template <int LPW, class Acc>
__global__ __launch_bounds__(kThreads) void lr_prob_bwd_det_kernel(const float* __restrict__ occ,
                                                                   const float* __restrict__ grad_prob,
                                                                   float* __restrict__ grad_occ, int Q, int Z, Geo g,
                                                                   typename Acc::Param param) {
  Acc acc(grad_occ, param);
  lr_prob_bwd<LPW, 0>(occ, grad_prob, grad_occ, Q, Z, g, 1, acc);
  acc.flush();
}
template <int LPW, class Acc>
__global__ __launch_bounds__(kThreads) void lr_gather_bwd_det_kernel(
    const float* __restrict__ prob, const float* __restrict__ a, const float* __restrict__ feat,
    const float* __restrict__ msum, const float* __restrict__ grad_feat, float* __restrict__ grad_prob,
    float* __restrict__ grad_a, int Q, int Z, int A, Geo g, typename Acc::Param param_prob,
    typename Acc::Param param_a) {
  Acc acc_prob(grad_prob, param_prob), acc_a(grad_a, param_a);
  lr_gather_bwd<LPW, 0>(prob, a, feat, msum, grad_feat, grad_prob, grad_a, Q, Z, A, g, 1, acc_prob, acc_a);
  acc_prob.flush();
  acc_a.flush();
}

inline bool lr_bad(int bs, int H, int W, int Z, int G, int act) {
  return bs < 0 || H <= 0 || W <= 0 || Z < 1 || Z > kMaxZ || G <= 0 || (act != 0 && act != 1);
}
inline bool lr_bad_group(int Z, int A) { return A < Z || A % Z != 0 || A > kMaxA; }
inline dim3 lr_grid(int bs, int Q) { return dim3((Q + kCellsPerBlock - 1) / kCellsPerBlock, bs); }

// the channel lanes per waypoint for n channels (or float4s of channels), as a compile-time constant for `f`: 1, 4, 16 or
// 64 -- the smallest that covers n, so at most 3/4 of the channel lanes idle; n > 64 is walked in chunks of 64
template <class F>
void with_lanes(int n, F f) {
  if (n <= 1) f(std::integral_constant<int, 1>{});
  else if (n <= 4) f(std::integral_constant<int, 4>{});
  else if (n <= 16) f(std::integral_constant<int, 16>{});
  else f(std::integral_constant<int, 64>{});
}
template <class K, class... Args>
void lr_launch(K kernel, int bs, int Q, hipStream_t s, Args... args) {
  hipLaunchKernelGGL(kernel, lr_grid(bs, Q), dim3(kThreads), 0, s, args...);
}

// The released shape (Z = A = 16) runs the instantiation with its counts compiled in; every other shape picks the lane
// map from its channel count: float4 lanes where the rows are a multiple of 4 floats, scalar lanes otherwise.
void launch_prob_fwd(const float* occ, float* prob, int bs, int H, int W, int Z, Geo g, hipStream_t s) {
  const int Q = H * W;
  if (Z == 16) lr_launch(lr_prob_fwd_kernel, bs, Q, s, occ, prob, Q, g);
  else if (Z % 4 == 0)
    with_lanes(Z / 4, [&](auto l) { lr_launch(lr_prob_fwd_any_kernel<decltype(l)::value, 4>, bs, Q, s, occ, prob, Q, Z, g); });
  else
    with_lanes(Z, [&](auto l) { lr_launch(lr_prob_fwd_any_kernel<decltype(l)::value, 1>, bs, Q, s, occ, prob, Q, Z, g); });
}
void launch_prob_bwd(const float* occ, const float* go, float* acc, int bs, int H, int W, int Z, Geo g, int ncopies,
                     hipStream_t s) {
  const int Q = H * W;
  if (Z == 16) lr_launch(lr_prob_bwd_kernel, bs, Q, s, occ, go, acc, Q, g, ncopies);
  else
    with_lanes(Z, [&](auto l) {
      lr_launch(lr_prob_bwd_any_kernel<decltype(l)::value>, bs, Q, s, occ, go, acc, Q, Z, g, ncopies);
    });
}
void launch_gather_fwd(const float* prob, const float* a, float* feat, float* msum, int bs, int H, int W, int Z, int A,
                       Geo g, hipStream_t s) {
  const int Q = H * W;
  if (Z == 16 && A == 16) lr_launch(lr_gather_fwd_kernel, bs, Q, s, prob, a, feat, msum, Q, g);
  else if (A % 4 == 0)
    with_lanes(A / 4, [&](auto l) {
      lr_launch(lr_gather_fwd_any_kernel<decltype(l)::value, 4>, bs, Q, s, prob, a, feat, msum, Q, Z, A, g);
    });
  else
    with_lanes(A, [&](auto l) {
      lr_launch(lr_gather_fwd_any_kernel<decltype(l)::value, 1>, bs, Q, s, prob, a, feat, msum, Q, Z, A, g);
    });
}

// The two gradient maps of the stage 2 backward differ in size (Z and A channels); the copies are summed as float4
// where both sizes allow it.
int gather_bwd(const float* prob, const float* a, const float* feat, const float* msum, const float* grad_feat,
               float* grad_prob, float* grad_a, int bs, int H, int W, int Z, int A, Geo g, void* workspace,
               size_t workspace_bytes, hipStream_t s) {
  const size_t nz = (size_t)bs * H * W * Z, na = (size_t)bs * H * W * A;
  const int Q = H * W;
  const auto launch = [&](float* sp, float* sa, int ncopies) {
    if (Z == 16 && A == 16)
      lr_launch(lr_gather_bwd_kernel, bs, Q, s, prob, a, feat, msum, grad_feat, sp, sa, Q, g, ncopies);
    else
      with_lanes(A, [&](auto l) {
        lr_launch(lr_gather_bwd_any_kernel<decltype(l)::value>, bs, Q, s, prob, a, feat, msum, grad_feat, sp, sa, Q, Z, A,
                  g, ncopies);
      });
  };
  const auto det_launch = [&](auto tag, auto param_prob, auto param_a) {
    with_lanes(A, [&](auto l) {
      lr_launch(lr_gather_bwd_det_kernel<decltype(l)::value, decltype(tag)>, bs, Q, s, prob, a, feat, msum, grad_feat,
                grad_prob, grad_a, Q, Z, A, g, param_prob, param_a);
    });
  };
  const uint64_t adds = (uint64_t)na * g.G * 4;   // 4 corners of G waypoints per (cell, channel), for either map
  if ((nz | na) % 4 == 0)
    return scatter_backward<float4>(grad_prob, grad_a, nz, na, adds, false, workspace, workspace_bytes, s, launch, det_launch);
  return scatter_backward<float>(grad_prob, grad_a, nz, na, adds, false, workspace, workspace_bytes, s, launch, det_launch);
}

}  // namespace

extern "C" {

size_t vidar_latent_render_bwd_workspace_bytes(int bs, int H, int W, int Z, int maps) {
  if (bs <= 0 || H <= 0 || W <= 0 || Z <= 0 || maps < 1 || maps > 2) return 0;
  // maps: 1 = prob_bwd (grad_occ), 2 = gather_bwd
  return scatter_backward_workspace_bytes((size_t)bs * H * W * Z * maps, maps);
}

int vidar_latent_render_prob_fwd_f32(const float* occ, float* path_prob, int bs, int H, int W, int Z,
                                     int grid_num, float step, int act, void* stream) {
  VIDAR_ENTER();
  if (lr_bad(bs, H, W, Z, grid_num, act)) return VIDAR_ERR_BAD_ARG;
  if (bs == 0) return 0;
  launch_prob_fwd(occ, path_prob, bs, H, W, Z, Geo{H, W, grid_num, step, act, 0.f}, (hipStream_t)stream);
  return vidar_last_error();
}

int vidar_latent_render_prob_bwd_f32(const float* occ, const float* grad_path_prob, float* grad_occ,
                                     int bs, int H, int W, int Z, int grid_num, float step, int act,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  VIDAR_ENTER();
  if (lr_bad(bs, H, W, Z, grid_num, act)) return VIDAR_ERR_BAD_ARG;
  if (bs == 0) return 0;   // before anything is touched
  hipStream_t s = (hipStream_t)stream;
  Geo g{H, W, grid_num, step, act, 0.f};
  const size_t n = (size_t)bs * H * W * Z;
  const auto launch = [&](float* acc, float*, int ncopies) {
    launch_prob_bwd(occ, grad_path_prob, acc, bs, H, W, Z, g, ncopies, s);
  };
  const auto det_launch = [&](auto tag, auto param, auto) {
    with_lanes(Z, [&](auto l) {
      lr_launch(lr_prob_bwd_det_kernel<decltype(l)::value, decltype(tag)>, bs, H * W, s, occ, grad_path_prob, grad_occ,
                H * W, Z, g, param);
    });
  };
  // 4 corners of the G waypoints and of the cell itself per (cell, bin)
  const uint64_t adds = (uint64_t)n * ((uint64_t)grid_num + 1) * 4;
  if (n % 4 == 0)
    return scatter_backward<float4>(grad_occ, nullptr, n, 0, adds, false, workspace, workspace_bytes, s, launch, det_launch);
  return scatter_backward<float>(grad_occ, nullptr, n, 0, adds, false, workspace, workspace_bytes, s, launch, det_launch);
}

int vidar_latent_render_gather_grouped_fwd_f32(const float* path_prob, const float* lora_a, float* feat, float* msum,
                                               int bs, int H, int W, int Z, int A, int grid_num, float step,
                                               float eps, void* stream) {
  VIDAR_ENTER();
  if (lr_bad(bs, H, W, Z, grid_num, 0) || lr_bad_group(Z, A)) return VIDAR_ERR_BAD_ARG;
  if (bs == 0) return 0;
  launch_gather_fwd(path_prob, lora_a, feat, msum, bs, H, W, Z, A, Geo{H, W, grid_num, step, 0, eps},
                    (hipStream_t)stream);
  return vidar_last_error();
}

int vidar_latent_render_gather_grouped_bwd_f32(const float* path_prob, const float* lora_a, const float* feat,
                                               const float* msum, const float* grad_feat, float* grad_path_prob,
                                               float* grad_lora_a, int bs, int H, int W, int Z, int A, int grid_num,
                                               float step, float eps, void* workspace, size_t workspace_bytes,
                                               void* stream) {
  VIDAR_ENTER();
  if (lr_bad(bs, H, W, Z, grid_num, 0) || lr_bad_group(Z, A)) return VIDAR_ERR_BAD_ARG;
  if (bs == 0) return 0;   // before anything is touched
  return gather_bwd(path_prob, lora_a, feat, msum, grad_feat, grad_path_prob, grad_lora_a, bs, H, W, Z, A,
                    Geo{H, W, grid_num, step, 0, eps}, workspace, workspace_bytes, (hipStream_t)stream);
}

int vidar_latent_render_gather_fwd_f32(const float* path_prob, const float* lora_a, float* feat,
                                       float* msum, int bs, int H, int W, int Z, int grid_num,
                                       float step, float eps, void* stream) {
  return vidar_latent_render_gather_grouped_fwd_f32(path_prob, lora_a, feat, msum, bs, H, W, Z, Z, grid_num, step, eps,
                                                    stream);
}

int vidar_latent_render_gather_bwd_f32(const float* path_prob, const float* lora_a, const float* feat,
                                       const float* msum, const float* grad_feat,
                                       float* grad_path_prob, float* grad_lora_a, int bs, int H,
                                       int W, int Z, int grid_num, float step, float eps,
                                       void* workspace, size_t workspace_bytes, void* stream) {
  return vidar_latent_render_gather_grouped_bwd_f32(path_prob, lora_a, feat, msum, grad_feat, grad_path_prob,
                                                    grad_lora_a, bs, H, W, Z, Z, grid_num, step, eps, workspace,
                                                    workspace_bytes, stream);
}

}  // extern "C"
