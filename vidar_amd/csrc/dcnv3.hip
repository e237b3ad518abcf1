// Deformable convolution v3 (DCNv3) sampling kernels for gfx950: the core op of the InternImage backbone.
//
// Replaces the reference's fifth native extension, projects/mmdet3d_plugin/bevformer/backbones/ops_dcnv3
// (forward src/cuda/dcnv3_im2col_cuda.cuh:217-276, backward :149-213 and :776-839, host side dcnv3_cuda.cu).
// Channel-last, fp32:
//   input [N,H,W,G*gc], offset [N,Ho,Wo,G*P*2] as (w, h) pairs, mask [N,Ho,Wo,G*P], P = kh*kw, point p = i_w*kh + j_h,
//   out[n,ho,wo,g,:] = sum_p mask_p * bilinear(input[n,:,:,g,:], loc_p)       (zero outside the image)
//   loc = (p0 - ((dil*(k-1))>>1)*offset_scale) + (i*dil + offset)*offset_scale,  p0 = ((dil*(k-1))>>1) - pad + out*stride;
//   a point counts iff loc_h > -1 && loc_w > -1 && loc_h < H && loc_w < W.
// This file is compiled without multiply-add contraction, and the location is evaluated in the reference's operation
// order, so the in/out decision and the bilinear cell are the reference's whenever the operands are.
//
// Work split.  An ITEM is one (image, output pixel, group); it is served by LP = 2^k lanes of one wave, each lane owning
// V channels (V = 4: one 16-byte load per corner when gc % 4 == 0, V = 1 otherwise) and walking the group's channels in
// steps of LP*V.  The 3P offset / mask values of an item are read at one address by its LP lanes (one request), not once
// per channel as the reference does; a corner fetch of an item is one contiguous gc*4-byte segment.
// Backward: grad_offset / grad_mask are the sums over the gc channels of one (item, point): per-lane partial sums, then a
// butterfly over the item's LP lanes and ONE plain store per value -- no atomics, bit-reproducible.  grad_input is zeroed
// by the call and accumulated with fp32 hardware atomics, the item's lanes adding neighbouring addresses of one segment.
// Workgroup order: hardware deals consecutive workgroup ids round-robin to the 8 XCDs; here XCD k walks the k-th
// contiguous eighth of the item range, with the intent that the rows of one image (whose footprints overlap) meet in one L2
// (not measured against the plain order).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vidar_hip.h"
#include "vidar_common.h"

namespace {

constexpr int kMaxPoints = 1024;     // kh*kw accepted by the entry points (the kernels loop over points: no resource depends on it)

struct Geo {
  int H, W, Ho, Wo, kh, kw, sh, sw, ph, pw, dh, dw, G, gc;
  float os;
};

template <int V> struct Vec;
template <> struct Vec<1> { typedef float T; };
template <> struct Vec<4> { typedef float4 T; };

__device__ __forceinline__ float4 operator*(float a, const float4& b) { return make_float4(a * b.x, a * b.y, a * b.z, a * b.w); }
__device__ __forceinline__ float4 operator+(const float4& a, const float4& b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float dotv(float a, float b) { return a * b; }
__device__ __forceinline__ float dotv(const float4& a, const float4& b) { return ((a.x * b.x + a.y * b.y) + a.z * b.z) + a.w * b.w; }
__device__ __forceinline__ void zero(float& a) { a = 0.f; }
__device__ __forceinline__ void zero(float4& a) { a = make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ void atomic_addv(float* p, float v) { if (v != 0.f) unsafeAtomicAdd(p, v); }
__device__ __forceinline__ void atomic_addv(float* p, const float4& v) {
  atomic_addv(p, v.x); atomic_addv(p + 1, v.y); atomic_addv(p + 2, v.z); atomic_addv(p + 3, v.w);
}

// the item of this lane: blocks are renumbered so that XCD (blockIdx % 8) owns a contiguous range of items
struct Item { int n, ho, wo, g, sub; bool ok; };
__device__ __forceinline__ Item my_item(const Geo& q, int lp, int blocks, int items) {
  const int per = (blocks + 7) >> 3;
  const int b = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
  const int ipb = 256 / lp;
  Item it;
  it.sub = (int)threadIdx.x % lp;
  // b * ipb <= items + 256 < 2^31 (items is checked against 2^31 - 512 by the host side)
  int id = (b < blocks) ? b * ipb + (int)threadIdx.x / lp : items;
  it.ok = id < items;
  if (!it.ok) id = 0;
  it.g = id % q.G; id /= q.G;
  it.wo = id % q.Wo; id /= q.Wo;
  it.ho = id % q.Ho; it.n = id / q.Ho;
  return it;
}

struct Cell {
  int h0, w0;
  float lh, lw;
  bool in, t, b, l, r;
};

// sampling location of point (i over kernel_w, j over kernel_h) in the reference's operation order (:249-260)
__device__ __forceinline__ Cell cell(const Geo& q, int ho, int wo, int i, int j, float off_w, float off_h) {
  const int p0_w = ((q.dw * (q.kw - 1)) >> 1) - q.pw + wo * q.sw;
  const int p0_h = ((q.dh * (q.kh - 1)) >> 1) - q.ph + ho * q.sh;
  const float p0_w_ = p0_w - ((q.dw * (q.kw - 1)) >> 1) * q.os;
  const float p0_h_ = p0_h - ((q.dh * (q.kh - 1)) >> 1) * q.os;
  const float w = p0_w_ + (i * q.dw + off_w) * q.os;
  const float h = p0_h_ + (j * q.dh + off_h) * q.os;
  Cell c;
  c.in = h > -1.f && w > -1.f && h < q.H && w < q.W;
  const float fh = floorf(h), fw = floorf(w);
  c.h0 = c.in ? (int)fh : 0; c.w0 = c.in ? (int)fw : 0;
  c.lh = h - fh; c.lw = w - fw;
  c.t = c.h0 >= 0; c.b = c.h0 + 1 <= q.H - 1; c.l = c.w0 >= 0; c.r = c.w0 + 1 <= q.W - 1;
  return c;
}

template <int V>
__global__ __launch_bounds__(256) void dcnv3_fwd_kernel(const float* __restrict__ input, const float* __restrict__ offset,
                                                        const float* __restrict__ mask, float* __restrict__ out, Geo q,
                                                        int lp, int blocks, int items) {
  typedef typename Vec<V>::T T;
  const Item it = my_item(q, lp, blocks, items);
  if (!it.ok) return;
  const int P = q.kh * q.kw, C = q.G * q.gc;
  const size_t pix = ((size_t)it.n * q.Ho + it.ho) * q.Wo + it.wo;
  const float* off = offset + (pix * q.G + it.g) * P * 2;
  const float* msk = mask + (pix * q.G + it.g) * P;
  const float* im = input + (size_t)it.n * q.H * q.W * C + it.g * q.gc;
  for (int c = it.sub * V; c < q.gc; c += lp * V) {
    T acc; zero(acc);
    int i = 0, j = 0;
    for (int p = 0; p < P; ++p) {
      const Cell k = cell(q, it.ho, it.wo, i, j, off[2 * p], off[2 * p + 1]);
      const float m = msk[p];
      if (++j == q.kh) { j = 0; ++i; }
      if (!k.in) continue;
      const float* a = im + ((size_t)k.h0 * q.W + k.w0) * C + c;
      const size_t dn = (size_t)q.W * C;
      T v1, v2, v3, v4; zero(v1); zero(v2); zero(v3); zero(v4);
      if (k.t && k.l) v1 = *reinterpret_cast<const T*>(a);
      if (k.t && k.r) v2 = *reinterpret_cast<const T*>(a + C);
      if (k.b && k.l) v3 = *reinterpret_cast<const T*>(a + dn);
      if (k.b && k.r) v4 = *reinterpret_cast<const T*>(a + dn + C);
      const float hh = 1.f - k.lh, hw = 1.f - k.lw;
      const T val = (((hh * hw) * v1 + (hh * k.lw) * v2) + (k.lh * hw) * v3) + (k.lh * k.lw) * v4;
      acc = acc + m * val;
    }
    *reinterpret_cast<T*>(out + pix * C + it.g * q.gc + c) = acc;
  }
}

// LDS window of the on-chip grad_input accumulation (dcnv3_bwd_lds_kernel): rows / columns [y0, y0 + wh) x [x0, x0 + ww) of
// the input, gc channels of one group per pixel.  wh == 0: no window, every contribution is a global atomic.
struct Window { float* s; int y0, x0, wh, ww; };

__device__ __forceinline__ void lds_addv(float* p, float v) { if (v != 0.f) atomicAdd(p, v); }
__device__ __forceinline__ void lds_addv(float* p, const float4& v) {
  lds_addv(p, v.x); lds_addv(p + 1, v.y); lds_addv(p + 2, v.z); lds_addv(p + 3, v.w);
}

// backward of one item by its lp lanes (all of them enter, `ok` is the same on all): grad_offset / grad_mask are reduced
// over the lanes and stored by lane 0; a grad_input contribution goes to the window when its pixel is inside, else to memory
template <int V>
__device__ __forceinline__ void bwd_item(const float* __restrict__ input, const float* __restrict__ offset,
                                         const float* __restrict__ mask, const float* __restrict__ grad_out,
                                         float* __restrict__ grad_input, float* __restrict__ grad_offset,
                                         float* __restrict__ grad_mask, const Geo& q, int lp, const Item& it, const Window& wn) {
  typedef typename Vec<V>::T T;
  const int P = q.kh * q.kw, C = q.G * q.gc;
  const size_t pix = ((size_t)it.n * q.Ho + it.ho) * q.Wo + it.wo;
  const size_t o = (pix * q.G + it.g) * P;
  const float* off = offset + o * 2;
  const float* msk = mask + o;
  const size_t img = (size_t)it.n * q.H * q.W * C + it.g * q.gc;
  const float* im = input + img;
  float* gim = grad_input + img;
  const float* go = grad_out + pix * C + it.g * q.gc;
  const size_t dn = (size_t)q.W * C;
  int i = 0, j = 0;
  for (int p = 0; p < P; ++p) {
    float gh = 0.f, gw = 0.f, gm = 0.f;
    if (it.ok) {
      const Cell k = cell(q, it.ho, it.wo, i, j, off[2 * p], off[2 * p + 1]);
      const float m = msk[p];
      if (k.in) {
        const float hh = 1.f - k.lh, hw = 1.f - k.lw;
        const int ly = k.h0 - wn.y0, lx = k.w0 - wn.x0;
        // the four corners share one test: rows ly, ly + 1 and columns lx, lx + 1 inside the window
        const bool in_win = ly >= 0 && ly + 1 < wn.wh && lx >= 0 && lx + 1 < wn.ww;
        for (int c = it.sub * V; c < q.gc; c += lp * V) {
          const T tg = *reinterpret_cast<const T*>(go + c);
          const T tgm = m * tg;
          const size_t a = ((size_t)k.h0 * q.W + k.w0) * C + c;
          T v1, v2, v3, v4; zero(v1); zero(v2); zero(v3); zero(v4);
          if (k.t && k.l) v1 = *reinterpret_cast<const T*>(im + a);
          if (k.t && k.r) v2 = *reinterpret_cast<const T*>(im + a + C);
          if (k.b && k.l) v3 = *reinterpret_cast<const T*>(im + a + dn);
          if (k.b && k.r) v4 = *reinterpret_cast<const T*>(im + a + dn + C);
          if (in_win) {
            float* w = wn.s + ((size_t)ly * wn.ww + lx) * q.gc + c;
            const int wd = wn.ww * q.gc;
            if (k.t && k.l) lds_addv(w, (hh * hw) * tgm);
            if (k.t && k.r) lds_addv(w + q.gc, (hh * k.lw) * tgm);
            if (k.b && k.l) lds_addv(w + wd, (k.lh * hw) * tgm);
            if (k.b && k.r) lds_addv(w + wd + q.gc, (k.lh * k.lw) * tgm);
          } else {
            if (k.t && k.l) atomic_addv(gim + a, (hh * hw) * tgm);
            if (k.t && k.r) atomic_addv(gim + a + C, (hh * k.lw) * tgm);
            if (k.b && k.l) atomic_addv(gim + a + dn, (k.lh * hw) * tgm);
            if (k.b && k.r) atomic_addv(gim + a + dn + C, (k.lh * k.lw) * tgm);
          }
          // d val / d loc_h = hw (v3 - v1) + lw (v4 - v2),  d val / d loc_w = hh (v2 - v1) + lh (v4 - v3)   (:181-206)
          gh += dotv(tgm, ((-hw) * v1 + (-k.lw) * v2) + (hw * v3 + k.lw * v4));
          gw += dotv(tgm, ((-hh) * v1 + hh * v2) + ((-k.lh) * v3 + k.lh * v4));
          gm += dotv(tg, (((hh * hw) * v1 + (hh * k.lw) * v2) + (k.lh * hw) * v3) + (k.lh * k.lw) * v4);
        }
      }
    }
    if (++j == q.kh) { j = 0; ++i; }
    for (int s = lp >> 1; s > 0; s >>= 1) {
      gh += __shfl_xor(gh, s, 64);
      gw += __shfl_xor(gw, s, 64);
      gm += __shfl_xor(gm, s, 64);
    }
    if (it.ok && it.sub == 0) {
      grad_offset[(o + p) * 2] = q.os * gw;
      grad_offset[(o + p) * 2 + 1] = q.os * gh;
      grad_mask[o + p] = gm;
    }
  }
}

template <int V>
__global__ __launch_bounds__(256) void dcnv3_bwd_kernel(const float* __restrict__ input, const float* __restrict__ offset,
                                                        const float* __restrict__ mask, const float* __restrict__ grad_out,
                                                        float* __restrict__ grad_input, float* __restrict__ grad_offset,
                                                        float* __restrict__ grad_mask, Geo q, int lp, int blocks, int items) {
  const Item it = my_item(q, lp, blocks, items);
  bwd_item<V>(input, offset, mask, grad_out, grad_input, grad_offset, grad_mask, q, lp, it, Window{nullptr, 0, 0, 0, 0});
}

// On-chip accumulation of grad_input.  A workgroup owns a th x tw tile of output pixels of ONE (image, group).  Learned
// offsets are a few pixels, so the tile's samples fall into a bounded window of the input -- the tile's footprint, the
// kernel extent, the bilinear neighbour and kHalo pixels on every side: it is kept in LDS ([row][column][gc] floats), the
// contributions are added there (ds_add_f32) and the window is flushed ONCE, lanes running over the gc channels of a pixel so
// that an atomic instruction covers contiguous segments; zero entries are skipped.  A sample whose cell leaves the window
// (far-field offsets, unusual offset_scale) adds straight to memory as in the plain form.
constexpr int kHalo = 3;
struct Tiling { int th, tw, wh, ww, tiles_y, tiles_x; };

template <int V>
__global__ __launch_bounds__(256) void dcnv3_bwd_lds_kernel(const float* __restrict__ input, const float* __restrict__ offset,
                                                            const float* __restrict__ mask, const float* __restrict__ grad_out,
                                                            float* __restrict__ grad_input, float* __restrict__ grad_offset,
                                                            float* __restrict__ grad_mask, Geo q, Tiling tl, int lp, int blocks) {
  extern __shared__ __attribute__((aligned(16))) float s_win[];
  const int per = (blocks + 7) >> 3;
  const int b = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);     // XCD k: the k-th contiguous eighth of the tiles
  if (b >= blocks) return;
  const int tiles = tl.tiles_y * tl.tiles_x;
  const int tile = b % tiles, r = b / tiles, g = r % q.G, n = r / q.G;
  const int ty0 = (tile / tl.tiles_x) * tl.th, tx0 = (tile % tl.tiles_x) * tl.tw;
  const Window wn{s_win, ty0 * q.sh - q.ph - kHalo, tx0 * q.sw - q.pw - kHalo, tl.wh, tl.ww};
  const int nwin = tl.wh * tl.ww * q.gc;
  for (int e = threadIdx.x; e < nwin; e += 256) s_win[e] = 0.f;
  __syncthreads();
  const int ipb = 256 / lp, npix = tl.th * tl.tw;
  for (int base = 0; base < npix; base += ipb) {          // same trip count on every lane: the butterflies are complete
    const int px = base + (int)threadIdx.x / lp;
    const int ly = px / tl.tw, lx = px - ly * tl.tw;
    Item it;
    it.n = n; it.g = g; it.ho = ty0 + ly; it.wo = tx0 + lx; it.sub = (int)threadIdx.x % lp;
    it.ok = px < npix && it.ho < q.Ho && it.wo < q.Wo;
    if (!it.ok) { it.ho = 0; it.wo = 0; }
    bwd_item<V>(input, offset, mask, grad_out, grad_input, grad_offset, grad_mask, q, lp, it, wn);
  }
  __syncthreads();
  const int C = q.G * q.gc;
  float* gim = grad_input + (size_t)n * q.H * q.W * C + g * q.gc;
  for (int e = threadIdx.x; e < nwin; e += 256) {
    const float v = s_win[e];
    const int pi = e / q.gc, c = e - pi * q.gc;
    const int wy = pi / tl.ww, h = wn.y0 + wy, w = wn.x0 + (pi - wy * tl.ww);
    if (v != 0.f && h >= 0 && h < q.H && w >= 0 && w < q.W) unsafeAtomicAdd(gim + ((size_t)h * q.W + w) * C + c, v);
  }
}

int g_dcnv3_variant = 1;       // vidar_dcnv3_set_variant; 1 measured fastest (profiles/kbench_dcnv3.md)

struct Plan { Geo q; int lp, blocks, items; bool vec; };

// 0 = nothing to do, 1 = launch, < 0 = VIDAR_ERR_BAD_ARG
int plan(Plan& pl, int N, int H, int W, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int G, int gc,
         float os) {
  if (N < 0 || H <= 0 || W <= 0 || kh <= 0 || kw <= 0 || sh <= 0 || sw <= 0 || ph < 0 || pw < 0 || dh <= 0 || dw <= 0 ||
      G <= 0 || gc <= 0 || !(os == os))
    return VIDAR_ERR_BAD_ARG;
  const long long eh = (long long)dh * (kh - 1) + 1, ew = (long long)dw * (kw - 1) + 1;
  const long long P = (long long)kh * kw;
  if (P > kMaxPoints || eh > (1 << 20) || ew > (1 << 20) || ph > (1 << 20) || pw > (1 << 20)) return VIDAR_ERR_BAD_ARG;
  if (H + 2LL * ph < eh || W + 2LL * pw < ew) return VIDAR_ERR_BAD_ARG;
  const long long Ho = (H + 2LL * ph - eh) / sh + 1, Wo = (W + 2LL * pw - ew) / sw + 1;
  const long long lim = (1LL << 31) - 512;       // every tensor is indexed with 32-bit element counts in mind (:226-247)
  const long long C = (long long)G * gc;
  if (C >= lim || (long long)N * H * W >= lim / C || (long long)N * Ho * Wo >= lim / C) return VIDAR_ERR_BAD_ARG;
  if ((long long)N * Ho * Wo * G >= lim / (2 * P)) return VIDAR_ERR_BAD_ARG;
  if ((long long)Ho * sh + eh + ph >= lim || (long long)Wo * sw + ew + pw >= lim) return VIDAR_ERR_BAD_ARG;
  if (N == 0) return 0;
  pl.q = Geo{H, W, (int)Ho, (int)Wo, kh, kw, sh, sw, ph, pw, dh, dw, G, gc, os};
  pl.vec = gc % 4 == 0;
  const int chunks = pl.vec ? gc / 4 : gc;
  int lp = 1;
  while (lp < chunks && lp < 64) lp <<= 1;
  pl.lp = lp;
  pl.items = (int)((long long)N * Ho * Wo * G);
  const int ipb = 256 / lp;
  pl.blocks = (pl.items + ipb - 1) / ipb;
  return 1;
}

// 16-byte loads need 16-byte row starts: a group size that is a multiple of 4 on unaligned buffers takes the scalar form
inline void to_scalar(Plan& pl) {
  int lp = 1;
  while (lp < pl.q.gc && lp < 64) lp <<= 1;
  pl.lp = lp;
  pl.blocks = (pl.items + 256 / lp - 1) / (256 / lp);
}
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline unsigned grid_of(const Plan& pl) { return 8u * (unsigned)((pl.blocks + 7) / 8); }

}  // namespace

extern "C" {

int vidar_dcnv3_set_variant(int variant) {
  const int prev = g_dcnv3_variant;
  if (variant >= 0 && variant <= 3) g_dcnv3_variant = variant;
  return prev;
}

size_t vidar_dcnv3_backward_workspace_bytes(int N, int H, int W, int kh, int kw, int stride_h, int stride_w, int pad_h,
                                            int pad_w, int dil_h, int dil_w, int group, int group_channels) {
  (void)N; (void)H; (void)W; (void)kh; (void)kw; (void)stride_h; (void)stride_w; (void)pad_h; (void)pad_w; (void)dil_h;
  (void)dil_w; (void)group; (void)group_channels;
  return 0;      // reserved: every form of the backward accumulates on chip or straight into grad_input
}

int vidar_dcnv3_forward_f32(const float* input, const float* offset, const float* mask, float* out, int N, int H, int W,
                            int kh, int kw, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w,
                            int group, int group_channels, float offset_scale, void* stream) {
  VIDAR_ENTER();
  Plan pl;
  const int rc = plan(pl, N, H, W, kh, kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, group, group_channels, offset_scale);
  if (rc <= 0) return rc;
  if (!input || !offset || !mask || !out) return VIDAR_ERR_BAD_ARG;
  if (pl.vec && aligned16(input) && aligned16(out))
    hipLaunchKernelGGL(dcnv3_fwd_kernel<4>, dim3(grid_of(pl)), dim3(256), 0, (hipStream_t)stream, input, offset, mask, out,
                       pl.q, pl.lp, pl.blocks, pl.items);
  else {
    to_scalar(pl);
    hipLaunchKernelGGL(dcnv3_fwd_kernel<1>, dim3(grid_of(pl)), dim3(256), 0, (hipStream_t)stream, input, offset, mask, out,
                       pl.q, pl.lp, pl.blocks, pl.items);
  }
  return vidar_last_error();
}

int vidar_dcnv3_backward_f32(const float* input, const float* offset, const float* mask, const float* grad_out,
                             float* grad_input, float* grad_offset, float* grad_mask, int N, int H, int W, int kh, int kw,
                             int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w, int group,
                             int group_channels, float offset_scale, void* workspace, size_t workspace_bytes, void* stream) {
  VIDAR_ENTER();
  (void)workspace; (void)workspace_bytes;
  Plan pl;
  const int rc = plan(pl, N, H, W, kh, kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, group, group_channels, offset_scale);
  if (rc <= 0) return rc;
  if (!input || !offset || !mask || !grad_out || !grad_input || !grad_offset || !grad_mask) return VIDAR_ERR_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(grad_input, 0, sizeof(float) * (size_t)N * H * W * group * group_channels, s);
  if (e != hipSuccess) return (int)e;
  bool vec = pl.vec && aligned16(input) && aligned16(grad_out) && (g_dcnv3_variant & 1) == 0;
  if (!vec) to_scalar(pl);
  // the largest tile whose window fits 64 KiB of LDS; none (huge kernels / groups): the plain form
  Tiling tl{0, 0, 0, 0, 0, 0};
  if (g_dcnv3_variant >= 2) {
    static const int cand[5][2] = {{16, 16}, {16, 8}, {8, 8}, {8, 4}, {4, 4}};
    for (int c = 0; c < 5 && tl.th == 0; ++c) {
      const long long wh = (long long)(cand[c][0] - 1) * stride_h + (long long)dil_h * (kh - 1) + 2 + 2 * kHalo;
      const long long ww = (long long)(cand[c][1] - 1) * stride_w + (long long)dil_w * (kw - 1) + 2 + 2 * kHalo;
      if (wh * ww * group_channels * 4 <= 65536)
        tl = Tiling{cand[c][0], cand[c][1], (int)wh, (int)ww, (pl.q.Ho + cand[c][0] - 1) / cand[c][0],
                    (pl.q.Wo + cand[c][1] - 1) / cand[c][1]};
    }
  }
  if (tl.th) {
    const long long blocks = (long long)N * group * tl.tiles_y * tl.tiles_x;      // <= items < 2^31
    const unsigned grid = 8u * (unsigned)((blocks + 7) / 8);
    const size_t lds = sizeof(float) * (size_t)tl.wh * tl.ww * group_channels;
    if (vec)
      hipLaunchKernelGGL(dcnv3_bwd_lds_kernel<4>, dim3(grid), dim3(256), lds, s, input, offset, mask, grad_out, grad_input,
                         grad_offset, grad_mask, pl.q, tl, pl.lp, (int)blocks);
    else
      hipLaunchKernelGGL(dcnv3_bwd_lds_kernel<1>, dim3(grid), dim3(256), lds, s, input, offset, mask, grad_out, grad_input,
                         grad_offset, grad_mask, pl.q, tl, pl.lp, (int)blocks);
  } else if (vec)
    hipLaunchKernelGGL(dcnv3_bwd_kernel<4>, dim3(grid_of(pl)), dim3(256), 0, s, input, offset, mask, grad_out, grad_input,
                       grad_offset, grad_mask, pl.q, pl.lp, pl.blocks, pl.items);
  else
    hipLaunchKernelGGL(dcnv3_bwd_kernel<1>, dim3(grid_of(pl)), dim3(256), 0, s, input, offset, mask, grad_out, grad_input,
                       grad_offset, grad_mask, pl.q, pl.lp, pl.blocks, pl.items);
  return vidar_last_error();
}

}  // extern "C"
