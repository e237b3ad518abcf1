// Device-side image pipeline: raw uint8 HWC BGR camera frames -> fp32 [n, 3, Hpad, Wpad] network input, the arithmetic of
// vidar_amd/data/augment.py + reader.normalise_pad (PhotoMetricDistortionMultiViewImage, CropResizeFlipImage = PIL
// crop / bicubic resize / flip, NormalizeMultiviewImage, RandomScaleImageMultiViewImage, PadMultiViewImage) with the
// host path's bits.  One call serves every image of a sample (n = T * cams) with per-image photometric parameters:
//   * img_photo_kernel     pixel-wise photometric distortion in fp32, then THE uint8 cast (truncate toward zero to int32,
//                          keep the low 8 bits) -- or fp32 out, for tests;
//   * img_resample_h_kernel / img_resample_v_kernel
//                          PIL's two-pass 8-bit resampler in integers: 22-bit fixed-point coefficient tables built by the
//                          host in float64 (vidar_amd/data/device_prep.py), uint8 intermediate, the crop folded into the
//                          indexing (the tables refer to the crop window), the flip into the horizontal pass' output column;
//   * img_normalise_kernel (x - mean) / std with optional channel reversal, optional photometric stage on the taps (fp32,
//                          no uint8 cast: the OpenScene pipeline), optional bilinear resize of the NORMALISED values
//                          (torch's align_corners=False source index), HWC -> CHW, and the zero padding at bottom / right
//                          written by the kernel itself.
// All per-pixel math lives in img_prep_math.h, which the CPU tests compile for the host.
//
// Kernel notes (gfx950, wave64).  Everything here is streaming, bandwidth-side work: 30 images of 900 x 1600 are 130 MB of
// uint8 in and up to 535 MB of fp32 out, against a few dozen integer / fp32 operations per byte.
//   * a uint8 HWC pixel is 3 bytes, so a lane owns 4 pixels = 12 bytes = 3 dwords (one dwordx3 load when the 12 bytes are
//     dword-aligned, i.e. the row / image starts on a dword; byte loads otherwise and in the tail when the extent is no
//     multiple of 4).  Consecutive lanes own consecutive 12-byte groups: a wave reads 768 contiguous bytes.
//   * fp32 CHW output: the same lane stores its 4 pixels of a channel with one 16-byte store (the padded width is a
//     multiple of 4 by contract, rows therefore 16-byte aligned); a wave writes 1 KiB contiguous per channel.
//   * the vertical resample pass is per BYTE column (channels do not mix), so a lane owns 4 consecutive bytes of an output
//     row and walks the taps down the rows: dword loads, fully coalesced.  The horizontal pass gathers bytes (neighbouring
//     lanes read overlapping windows of the same cache lines).  int32 accumulation: sum |k| * 255 < 2^31.
//   * no LDS, no atomics; grids are flat 1-D with 64-bit element indices.
//   * compiled with -ffp-contract=off (the library default) and hipcc's correctly rounded fp32 division: bit-identical to
//     numpy is the requirement, see img_prep_math.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vidar_hip.h"
#include "vidar_common.h"
#include "img_prep_math.h"

namespace {

constexpr int kThreads = 256;

struct alignas(4) Bytes12 { uint32_t w[3]; };
struct Norm3 { float mean[3], stdv[3]; };

__device__ __forceinline__ bool dword_aligned(const void* p) { return ((uintptr_t)p & 3u) == 0; }

// 4 pixels (12 bytes) starting at p; `count` of them exist (1..4)
__device__ __forceinline__ Bytes12 load_quad(const uint8_t* p, int count) {
  Bytes12 v;
  if (count == 4 && dword_aligned(p)) {
    v = *reinterpret_cast<const Bytes12*>(p);
  } else {
    v.w[0] = v.w[1] = v.w[2] = 0;
    for (int k = 0; k < count * 3; ++k) v.w[k >> 2] |= (uint32_t)p[k] << ((k & 3) * 8);
  }
  return v;
}

__device__ __forceinline__ void store_quad(uint8_t* p, const Bytes12& v, int count) {
  if (count == 4 && dword_aligned(p)) {
    *reinterpret_cast<Bytes12*>(p) = v;
  } else {
    for (int k = 0; k < count * 3; ++k) p[k] = (uint8_t)(v.w[k >> 2] >> ((k & 3) * 8));
  }
}

__device__ __forceinline__ uint32_t quad_byte(const Bytes12& v, int k) { return (v.w[k >> 2] >> ((k & 3) * 8)) & 255u; }
__device__ __forceinline__ void quad_set(Bytes12& v, int k, uint32_t b) { v.w[k >> 2] |= b << ((k & 3) * 8); }

// ---- photometric --------------------------------------------------------------------------------------------------
// an image is a flat list of P = H * W pixels: thread = (image, group of 4 pixels)
template <bool F32OUT>
__global__ __launch_bounds__(kThreads) void img_photo_kernel(const uint8_t* __restrict__ src,
                                                             const float* __restrict__ photo, void* __restrict__ dst,
                                                             int64_t P, int64_t quads, int64_t total) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= total) return;
  const int64_t i = t / quads, q = t - i * quads;
  const int64_t px = q * 4;
  const int count = (int)(P - px < 4 ? P - px : 4);
  const int64_t off = (i * P + px) * 3;
  const VidarImgPhoto par = vidar_img_photo_load(photo + i * VIDAR_IMG_PHOTO_STRIDE);
  const Bytes12 in = load_quad(src + off, count);
  Bytes12 out;
  out.w[0] = out.w[1] = out.w[2] = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (j < count) {
      float b = (float)quad_byte(in, 3 * j), g = (float)quad_byte(in, 3 * j + 1), r = (float)quad_byte(in, 3 * j + 2);
      vidar_img_photometric(b, g, r, par);
      if (F32OUT) {
        float* o = (float*)dst + off + 3 * j;
        o[0] = b; o[1] = g; o[2] = r;
      } else {
        quad_set(out, 3 * j, vidar_img_cast_u8(b));
        quad_set(out, 3 * j + 1, vidar_img_cast_u8(g));
        quad_set(out, 3 * j + 2, vidar_img_cast_u8(r));
      }
    }
  }
  if (!F32OUT) store_quad((uint8_t*)dst + off, out, count);
}

// ---- PIL resample -------------------------------------------------------------------------------------------------
// table of an axis (int32, device): bounds [out, 2] = (first source index inside the crop window, tap count), then the
// coefficients [out, ksize].  Whatever the table holds, no access leaves the window: the tap count is clamped to ksize and
// the first index to [0, in - count].
struct Taps { int first, count; const int32_t* k; };

__device__ __forceinline__ Taps taps_of(const int32_t* __restrict__ tab, int out, int ksize, int in, int idx) {
  Taps t;
  int count = tab[2 * idx + 1];
  count = count < 0 ? 0 : (count > ksize ? ksize : count);
  count = count > in ? in : count;
  int first = tab[2 * idx];
  first = first < 0 ? 0 : (first > in - count ? in - count : first);
  t.first = first; t.count = count;
  t.k = tab + 2 * (int64_t)out + (int64_t)idx * ksize;
  return t;
}

// horizontal pass: src [n, H, W, 3] window (crop_x, crop_y, crop_w, rows) -> dst [n, rows, ow, 3]; thread = (image, row,
// group of 4 output columns); output column dx holds table entry ow - 1 - dx when `flip`
__global__ __launch_bounds__(kThreads) void img_resample_h_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                                  const int32_t* __restrict__ tab, int ksize, int H, int W,
                                                                  int crop_x, int crop_y, int crop_w, int rows, int ow,
                                                                  int flip, int quads, int64_t total) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= total) return;
  const int q = (int)(t % quads);
  const int64_t ry = t / quads;
  const int y = (int)(ry % rows);
  const int64_t i = ry / rows;
  const uint8_t* row = src + ((i * H + crop_y + y) * W + crop_x) * 3;
  const int dx0 = q * 4;
  const int count = ow - dx0 < 4 ? ow - dx0 : 4;
  Bytes12 out;
  out.w[0] = out.w[1] = out.w[2] = 0;
  for (int j = 0; j < count; ++j) {
    const int dx = dx0 + j;
    const Taps tp = taps_of(tab, ow, ksize, crop_w, flip ? ow - 1 - dx : dx);
    int32_t a0 = 1 << (VIDAR_IMG_PRECISION_BITS - 1), a1 = a0, a2 = a0;
    const uint8_t* p = row + (int64_t)tp.first * 3;
    for (int k = 0; k < tp.count; ++k) {
      const int32_t c = tp.k[k];
      a0 += (int32_t)p[3 * k] * c; a1 += (int32_t)p[3 * k + 1] * c; a2 += (int32_t)p[3 * k + 2] * c;
    }
    quad_set(out, 3 * j, vidar_img_clip8(a0));
    quad_set(out, 3 * j + 1, vidar_img_clip8(a1));
    quad_set(out, 3 * j + 2, vidar_img_clip8(a2));
  }
  store_quad(dst + ((i * rows + y) * ow + dx0) * 3, out, count);
}

// vertical pass, per byte column: src rows of `row_bytes` used bytes, `src_stride` bytes apart, image `src_image` bytes
// apart, starting `src_off` bytes into the image -> dst [n, oh, row_bytes]; thread = (image, output row, 4 bytes)
__global__ __launch_bounds__(kThreads) void img_resample_v_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                                  const int32_t* __restrict__ tab, int ksize, int in_rows,
                                                                  int oh, int row_bytes, int64_t src_stride,
                                                                  int64_t src_image, int64_t src_off, int groups,
                                                                  int64_t total) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= total) return;
  const int gq = (int)(t % groups);
  const int64_t ry = t / groups;
  const int y = (int)(ry % oh);
  const int64_t i = ry / oh;
  const int b0 = gq * 4;
  const int count = row_bytes - b0 < 4 ? row_bytes - b0 : 4;
  const Taps tp = taps_of(tab, oh, ksize, in_rows, y);
  const uint8_t* p = src + i * src_image + src_off + (int64_t)tp.first * src_stride + b0;
  int32_t a[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) a[j] = 1 << (VIDAR_IMG_PRECISION_BITS - 1);
  const bool fast = count == 4 && dword_aligned(p) && (src_stride & 3) == 0;
  for (int k = 0; k < tp.count; ++k) {
    const int32_t c = tp.k[k];
    const uint8_t* r = p + (int64_t)k * src_stride;
    if (fast) {
      const uint32_t w = *reinterpret_cast<const uint32_t*>(r);
#pragma unroll
      for (int j = 0; j < 4; ++j) a[j] += (int32_t)((w >> (8 * j)) & 255u) * c;
    } else {
      for (int j = 0; j < count; ++j) a[j] += (int32_t)r[j] * c;
    }
  }
  uint8_t* o = dst + (i * oh + y) * (int64_t)row_bytes + b0;
  if (count == 4 && dword_aligned(o)) {
    uint32_t w = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) w |= (uint32_t)vidar_img_clip8(a[j]) << (8 * j);
    *reinterpret_cast<uint32_t*>(o) = w;
  } else {
    for (int j = 0; j < count; ++j) o[j] = vidar_img_clip8(a[j]);
  }
}

// ---- normalise + (bilinear) + pad + HWC -> CHW -----------------------------------------------------------------------
// the normalised channels of one source pixel (already in OUTPUT channel order)
template <bool PHOTO>
__device__ __forceinline__ void tap3(float b, float g, float r, const VidarImgPhoto& par, const Norm3& nm, int to_rgb,
                                     float out[3]) {
  if (PHOTO) vidar_img_photometric(b, g, r, par);
  out[0] = vidar_img_normalise(to_rgb ? r : b, nm.mean[0], nm.stdv[0]);
  out[1] = vidar_img_normalise(g, nm.mean[1], nm.stdv[1]);
  out[2] = vidar_img_normalise(to_rgb ? b : r, nm.mean[2], nm.stdv[2]);
}

// thread = (image, padded output row, group of 4 padded output columns) -> three 16-byte stores
template <bool PHOTO, bool SCALED>
__global__ __launch_bounds__(kThreads) void img_normalise_kernel(const uint8_t* __restrict__ src,
                                                                 const float* __restrict__ photo, float* __restrict__ dst,
                                                                 int H, int W, int oh, int ow, int Hp, int Wp, Norm3 nm,
                                                                 int to_rgb, int quads, int64_t total) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= total) return;
  const int q = (int)(t % quads);
  const int64_t ry = t / quads;
  const int y = (int)(ry % Hp);
  const int64_t i = ry / Hp;
  const int x0 = q * 4;
  float v[3][4];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int j = 0; j < 4; ++j) v[c][j] = 0.0f;
  VidarImgPhoto par = {};
  if (PHOTO) par = vidar_img_photo_load(photo + i * VIDAR_IMG_PHOTO_STRIDE);
  const uint8_t* img = src + i * (int64_t)H * W * 3;
  if (y < oh && x0 < ow) {
    const int count = ow - x0 < 4 ? ow - x0 : 4;
    if (!SCALED) {
      const Bytes12 in = load_quad(img + ((int64_t)y * W + x0) * 3, count);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < count) {
          float o[3];
          tap3<PHOTO>((float)quad_byte(in, 3 * j), (float)quad_byte(in, 3 * j + 1), (float)quad_byte(in, 3 * j + 2), par, nm,
                      to_rgb, o);
          v[0][j] = o[0]; v[1][j] = o[1]; v[2][j] = o[2];
        }
      }
    } else {
      int y0, y1; float wy0, wy1;
      vidar_img_bilinear_src(y, H, oh, y0, y1, wy0, wy1);
      const uint8_t* r0 = img + (int64_t)y0 * W * 3;
      const uint8_t* r1 = img + (int64_t)y1 * W * 3;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < count) {
          int xa, xb; float wx0, wx1;
          vidar_img_bilinear_src(x0 + j, W, ow, xa, xb, wx0, wx1);
          float t00[3], t01[3], t10[3], t11[3];
          tap3<PHOTO>((float)r0[3 * xa], (float)r0[3 * xa + 1], (float)r0[3 * xa + 2], par, nm, to_rgb, t00);
          tap3<PHOTO>((float)r0[3 * xb], (float)r0[3 * xb + 1], (float)r0[3 * xb + 2], par, nm, to_rgb, t01);
          tap3<PHOTO>((float)r1[3 * xa], (float)r1[3 * xa + 1], (float)r1[3 * xa + 2], par, nm, to_rgb, t10);
          tap3<PHOTO>((float)r1[3 * xb], (float)r1[3 * xb + 1], (float)r1[3 * xb + 2], par, nm, to_rgb, t11);
#pragma unroll
          for (int c = 0; c < 3; ++c) v[c][j] = vidar_img_bilinear(t00[c], t01[c], t10[c], t11[c], wx0, wx1, wy0, wy1);
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float4* o = reinterpret_cast<float4*>(dst + ((i * 3 + c) * Hp + y) * (int64_t)Wp + x0);
    *o = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
  }
}

inline bool grid_for(int64_t total, unsigned* blocks) {
  const int64_t b = (total + kThreads - 1) / kThreads;
  if (b <= 0 || b > 0x7fffffffLL) return false;
  *blocks = (unsigned)b;
  return true;
}

// 2 * ceil(2 * max(in / out, 1)) + 1: the row length of an axis' coefficient table (PIL's ksize for the bicubic filter)
inline int bicubic_ksize(int in, int out) {
  double scale = (double)in / (double)out;
  if (scale < 1.0) scale = 1.0;
  return 2 * (int)ceil(2.0 * scale) + 1;
}

template <bool F32OUT>
int photometric(const uint8_t* src, const float* photo, void* dst, int n, int H, int W, void* stream) {
  VIDAR_ENTER();
  if (src == nullptr || photo == nullptr || dst == nullptr || n <= 0 || H <= 0 || W <= 0) return VIDAR_ERR_BAD_ARG;
  const int64_t P = (int64_t)H * W, quads = (P + 3) / 4, total = quads * n;
  unsigned blocks;
  if (!grid_for(total, &blocks)) return VIDAR_ERR_BAD_ARG;
  hipLaunchKernelGGL(img_photo_kernel<F32OUT>, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, src, photo, dst, P,
                     quads, total);
  return vidar_last_error();
}

}  // namespace

extern "C" {

int vidar_img_photometric_u8(const uint8_t* src, const float* photo, uint8_t* dst, int n, int H, int W, void* stream) {
  return photometric<false>(src, photo, dst, n, H, W, stream);
}

int vidar_img_photometric_f32(const uint8_t* src, const float* photo, float* dst, int n, int H, int W, void* stream) {
  return photometric<true>(src, photo, dst, n, H, W, stream);
}

size_t vidar_img_resample_workspace_bytes(int n, int crop_h, int out_w) {
  if (n <= 0 || crop_h <= 0 || out_w <= 0) return 0;
  return ((size_t)n * (size_t)crop_h * (size_t)out_w * 3 + 15) / 16 * 16;
}

int vidar_img_resample_u8(const uint8_t* src, uint8_t* dst, int n, int H, int W, int crop_x, int crop_y, int crop_w,
                          int crop_h, int out_w, int out_h, const int32_t* tab_x, int ksize_x, const int32_t* tab_y,
                          int ksize_y, int flip, void* workspace, size_t workspace_bytes, void* stream) {
  VIDAR_ENTER();
  if (src == nullptr || dst == nullptr || n <= 0 || H <= 0 || W <= 0 || crop_w <= 0 || crop_h <= 0 || out_w <= 0 ||
      out_h <= 0)
    return VIDAR_ERR_BAD_ARG;
  if (crop_x < 0 || crop_y < 0 || crop_x > W - crop_w || crop_y > H - crop_h) return VIDAR_ERR_BAD_ARG;
  if (tab_x == nullptr && tab_y == nullptr) return VIDAR_ERR_BAD_ARG;                  // nothing to do is not a call
  if (tab_x == nullptr && (out_w != crop_w || flip || ksize_x != 0)) return VIDAR_ERR_BAD_ARG;
  if (tab_y == nullptr && (out_h != crop_h || ksize_y != 0)) return VIDAR_ERR_BAD_ARG;
  if (tab_x != nullptr && ksize_x != bicubic_ksize(crop_w, out_w)) return VIDAR_ERR_BAD_ARG;
  if (tab_y != nullptr && ksize_y != bicubic_ksize(crop_h, out_h)) return VIDAR_ERR_BAD_ARG;
  const bool both = tab_x != nullptr && tab_y != nullptr;
  if (both && (workspace == nullptr || workspace_bytes < vidar_img_resample_workspace_bytes(n, crop_h, out_w)))
    return VIDAR_ERR_BAD_ARG;
  const hipStream_t st = (hipStream_t)stream;
  unsigned blocks;
  if (tab_x != nullptr) {
    uint8_t* hdst = both ? (uint8_t*)workspace : dst;
    const int quads = (out_w + 3) / 4;
    const int64_t total = (int64_t)n * crop_h * quads;
    if (!grid_for(total, &blocks)) return VIDAR_ERR_BAD_ARG;
    hipLaunchKernelGGL(img_resample_h_kernel, dim3(blocks), dim3(kThreads), 0, st, src, hdst, tab_x, ksize_x, H, W, crop_x,
                       crop_y, crop_w, crop_h, out_w, flip ? 1 : 0, quads, total);
  }
  if (tab_y != nullptr) {
    const int row_bytes = out_w * 3;
    const int groups = (row_bytes + 3) / 4;
    const int64_t total = (int64_t)n * out_h * groups;
    if (!grid_for(total, &blocks)) return VIDAR_ERR_BAD_ARG;
    const uint8_t* vsrc = both ? (const uint8_t*)workspace : src;
    const int64_t stride = both ? (int64_t)row_bytes : (int64_t)W * 3;
    const int64_t image = both ? (int64_t)crop_h * row_bytes : (int64_t)H * W * 3;
    const int64_t off = both ? 0 : ((int64_t)crop_y * W + crop_x) * 3;
    hipLaunchKernelGGL(img_resample_v_kernel, dim3(blocks), dim3(kThreads), 0, st, vsrc, dst, tab_y, ksize_y, crop_h, out_h,
                       row_bytes, stride, image, off, groups, total);
  }
  return vidar_last_error();
}

int vidar_img_normalise_f32(const uint8_t* src, const float* photo, float* dst, int n, int H, int W, int out_h, int out_w,
                            int Hp, int Wp, const float* mean, const float* stdv, int to_rgb, void* stream) {
  VIDAR_ENTER();
  if (src == nullptr || dst == nullptr || mean == nullptr || stdv == nullptr || n <= 0 || H <= 0 || W <= 0 || out_h <= 0 ||
      out_w <= 0)
    return VIDAR_ERR_BAD_ARG;
  if (Hp < out_h || Wp < out_w || (Wp & 3) != 0 || ((uintptr_t)dst & 15u) != 0) return VIDAR_ERR_BAD_ARG;
  Norm3 nm;
  for (int c = 0; c < 3; ++c) { nm.mean[c] = mean[c]; nm.stdv[c] = stdv[c]; }
  const int quads = Wp / 4;
  const int64_t total = (int64_t)n * Hp * quads;
  unsigned blocks;
  if (!grid_for(total, &blocks)) return VIDAR_ERR_BAD_ARG;
  const bool scaled = out_h != H || out_w != W;
  const hipStream_t st = (hipStream_t)stream;
#define VIDAR_IMG_NORM_LAUNCH(PH, SC)                                                                                     \
  hipLaunchKernelGGL((img_normalise_kernel<PH, SC>), dim3(blocks), dim3(kThreads), 0, st, src, photo, dst, H, W, out_h,   \
                     out_w, Hp, Wp, nm, to_rgb ? 1 : 0, quads, total)
  if (photo != nullptr) { if (scaled) VIDAR_IMG_NORM_LAUNCH(true, true); else VIDAR_IMG_NORM_LAUNCH(true, false); }
  else { if (scaled) VIDAR_IMG_NORM_LAUNCH(false, true); else VIDAR_IMG_NORM_LAUNCH(false, false); }
#undef VIDAR_IMG_NORM_LAUNCH
  return vidar_last_error();
}

}  // extern "C"
