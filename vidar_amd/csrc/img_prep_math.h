// Per-pixel arithmetic of the image pipeline (csrc/img_prep.hip), shared by the device kernels and a HOST build:
// the same text compiles with hipcc for gfx950 and with the host C++ compiler, so the CPU tests run the identical
// operation sequence (tests/test_img_prep_cpu.py compiles this header with -DVIDAR_IMG_PREP_HOST_BUILD).
//
// Every function is a chain of single, correctly rounded fp32 operations in the order numpy evaluates
// vidar_amd/data/augment.py (`_distort`, `bgr2hsv`, `hsv2bgr`) and reader.normalise_pad.  It MUST be compiled with
// -ffp-contract=off (a fused multiply-add rounds once where numpy rounds twice) and with correctly rounded fp32
// division (hipcc's default), otherwise the results are not bit-identical and the uint8 cast after the photometric
// stage turns a 1-ulp difference at an integer boundary into a different pixel.
#ifndef VIDAR_IMG_PREP_MATH_H_
#define VIDAR_IMG_PREP_MATH_H_
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define VIDAR_IMG_FN __host__ __device__ __forceinline__
#else
#define VIDAR_IMG_FN static inline
#endif

// per-image photometric parameters: VIDAR_IMG_PHOTO_STRIDE floats (include/vidar_hip.h)
//   [0] shift  [1] gain applied before the HSV stage  [2] saturation factor  [3] hue turn (degrees)
//   [4] gain applied after the HSV stage  [5] flags (bit per step, as a float)  [6..8] channel permutation
//   (out[c] = in[perm[c]])  [9..11] reserved
#define VIDAR_IMG_PHOTO_STRIDE 12
#define VIDAR_IMG_PHOTO_SHIFT 1
#define VIDAR_IMG_PHOTO_GAIN_FIRST 2
#define VIDAR_IMG_PHOTO_SAT 4
#define VIDAR_IMG_PHOTO_TURN 8
#define VIDAR_IMG_PHOTO_GAIN_LAST 16

#define VIDAR_IMG_PRECISION_BITS 22          // PIL's 8-bit resampler: 32 - 8 - 2 fractional bits per coefficient

struct VidarImgPhoto {
  float shift, gain_first, sat, turn, gain_last;
  int flags, perm[3];
};

VIDAR_IMG_FN VidarImgPhoto vidar_img_photo_load(const float* p) {
  VidarImgPhoto q;
  q.shift = p[0]; q.gain_first = p[1]; q.sat = p[2]; q.turn = p[3]; q.gain_last = p[4];
  q.flags = (int)p[5];
  for (int c = 0; c < 3; ++c) {
    const int k = (int)p[6 + c];
    q.perm[c] = k < 0 ? 0 : (k > 2 ? 2 : k);
  }
  return q;
}

VIDAR_IMG_FN float vidar_img_pick3(int k, float a0, float a1, float a2) { return k == 0 ? a0 : (k == 1 ? a1 : a2); }

// PhotoMetricDistortionMultiViewImage._distort on one BGR pixel, in place
VIDAR_IMG_FN void vidar_img_photometric(float& b, float& g, float& r, const VidarImgPhoto& q) {
  if (q.flags & VIDAR_IMG_PHOTO_SHIFT) { b = b + q.shift; g = g + q.shift; r = r + q.shift; }
  if (q.flags & VIDAR_IMG_PHOTO_GAIN_FIRST) { b = b * q.gain_first; g = g * q.gain_first; r = r * q.gain_first; }
  // bgr2hsv
  const float v = fmaxf(fmaxf(b, g), r);
  const float d = v - fminf(fminf(b, g), r);
  float s = v > 0.0f ? d / v : 0.0f;
  const float dd = d > 0.0f ? d : 1.0f;
  float h;
  if (v == r) h = (g - b) / dd;
  else if (v == g) h = 2.0f + (b - r) / dd;
  else h = 4.0f + (r - g) / dd;
  h = h * 60.0f;
  h = d > 0.0f ? h : 0.0f;
  h = h < 0.0f ? h + 360.0f : h;
  if (q.flags & VIDAR_IMG_PHOTO_SAT) s = s * q.sat;
  if (q.flags & VIDAR_IMG_PHOTO_TURN) {
    h = h + q.turn;
    if (h > 360.0f) h = h - 360.0f;
    if (h < 0.0f) h = h + 360.0f;
  }
  // hsv2bgr
  const float h6 = h / 60.0f;
  const float fl = floorf(h6);
  int i = (int)fl % 6;
  if (i < 0) i += 6;
  const float f = h6 - fl;
  const float p = v * (1.0f - s);
  const float qq = v * (1.0f - s * f);
  const float t = v * (1.0f - s * (1.0f - f));
  float rr, gg, bb;
  switch (i) {
    case 0: rr = v; gg = t; bb = p; break;
    case 1: rr = qq; gg = v; bb = p; break;
    case 2: rr = p; gg = v; bb = t; break;
    case 3: rr = p; gg = qq; bb = v; break;
    case 4: rr = t; gg = p; bb = v; break;
    default: rr = v; gg = p; bb = qq; break;
  }
  if (q.flags & VIDAR_IMG_PHOTO_GAIN_LAST) { bb = bb * q.gain_last; gg = gg * q.gain_last; rr = rr * q.gain_last; }
  b = vidar_img_pick3(q.perm[0], bb, gg, rr);
  g = vidar_img_pick3(q.perm[1], bb, gg, rr);
  r = vidar_img_pick3(q.perm[2], bb, gg, rr);
}

// THE float -> uint8 rule of the pipeline: truncate toward zero to int32, keep the low 8 bits
VIDAR_IMG_FN uint8_t vidar_img_cast_u8(float x) { return (uint8_t)((int32_t)x & 255); }

// one output value of PIL's 8-bit resampler: acc = sum pixel * k, started at 2^21
VIDAR_IMG_FN uint8_t vidar_img_clip8(int32_t acc) {
  const int32_t v = acc >> VIDAR_IMG_PRECISION_BITS;
  return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// NormalizeMultiviewImage: subtract, then divide
VIDAR_IMG_FN float vidar_img_normalise(float x, float mean, float stdv) { return (x - mean) / stdv; }

// torch's bilinear source index, align_corners=False: scale = float(in) / out, src = scale (dst + 0.5) - 0.5 >= 0.
// ONE rounding for the multiply-subtract (an explicit fmaf, which -ffp-contract=off leaves alone): torch's CPU kernel is
// built with contraction on and evaluates it that way; two roundings move the weights by up to 4e-6 at index ~80, which
// is 1e-3 on 8-bit pixel differences, against 1 ulp of the result with the fused form.
VIDAR_IMG_FN void vidar_img_bilinear_src(int dst, int in, int out, int& i0, int& i1, float& w0, float& w1) {
  const float scale = (float)in / (float)out;
  float src = fmaf(scale, (float)dst + 0.5f, -0.5f);
  if (src < 0.0f) src = 0.0f;
  i0 = (int)src;
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  w1 = src - (float)i0;
  w0 = 1.0f - w1;
}

// rows first, the two taps of a row inside: wy0 (wx0 v00 + wx1 v01) + wy1 (wx0 v10 + wx1 v11)
VIDAR_IMG_FN float vidar_img_bilinear(float v00, float v01, float v10, float v11, float wx0, float wx1, float wy0,
                                      float wy1) {
  return wy0 * (wx0 * v00 + wx1 * v01) + wy1 * (wx0 * v10 + wx1 * v11);
}

#ifdef VIDAR_IMG_PREP_HOST_BUILD
// Host loops over the functions above (CPU tests and tools only; the product never calls them).
extern "C" {

// src uint8 [n, hw, 3] BGR, photo [n, VIDAR_IMG_PHOTO_STRIDE] -> out_f32 [n, hw, 3] (may be NULL), out_u8 (may be NULL)
void vidar_img_host_photometric(const uint8_t* src, const float* photo, float* out_f32, uint8_t* out_u8, int n, long hw) {
  for (int i = 0; i < n; ++i) {
    const VidarImgPhoto q = vidar_img_photo_load(photo + (long)i * VIDAR_IMG_PHOTO_STRIDE);
    for (long k = 0; k < hw; ++k) {
      const long o = ((long)i * hw + k) * 3;
      float b = (float)src[o], g = (float)src[o + 1], r = (float)src[o + 2];
      vidar_img_photometric(b, g, r, q);
      if (out_f32) { out_f32[o] = b; out_f32[o + 1] = g; out_f32[o + 2] = r; }
      if (out_u8) { out_u8[o] = vidar_img_cast_u8(b); out_u8[o + 1] = vidar_img_cast_u8(g); out_u8[o + 2] = vidar_img_cast_u8(r); }
    }
  }
}

// src uint8 [H, W, 3] -> dst fp32 [3, oh, ow]: normalise (optional channel reversal first), bilinear when (oh, ow) != (H, W)
void vidar_img_host_normalise(const uint8_t* src, float* dst, int H, int W, int oh, int ow, const float* mean,
                              const float* stdv, int to_rgb) {
  for (int y = 0; y < oh; ++y) {
    int y0, y1; float wy0, wy1;
    vidar_img_bilinear_src(y, H, oh, y0, y1, wy0, wy1);
    for (int x = 0; x < ow; ++x) {
      int x0, x1; float wx0, wx1;
      vidar_img_bilinear_src(x, W, ow, x0, x1, wx0, wx1);
      for (int c = 0; c < 3; ++c) {
        const int cs = to_rgb ? 2 - c : c;
        float v;
        if (oh == H && ow == W) {
          v = vidar_img_normalise((float)src[((long)y * W + x) * 3 + cs], mean[c], stdv[c]);
        } else {
          const float v00 = vidar_img_normalise((float)src[((long)y0 * W + x0) * 3 + cs], mean[c], stdv[c]);
          const float v01 = vidar_img_normalise((float)src[((long)y0 * W + x1) * 3 + cs], mean[c], stdv[c]);
          const float v10 = vidar_img_normalise((float)src[((long)y1 * W + x0) * 3 + cs], mean[c], stdv[c]);
          const float v11 = vidar_img_normalise((float)src[((long)y1 * W + x1) * 3 + cs], mean[c], stdv[c]);
          v = vidar_img_bilinear(v00, v01, v10, v11, wx0, wx1, wy0, wy1);
        }
        dst[((long)c * oh + y) * ow + x] = v;
      }
    }
  }
}

}  // extern "C"
#endif  // VIDAR_IMG_PREP_HOST_BUILD
#endif  // VIDAR_IMG_PREP_MATH_H_
