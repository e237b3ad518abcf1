// Fused occupancy-volume ray-march kernels of the ViDAR head for gfx950.
//
// Replace the PyTorch op chains of projects/mmdet3d_plugin/bevformer/dense_heads/vidar_head_base.py:
//   ray_ce      : _get_grid_features (:420-509) + F.cross_entropy(label 0) (:586-592)
//   ray_gumbel  : _get_grid_features on the dense voxel rays (:594-630) +
//                 _custom_gumbel_softmax_distance (:754-773)
//   ray_argmax  : test-time decode in get_point_cloud_prediction (:697-731)
//   ray_dist    : the use_dist_loss branch (:575-585): _custom_gumbel_softmax_distance over the K + 1 logits
//                 {end point, K waypoints} of the GT rays
//   ray_argmax_cam : ray_argmax on rays that are a function of (frame, camera, pixel) and are never stored
//                 (cam_ray.h; no counterpart in the reference); cam_rays writes those rays out
//   ray_stats / ray_stats_cam : the two decodes with the softmax along the ray summarised next to the distance
//                 (peak probability, mean length, spread, entropy; no counterpart in the reference)
//   ray_occupancy / ray_occupancy_cam : the decode's softmax scattered back onto the voxels, mass at / beyond every
//                 waypoint (hit / free evidence of an occupancy grid; no counterpart in the reference)
//   sweep_evidence : the same evidence of a MEASURED sweep -- rays with known returns, no volume is read
//   point_occupancy / voxel_occupancy : the decode's softmax asked about one place on the ray -- the return lies at /
//                 beyond the ray's end point -- for listed end points and for one ray per voxel through its centre
//                 (occ_at_math.h; no scatter, no atomics)
// The reference materialises ~8 arrays of [rays, 513] floats per call (waypoints, lengths, masks,
// sampled logits, -inf masks, softmax); here one wave owns one ray, its 512 waypoints live in
// registers (8 per lane) and only O(1) values per ray ever reach HBM.
//
// Waypoint count K = ray_grid_num.  Every op's arithmetic is written once, as a `*_body<K512>` that the kernels
// instantiate in two forms:
//   K == 512        register-resident (the released configs): the kernels without a suffix.
//   1 <= K <= kKMax streamed (`*_any_kernel`): the wave walks the ray in passes of 64 waypoints (32 in the backward) and
//                   keeps O(1) state per lane.
// A forward body visits the waypoints twice (struct Waypoints): visit 1 finds the max logit (and the best perturbed
// logit, its index and length), visit 2 adds the exp sums (the "mass beyond the sample" needs pred_dist, known only
// after visit 1).  The register form samples in visit 1 and replays its 8 registers per lane in visit 2; the streamed
// form samples the logits AGAIN.  Waypoints k >= K are never sampled and never read noise.  Every lane adds its
// waypoints in the same order in both forms, so K = 512 through the streamed form gives the same bits
// (tests/test_ray_options_gpu.py; vidar_ray_force_streamed).
//   kKMax = 65536: nothing in the streamed kernels depends on K but the trip count ((k + 0.5f) is exact in fp32 far past
//   it, noise offsets are size_t); the bound only keeps a corrupt argument from becoming a minutes-long launch.  The
//   longest ray of the 200 x 200 x 16 volume is its 283-voxel diagonal = 2264 waypoints at step 0.125.
//
// Geometry (voxel units, fp32, same operation order as the reference):
//   rhat = (p - o)/|p - o| ;  s_k = o + rhat * (k + 0.5) * step, k = 0..K-1 (K = ray_grid_num)
//   normalised g = s / (X,Y,Z) * 2 - 1 ; a waypoint is masked (-inf) iff any g <= -1 or g >= 1
//   trilinear sample of sigma[Z,Y,X] at pixel ((g+1)*size-1)/2, zero padding, align_corners=False.
// sigma layout: [F, Z, Y, X] f32 (x fastest) -- the head's own [bs,F,16,200,200] view.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <atomic>

#include "vidar_hip.h"
#include "vidar_common.h"
#include "scatter_copies.h"
#include "det_scatter.h"
#include "cam_ray.h"
#include "occ_score_math.h"
#include "occ_at_math.h"

namespace {

constexpr int kWave = 64;
constexpr int kPerLane = 8;           // K = 512 waypoints
constexpr int kK = kWave * kPerLane;
constexpr int kKMax = 65536;
constexpr int kThreads = 256;
constexpr int kRaysPerBlock = kThreads / kWave;

struct VolDims { int F, Z, Y, X; };

struct Ray {
  float ox, oy, oz, dx, dy, dz;   // origin, unit direction
  float px, py, pz;               // target point
  int f;                          // frame slot, -1 = skip
};

// Where a kernel's rays come from: the ray-source policy of load_ray.  Either source hands over a frame slot, an fp32
// origin and an fp32 end point; the unit direction is derived from those two in one place (aim), so a ray read from a
// list and the same ray generated from its pixel march with the same bits.
// kTarget: the end point is a measured target -- the decode also reports |p - o|, and a ray without a live waypoint keeps
// the reference's answer (torch.max over all -inf picks waypoint 0).  A camera ray's end point is only the point at
// depth 1: nothing to report, and a ray without a live waypoint gives 0, "no return".
struct ListedRays {       // origin [F,3], pts [R,3], tindex [R]: every op of the head
  static constexpr bool kTarget = true;
  const float* __restrict__ origin;
  const float* __restrict__ pts;
  const float* __restrict__ tindex;
};
struct CameraRays {       // ray r = pixel (f, c, y, x) of [F, C, Hs, Ws] through pix2vox [F,C,4,4] (cam_ray.h)
  static constexpr bool kTarget = false;
  const float* __restrict__ pix2vox;
  vidar_cam::CamGrid g;
};
struct VoxelRays {        // ray r = voxel (f, z, y, x) of the volume itself, x fastest: from origin[f] through the voxel's
  const float* __restrict__ origin;   // centre (x + 0.5, y + 0.5, z + 0.5), exact in fp32.  No kTarget: only
};                                    // point_occupancy_body marches these, and it reports no distance

__device__ __forceinline__ void aim(Ray& ray) {
  const float rx = ray.px - ray.ox, ry = ray.py - ray.oy, rz = ray.pz - ray.oz;
  const float n = sqrtf(rx * rx + ry * ry + rz * rz);
  ray.dx = rx / n; ray.dy = ry / n; ray.dz = rz / n;
}

__device__ __forceinline__ Ray load_ray(const ListedRays& s, int r, const VolDims& v) {
  Ray ray;
  const float t = s.tindex[r];
  ray.f = (t >= 0.f && t < (float)v.F) ? (int)t : -1;   // NaN / -1 padding -> skip
  const int f = ray.f < 0 ? 0 : ray.f;
  ray.ox = s.origin[f * 3 + 0]; ray.oy = s.origin[f * 3 + 1]; ray.oz = s.origin[f * 3 + 2];
  ray.px = s.pts[(size_t)r * 3 + 0]; ray.py = s.pts[(size_t)r * 3 + 1]; ray.pz = s.pts[(size_t)r * 3 + 2];
  aim(ray);
  return ray;
}
__device__ __forceinline__ Ray load_ray(const CameraRays& s, int r, const VolDims&) {
  int fc, x, y;
  Ray ray;
  vidar_cam::split_ray_index(r, s.g, ray.f, fc, x, y);
  const vidar_cam::CamRay c = vidar_cam::pixel_ray(s.pix2vox + (size_t)fc * 16, s.g, x, y);
  ray.ox = c.ox; ray.oy = c.oy; ray.oz = c.oz;
  ray.px = c.px; ray.py = c.py; ray.pz = c.pz;
  aim(ray);
  return ray;
}
__device__ __forceinline__ Ray load_ray(const VoxelRays& s, int r, const VolDims& v) {
  Ray ray;
  const int x = r % v.X, zy = r / v.X, y = zy % v.Y, fz = zy / v.Y, z = fz % v.Z;
  ray.f = fz / v.Z;
  ray.ox = s.origin[ray.f * 3 + 0]; ray.oy = s.origin[ray.f * 3 + 1]; ray.oz = s.origin[ray.f * 3 + 2];
  ray.px = x + 0.5f; ray.py = y + 0.5f; ray.pz = z + 0.5f;
  aim(ray);
  return ray;
}
__device__ __forceinline__ Ray load_ray(const float* __restrict__ origin, const float* __restrict__ pts,
                                        const float* __restrict__ tindex, int r, const VolDims& v) {
  return load_ray(ListedRays{origin, pts, tindex}, r, v);
}

struct Tri {
  int o[8];      // linear voxel offsets or -1
  float w[8];
  bool masked;   // waypoint outside the open volume -> logit -inf
};

template <bool USE_MASK = true>
__device__ __forceinline__ Tri make_tri(float sx, float sy, float sz, const VolDims& v) {
  Tri t;
  const float gx = sx / v.X * 2.f - 1.f, gy = sy / v.Y * 2.f - 1.f, gz = sz / v.Z * 2.f - 1.f;
  t.masked = USE_MASK && ((gx <= -1.f) || (gx >= 1.f) || (gy <= -1.f) || (gy >= 1.f) ||
                          (gz <= -1.f) || (gz >= 1.f) || (gx != gx) || (gy != gy) || (gz != gz));
  const float ix = ((gx + 1.f) * v.X - 1.f) / 2.f;
  const float iy = ((gy + 1.f) * v.Y - 1.f) / 2.f;
  const float iz = ((gz + 1.f) * v.Z - 1.f) / 2.f;
  const float fx = floorf(ix), fy = floorf(iy), fz = floorf(iz);
  const int x0 = (int)fx, y0 = (int)fy, z0 = (int)fz;
  const float ax = ix - fx, ay = iy - fy, az = iz - fz;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int cx = c & 1, cy = (c >> 1) & 1, cz = c >> 2;
    const int x = x0 + cx, y = y0 + cy, z = z0 + cz;
    const bool ok = !t.masked && x >= 0 && x < v.X && y >= 0 && y < v.Y && z >= 0 && z < v.Z;
    t.o[c] = ok ? (z * v.Y + y) * v.X + x : -1;
    t.w[c] = (cx ? ax : 1.f - ax) * (cy ? ay : 1.f - ay) * (cz ? az : 1.f - az);
  }
  return t;
}

__device__ __forceinline__ float tri_load(const float* __restrict__ vol, const Tri& t) {
  float acc = 0.f;
#pragma unroll
  for (int c = 0; c < 8; ++c)
    if (t.o[c] >= 0) acc += t.w[c] * vol[t.o[c]];
  return acc;
}
// `acc`: the accumulate policy of det_acc.h (fp32 atomic / measure / fixed point)
template <class Acc>
__device__ __forceinline__ void tri_scatter(float* __restrict__ gvol, const Tri& t, float g, Acc& acc) {
  if (g == 0.f) return;
#pragma unroll
  for (int c = 0; c < 8; ++c)
    if (t.o[c] >= 0) acc.add(gvol + t.o[c], t.w[c] * g);
}
// the four corners with x-corner `cx` only.  fp32 global atomics cost per (instruction x 128-byte line touched)
// (tools/micro/atomic_bench.hip): the backward kernels pair adjacent lanes on ONE waypoint -- even lane x0, odd lane
// x0 + 1, neighbouring addresses of the x-fastest volume -- so an atomic instruction of 32 waypoints touches the lines
// of 32 corners instead of 64: half the requests of a lane-per-waypoint scatter for the same 8 adds per waypoint.
template <class Acc>
__device__ __forceinline__ void tri_scatter_x(float* __restrict__ gvol, const Tri& t, float g, int cx, Acc& acc) {
  if (g == 0.f) return;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int o = cx ? t.o[2 * c + 1] : t.o[2 * c];
    const float w = cx ? t.w[2 * c + 1] : t.w[2 * c];
    if (o >= 0) acc.add(gvol + o, w * g);
  }
}

__device__ __forceinline__ void waypoint(const Ray& r, int k, float step, float& sx, float& sy,
                                         float& sz) {
  const float d = (k + 0.5f) * step;
  sx = r.ox + r.dx * d; sy = r.oy + r.dy * d; sz = r.oz + r.dz * d;
}
__device__ __forceinline__ float dist_to(const Ray& r, float sx, float sy, float sz) {
  const float ex = sx - r.ox, ey = sy - r.oy, ez = sz - r.oz;
  return sqrtf(ex * ex + ey * ey + ez * ez);
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, kWave));
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, kWave);
  return v;
}

constexpr float kNegInf = -__builtin_inff();

// running (value, index, length) arg-max; the first index wins ties, like torch.max
// kNoIndex only has to be larger than every index any form can produce: it is never used but in `k < i`
constexpr int kNoIndex = 0x7fffffff;
struct Best {
  float v = kNegInf;
  int i = kNoIndex;
  float len = 0.f;
  __device__ __forceinline__ void take(float z, int k, float l) {
    if (z > v || (z == v && k < i)) { v = z; i = k; len = l; }
  }
};
__device__ __forceinline__ void wave_argmax(Best& b) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1)
    b.take(__shfl_xor(b.v, s, kWave), __shfl_xor(b.i, s, kWave), __shfl_xor(b.len, s, kWave));
}

// The K waypoints of one ray as the forward bodies walk them: every lane visits its waypoints k = lane, lane + 64, ...
// TWICE, in that order in both forms (which is what makes their sums the same bits).
//   K512 (K == kK): the first visit samples logit and length into 8 registers per lane, the second replays them;
//   streamed:       both visits sample; waypoints k >= K are never sampled.
// MASKED: the training ops' sampler (outside the open volume -> -inf); otherwise the decode's: plain zero padding, and
// an exact zero -- outside, or a zero of the volume -- counts as -inf (vidar_head_base.py:728).
template <bool K512, bool MASKED>
struct Waypoints {
  const float* vol;
  const Ray& ray;
  const VolDims& v;
  float step;
  int lane, K;
  float f[K512 ? kPerLane : 1], len[K512 ? kPerLane : 1];

  __device__ __forceinline__ void sample(int k, float& logit, float& length) const {
    float sx, sy, sz;
    waypoint(ray, k, step, sx, sy, sz);
    const Tri t = make_tri<MASKED>(sx, sy, sz, v);
    length = dist_to(ray, sx, sy, sz);
    if (MASKED) {
      logit = t.masked ? kNegInf : tri_load(vol, t);
    } else {
      const float val = (sx == sx) ? tri_load(vol, t) : 0.f;
      logit = (val == 0.f) ? kNegInf : val;
    }
  }
  // fn(k, logit, length)
  template <class Fn>
  __device__ __forceinline__ void first(Fn fn) {
    if (K512) {
#pragma unroll
      for (int j = 0; j < kPerLane; ++j) {
        sample(lane + j * kWave, f[j], len[j]);
        fn(lane + j * kWave, f[j], len[j]);
      }
    } else {
      for (int k = lane; k < K; k += kWave) {
        sample(k, f[0], len[0]);
        fn(k, f[0], len[0]);
      }
    }
  }
  template <class Fn>
  __device__ __forceinline__ void second(Fn fn) {
    if (K512) {
#pragma unroll
      for (int j = 0; j < kPerLane; ++j) fn(lane + j * kWave, f[j], len[j]);
    } else {
      first(fn);
    }
  }
  // A further visit in passes of 64 consecutive waypoints (k = 64 j + lane, one per lane: the layout of the registers)
  // from the LAST pass to the first: fn(k, logit).  Every lane runs every pass -- a lane with k >= K gets -inf, never
  // sampled -- so fn may hold cross-lane operations.
  template <class Fn>
  __device__ __forceinline__ void passes_down(Fn fn) const {
    if (K512) {
#pragma unroll
      for (int j = kPerLane - 1; j >= 0; --j) fn(lane + j * kWave, f[j]);
    } else {
      for (int j = (K + kWave - 1) / kWave - 1; j >= 0; --j) {
        const int k = lane + j * kWave;
        float z = kNegInf, l;
        if (k < K) sample(k, z, l);
        fn(k, z);
      }
    }
  }
};

// END_POINT, in the bodies below: the ray's end point is an entry of its own in front of the K waypoints (lane 0 carries
// it), and rays whose end point leaves the open volume are dropped (:464-467).  ray_ce and ray_dist; ray_gumbel and
// ray_argmax see the waypoints only and drop no ray.

// ---------------------------------------------------------------------------------------------
// GT-ray march + cross entropy on the end-point sample
// ---------------------------------------------------------------------------------------------
template <bool K512>
__device__ __forceinline__ void ray_ce_fwd_body(
    const float* __restrict__ sigma, const float* __restrict__ origin, const float* __restrict__ gt,
    const float* __restrict__ tindex, float* __restrict__ ce, float* __restrict__ lse_out,
    float* __restrict__ valid, int R, VolDims v, float step, int K) {
  const int r = blockIdx.x * kRaysPerBlock + threadIdx.x / kWave;
  if (r >= R) return;
  const int lane = threadIdx.x % kWave;
  const Ray ray = load_ray(origin, gt, tindex, r, v);
  const Tri t0 = make_tri(ray.px, ray.py, ray.pz, v);
  const bool ok = ray.f >= 0 && !t0.masked;
  float out_ce = 0.f, out_lse = 0.f;
  if (ok) {
    const float* vol = sigma + (size_t)ray.f * v.Z * v.Y * v.X;
    const float f0 = tri_load(vol, t0);
    Waypoints<K512, true> w{vol, ray, v, step, lane, K};
    float m = f0;
    w.first([&](int, float f, float) { m = fmaxf(m, f); });
    m = wave_max(m);
    float s = (lane == 0) ? expf(f0 - m) : 0.f;
    w.second([&](int, float f, float) { s += expf(f - m); });   // exp(-inf) == 0
    s = wave_sum(s);
    out_lse = m + logf(s);
    out_ce = out_lse - f0;
  }
  if (lane == 0) {
    ce[r] = out_ce; lse_out[r] = out_lse; valid[r] = ok ? 1.f : 0.f;
  }
}

// ---------------------------------------------------------------------------------------------
// hard gumbel sample of the hit entry + straight-through "mass beyond" factor (_custom_gumbel_softmax_distance)
//   ray_gumbel: the K waypoints of the dense rays, noise [R, K]
//   ray_dist:   the K + 1 entries {end point, K waypoints} of the GT rays (use_dist_loss, :575-585), noise [R, K + 1] in
//               that order; entry 0 is the sample AT the end point with length |p - o|; also gt_len[r], valid[r]
// aux[r] = {pred_dist, prob_next, lse}
// ---------------------------------------------------------------------------------------------
template <bool K512, bool END_POINT>
__device__ __forceinline__ void ray_sample_fwd_body(
    const float* __restrict__ sigma, const float* __restrict__ origin, const float* __restrict__ pts,
    const float* __restrict__ tindex, const float* __restrict__ noise, float* __restrict__ dist,
    float* __restrict__ gt_len, float* __restrict__ aux, float* __restrict__ valid, int R, VolDims v, float step,
    int K) {
  const int r = blockIdx.x * kRaysPerBlock + threadIdx.x / kWave;
  if (r >= R) return;
  const int lane = threadIdx.x % kWave;
  const Ray ray = load_ray(origin, pts, tindex, r, v);
  const Tri t0 = make_tri(ray.px, ray.py, ray.pz, v);
  const bool ok = ray.f >= 0 && !(END_POINT && t0.masked);
  float o_dist = 0.f, o_len = 0.f, o_pd = 0.f, o_pn = 0.f, o_lse = 0.f;
  if (ok) {
    const float* vol = sigma + (size_t)ray.f * v.Z * v.Y * v.X;
    const float* nz = noise + (size_t)r * ((size_t)K + END_POINT);
    Waypoints<K512, true> w{vol, ray, v, step, lane, K};
    // arg-max of logits + gumbel noise
    Best best;
    float m = kNegInf, f0 = 0.f, len0 = 0.f;
    if (END_POINT) {
      m = f0 = tri_load(vol, t0);
      len0 = dist_to(ray, ray.px, ray.py, ray.pz);
      if (lane == 0) best = Best{f0 + nz[0], 0, len0};
    }
    w.first([&](int k, float f, float len) {
      best.take(f + nz[k + END_POINT], k + END_POINT, len);
      m = fmaxf(m, f);
    });
    wave_argmax(best);
    m = wave_max(m);
    const float pd = best.len;
    const float e0 = (END_POINT && lane == 0) ? expf(f0 - m) : 0.f;
    float se = e0, sn = (len0 > pd) ? e0 : 0.f;
    w.second([&](int, float f, float len) {
      const float e = expf(f - m);
      se += e;
      sn += (len > pd) ? e : 0.f;
    });
    se = wave_sum(se); sn = wave_sum(sn);
    const float pn = sn / se;
    o_pd = pd; o_pn = pn; o_lse = m + logf(se); o_len = len0;
    o_dist = ((1.f - pn) + pn) * pd;
  }
  if (lane == 0) {
    dist[r] = o_dist;
    aux[(size_t)r * 3 + 0] = o_pd; aux[(size_t)r * 3 + 1] = o_pn; aux[(size_t)r * 3 + 2] = o_lse;
    if (END_POINT) { gt_len[r] = o_len; valid[r] = ok ? 1.f : 0.f; }
  }
}

// test-time decode (:697-731): arg-max waypoint -> distance.  `src` is the ray source: the listed rays of the head's
// decode, or a camera grid (gt_dist is not touched; see kTarget).
template <bool K512, class Src>
__device__ __forceinline__ void ray_argmax_body(
    const float* __restrict__ sigma, const Src& src, float* __restrict__ pred_dist, float* __restrict__ gt_dist,
    int R, VolDims v, float step, int K) {
  const int r = blockIdx.x * kRaysPerBlock + threadIdx.x / kWave;
  if (r >= R) return;
  const int lane = threadIdx.x % kWave;
  const Ray ray = load_ray(src, r, v);
  float o_pred = 0.f, o_gt = 0.f;
  if (ray.f >= 0) {
    Waypoints<K512, false> w{sigma + (size_t)ray.f * v.Z * v.Y * v.X, ray, v, step, lane, K};
    Best best;
    w.first([&](int k, float z, float len) { best.take(z, k, len); });
    wave_argmax(best);
    o_pred = (!Src::kTarget && best.v == kNegInf) ? 0.f : best.len;
    o_gt = dist_to(ray, ray.px, ray.py, ray.pz);
  }
  if (lane == 0) {
    pred_dist[r] = o_pred;
    if (Src::kTarget) gt_dist[r] = o_gt;
  }
}

// The decode with its confidence: ray_argmax_body's first visit, then a second one over the softmax of the ray's live
// waypoints (live = logit not -inf).  With m = max logit (the arg-max's own logit: no noise here, so Best carries it),
// e_k = exp(z_k - m), S = sum e_k and d = the decoded length, stats[r] = {p_max, mean, rms, entropy}:
//   p_max = exp(z_argmax - m) / S = 1 / S        mean = d + sum e_k (l_k - d) / S
//   rms = sqrt(sum e_k (l_k - d)^2 / S)          entropy = log S - sum e_k (z_k - m) / S   (nats)
// The lengths enter as deviations from d: the mass sits near d, so the sums stay small next to l_k and the spread needs
// no difference of two large sums.  A dead waypoint is skipped altogether (no 0 * -inf, no 0 * NaN length); a skipped
// ray and a ray without a live waypoint give four zeros; the distances are ray_argmax_body's, bit for bit.
// +inf / NaN logits may give non-finite statistics.
template <bool K512, class Src>
__device__ __forceinline__ void ray_stats_body(
    const float* __restrict__ sigma, const Src& src, float* __restrict__ pred_dist, float* __restrict__ gt_dist,
    float* __restrict__ stats, int R, VolDims v, float step, int K) {
  const int r = blockIdx.x * kRaysPerBlock + threadIdx.x / kWave;
  if (r >= R) return;
  const int lane = threadIdx.x % kWave;
  const Ray ray = load_ray(src, r, v);
  float o_pred = 0.f, o_gt = 0.f;
  float4 o_st = make_float4(0.f, 0.f, 0.f, 0.f);
  if (ray.f >= 0) {
    Waypoints<K512, false> w{sigma + (size_t)ray.f * v.Z * v.Y * v.X, ray, v, step, lane, K};
    Best best;
    w.first([&](int k, float z, float len) { best.take(z, k, len); });
    wave_argmax(best);
    const bool live = best.v != kNegInf;                 // the same in every lane
    o_pred = (!Src::kTarget && !live) ? 0.f : best.len;
    o_gt = dist_to(ray, ray.px, ray.py, ray.pz);
    if (live) {
      const float m = best.v, d = best.len;
      float se = 0.f, s1 = 0.f, s2 = 0.f, sz = 0.f;
      w.second([&](int, float z, float len) {
        if (z == kNegInf) return;
        const float e = expf(z - m), dl = len - d;
        se += e;
        s1 += e * dl;
        s2 += e * dl * dl;
        sz += e * (z - m);
      });
      se = wave_sum(se); s1 = wave_sum(s1); s2 = wave_sum(s2); sz = wave_sum(sz);
      o_st = make_float4(1.f / se, d + s1 / se, sqrtf(s2 / se), logf(se) - sz / se);
    }
  }
  if (lane == 0) {
    pred_dist[r] = o_pred;
    if (Src::kTarget) gt_dist[r] = o_gt;
    reinterpret_cast<float4*>(stats)[r] = o_st;
  }
}

// The occupancy query: the softmax of ray_stats_body (visits 1 and 2, live as there) asked about the ray's END POINT q.
// With L = |q - o| (dist_to: the length aim divides by) and the weights of occ_at_math.h -- waypoint k owns
// [k step, (k + 1) step) of the ray, the query [L - extent/2, L + extent/2] --
//   hit = sum p_k w_hit(k)        the return lies in the query's stretch
//   free = sum p_k w_free(k)      the return lies beyond it: the ray passed the query
// both sums of non-negative terms, hit + free <= 1.  The two answers of ray r go to hit[r * stride] and free_[r * stride]:
// stride 2 with free_ = hit + 1 is the listed form's [R,2], stride 1 the per-voxel form's two grids.  A skipped ray and a
// ray without a live waypoint (q == o: the direction is NaN and every waypoint dead) give two zeros.  No atomics, no
// workspace; +inf / NaN logits may give non-finite output.
template <bool K512, class Src>
__device__ __forceinline__ void point_occupancy_body(
    const float* __restrict__ sigma, const Src& src, float* __restrict__ hit, float* __restrict__ free_, int stride,
    int R, VolDims v, float step, float extent, int K) {
  const int r = blockIdx.x * kRaysPerBlock + threadIdx.x / kWave;
  if (r >= R) return;
  const int lane = threadIdx.x % kWave;
  const Ray ray = load_ray(src, r, v);
  float o_hit = 0.f, o_free = 0.f;
  if (ray.f >= 0) {
    Waypoints<K512, false> w{sigma + (size_t)ray.f * v.Z * v.Y * v.X, ray, v, step, lane, K};
    float m = kNegInf;
    w.first([&](int, float z, float) { m = fmaxf(m, z); });
    m = wave_max(m);
    if (m != kNegInf) {                                    // a live waypoint; the same in every lane
      const float L = dist_to(ray, ray.px, ray.py, ray.pz);
      float se = 0.f, sh = 0.f, sf = 0.f;
      w.second([&](int k, float z, float) {
        if (z == kNegInf) return;
        const float e = expf(z - m);
        const vidar_occ_at::Weights c = vidar_occ_at::weights(L, extent, k, step);
        se += e;
        sh += e * c.hit;
        sf += e * c.free;
      });
      se = wave_sum(se); sh = wave_sum(sh); sf = wave_sum(sf);
      o_hit = sh / se; o_free = sf / se;
    }
  }
  if (lane == 0) {
    hit[(size_t)r * stride] = o_hit;
    free_[(size_t)r * stride] = o_free;
  }
}

// ---------------------------------------------------------------------------------------------
// The backwards: d loss / d logit of every live entry, scattered through the entry's trilinear weights.
// A Coef is built from what the forward saved for ray r and gives g * d loss_r / d logit of an entry with softmax
// probability p = exp(logit - lse) and length len; `target` marks the cross-entropy label (the end point).
// ---------------------------------------------------------------------------------------------
struct CeCoef {       // saved: lse [R]
  float lse;
  __device__ __forceinline__ CeCoef(const float* __restrict__ saved, int r) : lse(saved[r]) {}
  __device__ __forceinline__ float operator()(float g, float p, float, bool target) const {
    return target ? g * (p - 1.f) : g * p;
  }
};
struct SampleCoef {   // saved: aux [R, 3]; d dist / d logit = pd * p * (ind - pn) on every entry, the end point included
  float pd, pn, lse;
  __device__ __forceinline__ SampleCoef(const float* __restrict__ saved, int r)
      : pd(saved[(size_t)r * 3 + 0]), pn(saved[(size_t)r * 3 + 1]), lse(saved[(size_t)r * 3 + 2]) {}
  __device__ __forceinline__ float operator()(float g, float p, float len, bool) const {
    const float ind = len > pd ? 1.f : 0.f;
    return g * pd * p * (ind - pn);
  }
};

// K512: the fixed 16 passes of the register form's K; otherwise ceil(K / 32) passes with a tail predicate.
// The adds go into private copies of the volume (scatter_copies.h).  (Leaving the 512-waypoint loop after the run of
// live waypoints -- the waypoints inside the volume are ONE run of consecutive k, tests/test_ray_early_exit_cpu.py --
// was measured too: no change, the masked passes cost almost nothing next to the atomics; removed.)
// (Acc: the accumulate policy of det_acc.h; the early `return`s are held to the contract at its AccMeasure::flush.)
template <bool K512, bool END_POINT, class Coef, class Acc>
__device__ __forceinline__ void ray_bwd_body(
    const float* __restrict__ sigma, const float* __restrict__ origin, const float* __restrict__ pts,
    const float* __restrict__ tindex, const float* __restrict__ saved, const float* __restrict__ grad,
    float* __restrict__ grad_sigma, int R, VolDims v, float step, int ncopies, int K, Acc& acc) {
  const int r = blockIdx.x * kRaysPerBlock + threadIdx.x / kWave;
  if (r >= R) return;
  const int lane = threadIdx.x % kWave;
  const float g = grad[r];
  if (g == 0.f) return;
  const Ray ray = load_ray(origin, pts, tindex, r, v);
  const Tri t0 = make_tri(ray.px, ray.py, ray.pz, v);
  if (ray.f < 0 || (END_POINT && t0.masked)) return;
  const size_t slice = (size_t)ray.f * v.Z * v.Y * v.X;
  const float* vol = sigma + slice;
  float* gvol = grad_sigma + scatter_copy_of_block(ncopies) * v.F * v.Z * v.Y * v.X + slice;
  const Coef coef(saved, r);
  if (END_POINT && lane == 0)
    tri_scatter(gvol, t0, coef(g, expf(tri_load(vol, t0) - coef.lse), dist_to(ray, ray.px, ray.py, ray.pz), true), acc);
  const int cx = lane & 1;
  const int passes = K512 ? 2 * kPerLane : (K + kWave / 2 - 1) / (kWave / 2);
  for (int j = 0; j < passes; ++j) {                   // 32 waypoints per pass, a lane pair per waypoint
    const int k = (lane >> 1) + j * (kWave / 2);
    if (!K512 && k >= K) break;                        // only in the last pass
    float sx, sy, sz;
    waypoint(ray, k, step, sx, sy, sz);
    const Tri t = make_tri(sx, sy, sz, v);
    if (t.masked) continue;
    tri_scatter_x(gvol, t, coef(g, expf(tri_load(vol, t) - coef.lse), dist_to(ray, sx, sy, sz), false), cx, acc);
  }
}

// ---------------------------------------------------------------------------------------------
// Occupancy evidence: the decode's softmax, scattered back onto the voxels it was read from (an inverse sensor model).
// Over the live waypoints of a ray (live as in ray_stats_body), with m = max z_k, e_k = exp(z_k - m), S = sum e_k:
//   p_k = e_k / S            the return lies at k          hit [f, corner c of k] += p_k * w_kc
//   b_k = sum_{j>k} p_j      the ray passed k              free[f, corner c of k] += b_k * w_kc
// w_kc: the trilinear weights the logit was sampled with; corners outside the volume are dropped, as the zero padding
// dropped them from the sample.  A dead waypoint, a skipped ray and a ray without a live waypoint add nothing.
// Visit 1 / 2 find m and S as ray_stats_body does; the third visit (Waypoints::passes_down) walks the passes of 64
// consecutive waypoints from the far end: b of a pass is the wave's exclusive suffix sum of p plus the carry of the later
// passes -- a sum of non-negative terms, never 1 - prefix, so b >= 0 and the last live waypoint has b == 0 exactly.
// The scatter is the backwards': a lane pair per waypoint (two half-passes of 32), the private copies, the Acc policy.
// ---------------------------------------------------------------------------------------------
// exclusive suffix sum over the wave: lane l gets v[l+1] + ... + v[63], lane 63 gets 0
__device__ __forceinline__ float wave_suffix_excl(float v, int lane) {
  float s = __shfl_down(v, 1, kWave);
  if (lane == kWave - 1) s = 0.f;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const float t = __shfl_down(s, d, kWave);
    if (lane + d < kWave) s += t;
  }
  return s;
}

template <bool K512, class Src, class Acc>
__device__ __forceinline__ void ray_occupancy_body(
    const float* __restrict__ sigma, const Src& src, float* __restrict__ hit, float* __restrict__ free_, int R,
    VolDims v, float step, int ncopies, int K, Acc& acc_hit, Acc& acc_free) {
  const int r = blockIdx.x * kRaysPerBlock + threadIdx.x / kWave;
  if (r >= R) return;
  const int lane = threadIdx.x % kWave;
  const Ray ray = load_ray(src, r, v);
  if (ray.f < 0) return;
  const size_t slice = (size_t)ray.f * v.Z * v.Y * v.X;
  Waypoints<K512, false> w{sigma + slice, ray, v, step, lane, K};
  float m = kNegInf;
  w.first([&](int, float z, float) { m = fmaxf(m, z); });
  m = wave_max(m);
  if (m == kNegInf) return;                              // no live waypoint; the same in every lane
  float se = 0.f;
  w.second([&](int, float z, float) { if (z != kNegInf) se += expf(z - m); });
  se = wave_sum(se);
  const size_t copy = scatter_copy_of_block(ncopies) * v.F * v.Z * v.Y * v.X + slice;
  float* hvol = hit + copy;
  float* fvol = free_ + copy;
  const int cx = lane & 1;
  float carry = 0.f;                                     // mass of the later passes
  w.passes_down([&](int k, float z) {
    const bool live = z != kNegInf;
    const float p = live ? expf(z - m) / se : 0.f;
    const float beyond = wave_suffix_excl(p, lane) + carry;
    carry = __shfl(beyond + p, 0, kWave);
    const float b = live ? beyond : 0.f;
#pragma unroll
    for (int h = 0; h < 2; ++h) {                        // 32 waypoints per half-pass, a lane pair per waypoint
      const int from = h * (kWave / 2) + (lane >> 1);
      const float pk = __shfl(p, from, kWave), bk = __shfl(b, from, kWave);
      const bool lk = __shfl((int)live, from, kWave) != 0;
      if (!lk) continue;
      float sx, sy, sz;
      waypoint(ray, k - lane + from, step, sx, sy, sz);
      const Tri t = make_tri<false>(sx, sy, sz, v);
      tri_scatter_x(hvol, t, pk, cx, acc_hit);
      tri_scatter_x(fvol, t, bk, cx, acc_free);
    }
  });
}

// ---------------------------------------------------------------------------------------------
// Measured evidence of a sweep: the other side of ray_occupancy_body's inverse sensor model.  The rays are listed rays
// whose end point p is a measured return; no volume is read.  With L = |p - o| (dist_to: the length aim divides by), a
// ray that is not skipped and has a finite L > 0 adds
//   free[f, corner c of s_k] += a_k * w_kc      a_k = beam_weight(L, k, step) (occ_score_math.h), k < K
//   hit [f, corner c of p  ] += w_pc            the trilinear weights of the end point itself, whatever K * step is
// on ray_occupancy_body's waypoints s_k and weights (make_tri<false>: corners outside the volume dropped).  a_k == 0 from
// the return on: only beam_trips(L, step, K) waypoints are marched, in passes of 32 with a lane pair per waypoint; the
// end point is lanes 0 and 1's.  One body for every K: nothing is sampled, so there is nothing to keep in registers.
// ---------------------------------------------------------------------------------------------
template <class Acc>
__device__ __forceinline__ void sweep_evidence_body(const ListedRays& src, float* __restrict__ hit,
                                                    float* __restrict__ free_, int R, VolDims v, float step, int ncopies,
                                                    int K, Acc& acc_hit, Acc& acc_free) {
  const int r = blockIdx.x * kRaysPerBlock + threadIdx.x / kWave;
  if (r >= R) return;
  const int lane = threadIdx.x % kWave;
  const Ray ray = load_ray(src, r, v);
  if (ray.f < 0) return;
  const float L = dist_to(ray, ray.px, ray.py, ray.pz);
  if (!(L > 0.f) || !(L < __builtin_inff())) return;       // zero length, NaN or overflowing end point: no measurement
  const size_t copy = scatter_copy_of_block(ncopies) * v.F * v.Z * v.Y * v.X + (size_t)ray.f * v.Z * v.Y * v.X;
  float* hvol = hit + copy;
  float* fvol = free_ + copy;
  const int cx = lane & 1;
  if (lane < 2) tri_scatter_x(hvol, make_tri<false>(ray.px, ray.py, ray.pz, v), 1.f, cx, acc_hit);
  const int trips = vidar_occ::beam_trips(L, step, K);
  for (int j = 0; j * (kWave / 2) < trips; ++j) {
    const int k = (lane >> 1) + j * (kWave / 2);
    if (k >= trips) break;                                 // only in the last pass
    float sx, sy, sz;
    waypoint(ray, k, step, sx, sy, sz);
    tri_scatter_x(fvol, make_tri<false>(sx, sy, sz, v), vidar_occ::beam_weight(L, k, step), cx, acc_free);
  }
}

// ---------------------------------------------------------------------------------------------
// The kernels: one instantiation of a body each.  The ones without a suffix are the register form (K == kK);
// ray_dist runs the streamed form for every K.
// ---------------------------------------------------------------------------------------------
#define RAY_IN const float* __restrict__ sigma, const float* __restrict__ origin, const float* __restrict__ pts, \
               const float* __restrict__ tindex
#define RAY_KERNEL __global__ __launch_bounds__(kThreads) void

RAY_KERNEL ray_ce_fwd_kernel(RAY_IN, float* __restrict__ ce, float* __restrict__ lse, float* __restrict__ valid, int R,
                             VolDims v, float step) {
  ray_ce_fwd_body<true>(sigma, origin, pts, tindex, ce, lse, valid, R, v, step, kK);
}
RAY_KERNEL ray_ce_fwd_any_kernel(RAY_IN, float* __restrict__ ce, float* __restrict__ lse, float* __restrict__ valid,
                                 int R, VolDims v, float step, int K) {
  ray_ce_fwd_body<false>(sigma, origin, pts, tindex, ce, lse, valid, R, v, step, K);
}
RAY_KERNEL ray_ce_bwd_kernel(RAY_IN, const float* __restrict__ lse, const float* __restrict__ grad_ce,
                             float* __restrict__ grad_sigma, int R, VolDims v, float step, int ncopies) {
  det::AccAtomic acc;
  ray_bwd_body<true, true, CeCoef>(sigma, origin, pts, tindex, lse, grad_ce, grad_sigma, R, v, step, ncopies, kK, acc);
}
RAY_KERNEL ray_ce_bwd_any_kernel(RAY_IN, const float* __restrict__ lse, const float* __restrict__ grad_ce,
                                 float* __restrict__ grad_sigma, int R, VolDims v, float step, int ncopies, int K) {
  det::AccAtomic acc;
  ray_bwd_body<false, true, CeCoef>(sigma, origin, pts, tindex, lse, grad_ce, grad_sigma, R, v, step, ncopies, K, acc);
}

RAY_KERNEL ray_gumbel_fwd_kernel(RAY_IN, const float* __restrict__ noise, float* __restrict__ dist,
                                 float* __restrict__ aux, int R, VolDims v, float step) {
  ray_sample_fwd_body<true, false>(sigma, origin, pts, tindex, noise, dist, nullptr, aux, nullptr, R, v, step, kK);
}
RAY_KERNEL ray_gumbel_fwd_any_kernel(RAY_IN, const float* __restrict__ noise, float* __restrict__ dist,
                                     float* __restrict__ aux, int R, VolDims v, float step, int K) {
  ray_sample_fwd_body<false, false>(sigma, origin, pts, tindex, noise, dist, nullptr, aux, nullptr, R, v, step, K);
}
RAY_KERNEL ray_gumbel_bwd_kernel(RAY_IN, const float* __restrict__ aux, const float* __restrict__ grad_dist,
                                 float* __restrict__ grad_sigma, int R, VolDims v, float step, int ncopies) {
  det::AccAtomic acc;
  ray_bwd_body<true, false, SampleCoef>(sigma, origin, pts, tindex, aux, grad_dist, grad_sigma, R, v, step, ncopies, kK, acc);
}
RAY_KERNEL ray_gumbel_bwd_any_kernel(RAY_IN, const float* __restrict__ aux, const float* __restrict__ grad_dist,
                                     float* __restrict__ grad_sigma, int R, VolDims v, float step, int ncopies, int K) {
  det::AccAtomic acc;
  ray_bwd_body<false, false, SampleCoef>(sigma, origin, pts, tindex, aux, grad_dist, grad_sigma, R, v, step, ncopies, K, acc);
}

RAY_KERNEL ray_dist_fwd_kernel(RAY_IN, const float* __restrict__ noise, float* __restrict__ dist,
                               float* __restrict__ gt_len, float* __restrict__ aux, float* __restrict__ valid, int R,
                               VolDims v, float step, int K) {
  ray_sample_fwd_body<false, true>(sigma, origin, pts, tindex, noise, dist, gt_len, aux, valid, R, v, step, K);
}
RAY_KERNEL ray_dist_bwd_kernel(RAY_IN, const float* __restrict__ aux, const float* __restrict__ grad_dist,
                               float* __restrict__ grad_sigma, int R, VolDims v, float step, int ncopies, int K) {
  det::AccAtomic acc;
  ray_bwd_body<false, true, SampleCoef>(sigma, origin, pts, tindex, aux, grad_dist, grad_sigma, R, v, step, ncopies, K, acc);
}

RAY_KERNEL ray_argmax_kernel(RAY_IN, float* __restrict__ pred_dist, float* __restrict__ gt_dist, int R, VolDims v,
                             float step) {
  ray_argmax_body<true>(sigma, ListedRays{origin, pts, tindex}, pred_dist, gt_dist, R, v, step, kK);
}
RAY_KERNEL ray_argmax_any_kernel(RAY_IN, float* __restrict__ pred_dist, float* __restrict__ gt_dist, int R, VolDims v,
                                 float step, int K) {
  ray_argmax_body<false>(sigma, ListedRays{origin, pts, tindex}, pred_dist, gt_dist, R, v, step, K);
}

// camera-view decode: the same body on rays generated from their pixel; dist [F,C,Hs,Ws] is the only store
RAY_KERNEL ray_argmax_cam_kernel(const float* __restrict__ sigma, CameraRays cam, float* __restrict__ dist, int R,
                                 VolDims v, float step) {
  ray_argmax_body<true>(sigma, cam, dist, nullptr, R, v, step, kK);
}
RAY_KERNEL ray_argmax_cam_any_kernel(const float* __restrict__ sigma, CameraRays cam, float* __restrict__ dist, int R,
                                     VolDims v, float step, int K) {
  ray_argmax_body<false>(sigma, cam, dist, nullptr, R, v, step, K);
}
// the decode with its confidence, on listed rays and on camera rays: stats [R,4]
RAY_KERNEL ray_stats_kernel(RAY_IN, float* __restrict__ pred_dist, float* __restrict__ gt_dist,
                            float* __restrict__ stats, int R, VolDims v, float step) {
  ray_stats_body<true>(sigma, ListedRays{origin, pts, tindex}, pred_dist, gt_dist, stats, R, v, step, kK);
}
RAY_KERNEL ray_stats_any_kernel(RAY_IN, float* __restrict__ pred_dist, float* __restrict__ gt_dist,
                                float* __restrict__ stats, int R, VolDims v, float step, int K) {
  ray_stats_body<false>(sigma, ListedRays{origin, pts, tindex}, pred_dist, gt_dist, stats, R, v, step, K);
}
RAY_KERNEL ray_stats_cam_kernel(const float* __restrict__ sigma, CameraRays cam, float* __restrict__ dist,
                                float* __restrict__ stats, int R, VolDims v, float step) {
  ray_stats_body<true>(sigma, cam, dist, nullptr, stats, R, v, step, kK);
}
RAY_KERNEL ray_stats_cam_any_kernel(const float* __restrict__ sigma, CameraRays cam, float* __restrict__ dist,
                                    float* __restrict__ stats, int R, VolDims v, float step, int K) {
  ray_stats_body<false>(sigma, cam, dist, nullptr, stats, R, v, step, K);
}
// the occupancy query at listed end points (out [R,2]) and at every voxel's centre (hit, free [F,Z,Y,X])
RAY_KERNEL point_occupancy_kernel(RAY_IN, float* __restrict__ out, int R, VolDims v, float step, float extent) {
  point_occupancy_body<true>(sigma, ListedRays{origin, pts, tindex}, out, out + 1, 2, R, v, step, extent, kK);
}
RAY_KERNEL point_occupancy_any_kernel(RAY_IN, float* __restrict__ out, int R, VolDims v, float step, float extent,
                                      int K) {
  point_occupancy_body<false>(sigma, ListedRays{origin, pts, tindex}, out, out + 1, 2, R, v, step, extent, K);
}
RAY_KERNEL voxel_occupancy_kernel(const float* __restrict__ sigma, VoxelRays vox, float* __restrict__ hit,
                                  float* __restrict__ free_, int R, VolDims v, float step, float extent) {
  point_occupancy_body<true>(sigma, vox, hit, free_, 1, R, v, step, extent, kK);
}
RAY_KERNEL voxel_occupancy_any_kernel(const float* __restrict__ sigma, VoxelRays vox, float* __restrict__ hit,
                                      float* __restrict__ free_, int R, VolDims v, float step, float extent, int K) {
  point_occupancy_body<false>(sigma, vox, hit, free_, 1, R, v, step, extent, K);
}
// what ray_argmax_cam_kernel marches, written out: origin [F,C,3], pts [F,C,Hs,Ws,3]; a thread per pixel
__global__ __launch_bounds__(kThreads) void cam_rays_kernel(CameraRays cam, float* __restrict__ origin,
                                                            float* __restrict__ pts, int R) {
  const int r = blockIdx.x * kThreads + threadIdx.x;
  if (r >= R) return;
  int f, fc, x, y;
  vidar_cam::split_ray_index(r, cam.g, f, fc, x, y);
  const vidar_cam::CamRay c = vidar_cam::pixel_ray(cam.pix2vox + (size_t)fc * 16, cam.g, x, y);
  pts[(size_t)r * 3 + 0] = c.px; pts[(size_t)r * 3 + 1] = c.py; pts[(size_t)r * 3 + 2] = c.pz;
  if (x == 0 && y == 0) { origin[fc * 3 + 0] = c.ox; origin[fc * 3 + 1] = c.oy; origin[fc * 3 + 2] = c.oz; }
}

// Deterministic mode (det_acc.h): the same body under the measure policy, then under the fixed-point policy, adding
// straight into the one accumulator volume (no private copies).  Both K forms produce the same contributions.
template <bool K512, bool END_POINT, class Coef, class Acc>
RAY_KERNEL ray_bwd_det_kernel(RAY_IN, const float* __restrict__ saved, const float* __restrict__ grad,
                              float* __restrict__ grad_sigma, int R, VolDims v, float step, int K,
                              typename Acc::Param param) {
  Acc acc(grad_sigma, param);
  ray_bwd_body<K512, END_POINT, Coef>(sigma, origin, pts, tindex, saved, grad, grad_sigma, R, v, step, 1, K, acc);
  acc.flush();
}
// Occupancy evidence, every mode: Acc = AccAtomic is the default launch (private copies when ncopies > 1), AccMeasure /
// AccFixed the deterministic mode's two passes (ncopies == 1).  `src`: ListedRays or CameraRays.
template <bool K512, class Src, class Acc>
RAY_KERNEL ray_occupancy_kernel(const float* __restrict__ sigma, Src src, float* __restrict__ hit,
                                float* __restrict__ free_, int R, VolDims v, float step, int ncopies, int K,
                                typename Acc::Param param_hit, typename Acc::Param param_free) {
  Acc acc_hit(hit, param_hit), acc_free(free_, param_free);
  ray_occupancy_body<K512>(sigma, src, hit, free_, R, v, step, ncopies, K, acc_hit, acc_free);
  acc_hit.flush();
  acc_free.flush();
}
// Measured evidence, every mode, as ray_occupancy_kernel
template <class Acc>
RAY_KERNEL sweep_evidence_kernel(ListedRays src, float* __restrict__ hit, float* __restrict__ free_, int R, VolDims v,
                                 float step, int ncopies, int K, typename Acc::Param param_hit,
                                 typename Acc::Param param_free) {
  Acc acc_hit(hit, param_hit), acc_free(free_, param_free);
  sweep_evidence_body(src, hit, free_, R, v, step, ncopies, K, acc_hit, acc_free);
  acc_hit.flush();
  acc_free.flush();
}
#undef RAY_KERNEL
#undef RAY_IN

inline bool rm_bad(int F, int R, int Z, int Y, int X, int K) {
  return F <= 0 || R < 0 || Z <= 0 || Y <= 0 || X <= 0 || K < 1 || K > kKMax;
}
// camera grid: F*C*Hs*Ws rays must fit the 32-bit ray index; `R` is set only when the geometry is good
inline bool cam_bad(int F, int C, int Hs, int Ws, float u0, float v0, float du, float dv, int& R) {
  if (F <= 0 || C <= 0 || Hs < 0 || Ws < 0) return true;
  if (!(u0 == u0 && v0 == v0 && du == du && dv == dv) || du == 0.f || dv == 0.f) return true;
  const uint64_t n = (uint64_t)F * (uint64_t)C * (uint64_t)Hs * (uint64_t)Ws;
  if (n > (uint64_t)0x7fffffff - kThreads) return true;
  R = (int)n;
  return false;
}
// stats [R,4] is stored as one 16-byte value per ray
inline bool stats_misaligned(const float* stats) { return ((uintptr_t)stats & 15) != 0; }
std::atomic<int> g_force_streamed{0};   // vidar_ray_force_streamed
inline bool rm_k512(int K) { return K == kK && !g_force_streamed.load(std::memory_order_relaxed); }
inline dim3 rm_grid(int R) { return dim3((R + kRaysPerBlock - 1) / kRaysPerBlock); }
inline size_t rm_cells(const VolDims& v) { return (size_t)v.F * v.Z * v.Y * v.X; }

// launch `k512` (register form) or `any` (streamed, takes K as its last argument) on a wave per ray
template <class K512Kernel, class AnyKernel, class... Args>
inline void rm_launch(K512Kernel k512, AnyKernel any, int R, int K, hipStream_t s, Args... args) {
  if (rm_k512(K))
    hipLaunchKernelGGL(k512, rm_grid(R), dim3(kThreads), 0, s, args...);
  else
    hipLaunchKernelGGL(any, rm_grid(R), dim3(kThreads), 0, s, args..., K);
}


// A ray backward: private copies of grad_sigma if the workspace allows (scatter_copies.h), or the deterministic mode's
// two passes over at most 8 corners of K (+ the end point) entries per ray; R == 0 leaves zeros.
// `default_launch(acc, nullptr, ncopies)` enqueues the op's own kernel.
template <bool END_POINT, class Coef, class DefaultLaunch>
int rm_bwd(const float* sigma, const float* origin, const float* pts, const float* tindex, const float* saved,
           const float* grad, float* grad_sigma, int R, int K, VolDims v, float step, void* workspace,
           size_t workspace_bytes, hipStream_t s, DefaultLaunch default_launch) {
  const bool k512 = rm_k512(K);
  return scatter_backward(
      grad_sigma, nullptr, rm_cells(v), 0, (uint64_t)R * ((uint64_t)K + END_POINT) * 8, R == 0, workspace,
      workspace_bytes, s, default_launch,
      [&](auto tag, auto param, auto) {
        using Acc = decltype(tag);
        const auto k = k512 ? ray_bwd_det_kernel<true, END_POINT, Coef, Acc> : ray_bwd_det_kernel<false, END_POINT, Coef, Acc>;
        hipLaunchKernelGGL(k, rm_grid(R), dim3(kThreads), 0, s, sigma, origin, pts, tindex, saved, grad, grad_sigma, R,
                           v, step, k512 ? kK : K, param);
      });
}

// The occupancy march from either ray source: the same shell with hit and free as its two outputs, at most 8 corners of
// K waypoints per ray and output.
template <class Acc> struct Policy { using type = Acc; };   // names a policy on the host (AccAtomic has no host object)
template <class Src>
int rm_occupancy(const float* sigma, const Src& src, float* hit, float* free_, int R, int K, VolDims v, float step,
                 void* workspace, size_t workspace_bytes, hipStream_t s) {
  const bool k512 = rm_k512(K);
  const auto launch = [&](auto policy, float* h, float* f, int ncopies, auto p_hit, auto p_free) {
    using Acc = typename decltype(policy)::type;
    const auto k = k512 ? ray_occupancy_kernel<true, Src, Acc> : ray_occupancy_kernel<false, Src, Acc>;
    hipLaunchKernelGGL(k, rm_grid(R), dim3(kThreads), 0, s, sigma, src, h, f, R, v, step, ncopies, k512 ? kK : K, p_hit,
                       p_free);
  };
  return scatter_backward(
      hit, free_, rm_cells(v), rm_cells(v), (uint64_t)R * (uint64_t)K * 8, R == 0, workspace, workspace_bytes, s,
      [&](float* h, float* f, int ncopies) {
        launch(Policy<det::AccAtomic>{}, h, f, ncopies, det::AccAtomic::Param{}, det::AccAtomic::Param{});
      },
      [&](auto tag, auto p_hit, auto p_free) { launch(Policy<decltype(tag)>{}, hit, free_, 1, p_hit, p_free); });
}

// The measured evidence: the same shell; at most 8 corners of K waypoints and of the end point per ray and output.
int rm_sweep_evidence(const ListedRays& src, float* hit, float* free_, int R, int K, VolDims v, float step,
                      void* workspace, size_t workspace_bytes, hipStream_t s) {
  const auto launch = [&](auto policy, float* h, float* f, int ncopies, auto p_hit, auto p_free) {
    using Acc = typename decltype(policy)::type;
    hipLaunchKernelGGL(sweep_evidence_kernel<Acc>, rm_grid(R), dim3(kThreads), 0, s, src, h, f, R, v, step, ncopies, K,
                       p_hit, p_free);
  };
  return scatter_backward(
      hit, free_, rm_cells(v), rm_cells(v), (uint64_t)R * ((uint64_t)K + 1) * 8, R == 0, workspace, workspace_bytes, s,
      [&](float* h, float* f, int ncopies) {
        launch(Policy<det::AccAtomic>{}, h, f, ncopies, det::AccAtomic::Param{}, det::AccAtomic::Param{});
      },
      [&](auto tag, auto p_hit, auto p_free) { launch(Policy<decltype(tag)>{}, hit, free_, 1, p_hit, p_free); });
}

}  // namespace

extern "C" {

size_t vidar_ray_bwd_workspace_bytes(int F, int Z, int Y, int X) {
  if (F <= 0 || Z <= 0 || Y <= 0 || X <= 0) return 0;
  return scatter_backward_workspace_bytes(rm_cells(VolDims{F, Z, Y, X}), 1);
}

int vidar_ray_max_k(void) { return kKMax; }

int vidar_ray_force_streamed(int on) {
  return g_force_streamed.exchange(on != 0, std::memory_order_relaxed);
}

int vidar_ray_ce_fwd_f32(const float* sigma, const float* origin, const float* gt_pts,
                         const float* tindex, float* ce, float* lse, float* valid, int F, int R,
                         int Z, int Y, int X, int K, float step, void* stream) {
  VIDAR_ENTER();
  if (rm_bad(F, R, Z, Y, X, K)) return VIDAR_ERR_BAD_ARG;
  if (R == 0) return 0;
  VolDims v{F, Z, Y, X};
  rm_launch(ray_ce_fwd_kernel, ray_ce_fwd_any_kernel, R, K, (hipStream_t)stream, sigma, origin, gt_pts, tindex, ce, lse,
            valid, R, v, step);
  return vidar_last_error();
}

// the three backwards: rm_bwd with the op's default kernels
int vidar_ray_ce_bwd_f32(const float* sigma, const float* origin, const float* gt_pts,
                         const float* tindex, const float* lse, const float* grad_ce,
                         float* grad_sigma, int F, int R, int Z, int Y, int X, int K, float step,
                         void* workspace, size_t workspace_bytes, void* stream) {
  VIDAR_ENTER();
  if (rm_bad(F, R, Z, Y, X, K)) return VIDAR_ERR_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  VolDims v{F, Z, Y, X};
  return rm_bwd<true, CeCoef>(sigma, origin, gt_pts, tindex, lse, grad_ce, grad_sigma, R, K, v, step, workspace,
                              workspace_bytes, s, [&](float* acc, float*, int ncopies) {
    rm_launch(ray_ce_bwd_kernel, ray_ce_bwd_any_kernel, R, K, s, sigma, origin, gt_pts, tindex, lse, grad_ce, acc, R, v,
              step, ncopies);
  });
}

int vidar_ray_gumbel_fwd_f32(const float* sigma, const float* origin, const float* pts,
                             const float* tindex, const float* noise, float* dist, float* aux, int F,
                             int R, int Z, int Y, int X, int K, float step, void* stream) {
  VIDAR_ENTER();
  if (rm_bad(F, R, Z, Y, X, K)) return VIDAR_ERR_BAD_ARG;
  if (R == 0) return 0;
  VolDims v{F, Z, Y, X};
  rm_launch(ray_gumbel_fwd_kernel, ray_gumbel_fwd_any_kernel, R, K, (hipStream_t)stream, sigma, origin, pts, tindex,
            noise, dist, aux, R, v, step);
  return vidar_last_error();
}

int vidar_ray_gumbel_bwd_f32(const float* sigma, const float* origin, const float* pts,
                             const float* tindex, const float* aux, const float* grad_dist,
                             float* grad_sigma, int F, int R, int Z, int Y, int X, int K, float step,
                             void* workspace, size_t workspace_bytes, void* stream) {
  VIDAR_ENTER();
  if (rm_bad(F, R, Z, Y, X, K)) return VIDAR_ERR_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  VolDims v{F, Z, Y, X};
  return rm_bwd<false, SampleCoef>(sigma, origin, pts, tindex, aux, grad_dist, grad_sigma, R, K, v, step, workspace,
                                   workspace_bytes, s, [&](float* acc, float*, int ncopies) {
    rm_launch(ray_gumbel_bwd_kernel, ray_gumbel_bwd_any_kernel, R, K, s, sigma, origin, pts, tindex, aux, grad_dist, acc,
              R, v, step, ncopies);
  });
}

int vidar_ray_dist_fwd_f32(const float* sigma, const float* origin, const float* gt_pts,
                           const float* tindex, const float* noise, float* dist, float* gt_len, float* aux,
                           float* valid, int F, int R, int Z, int Y, int X, int K, float step, void* stream) {
  VIDAR_ENTER();
  if (rm_bad(F, R, Z, Y, X, K)) return VIDAR_ERR_BAD_ARG;
  if (R == 0) return 0;
  VolDims v{F, Z, Y, X};
  hipLaunchKernelGGL(ray_dist_fwd_kernel, rm_grid(R), dim3(kThreads), 0, (hipStream_t)stream, sigma, origin,
                     gt_pts, tindex, noise, dist, gt_len, aux, valid, R, v, step, K);
  return vidar_last_error();
}

int vidar_ray_dist_bwd_f32(const float* sigma, const float* origin, const float* gt_pts,
                           const float* tindex, const float* aux, const float* grad_dist,
                           float* grad_sigma, int F, int R, int Z, int Y, int X, int K, float step,
                           void* workspace, size_t workspace_bytes, void* stream) {
  VIDAR_ENTER();
  if (rm_bad(F, R, Z, Y, X, K)) return VIDAR_ERR_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  VolDims v{F, Z, Y, X};
  return rm_bwd<true, SampleCoef>(sigma, origin, gt_pts, tindex, aux, grad_dist, grad_sigma, R, K, v, step, workspace,
                                  workspace_bytes, s, [&](float* acc, float*, int ncopies) {
    hipLaunchKernelGGL(ray_dist_bwd_kernel, rm_grid(R), dim3(kThreads), 0, s, sigma, origin, gt_pts, tindex, aux,
                       grad_dist, acc, R, v, step, ncopies, K);
  });
}

int vidar_ray_argmax_f32(const float* sigma, const float* origin, const float* pts,
                         const float* tindex, float* pred_dist, float* gt_dist, int F, int R, int Z,
                         int Y, int X, int K, float step, void* stream) {
  VIDAR_ENTER();
  if (rm_bad(F, R, Z, Y, X, K)) return VIDAR_ERR_BAD_ARG;
  if (R == 0) return 0;
  VolDims v{F, Z, Y, X};
  rm_launch(ray_argmax_kernel, ray_argmax_any_kernel, R, K, (hipStream_t)stream, sigma, origin, pts, tindex, pred_dist,
            gt_dist, R, v, step);
  return vidar_last_error();
}

int vidar_ray_argmax_cam_f32(const float* sigma, const float* pix2vox, float* dist, int F, int C, int Hs, int Ws,
                             float u0, float v0, float du, float dv, int Z, int Y, int X, int K, float step,
                             void* stream) {
  VIDAR_ENTER();
  int R = 0;
  if (cam_bad(F, C, Hs, Ws, u0, v0, du, dv, R) || rm_bad(F, R, Z, Y, X, K)) return VIDAR_ERR_BAD_ARG;
  if (R == 0) return 0;
  VolDims v{F, Z, Y, X};
  const CameraRays cam{pix2vox, vidar_cam::CamGrid{C, Hs, Ws, u0, v0, du, dv}};
  rm_launch(ray_argmax_cam_kernel, ray_argmax_cam_any_kernel, R, K, (hipStream_t)stream, sigma, cam, dist, R, v, step);
  return vidar_last_error();
}

int vidar_ray_stats_f32(const float* sigma, const float* origin, const float* pts, const float* tindex,
                        float* pred_dist, float* gt_dist, float* stats, int F, int R, int Z, int Y, int X, int K,
                        float step, void* stream) {
  VIDAR_ENTER();
  if (rm_bad(F, R, Z, Y, X, K) || stats_misaligned(stats)) return VIDAR_ERR_BAD_ARG;
  if (R == 0) return 0;
  VolDims v{F, Z, Y, X};
  rm_launch(ray_stats_kernel, ray_stats_any_kernel, R, K, (hipStream_t)stream, sigma, origin, pts, tindex, pred_dist,
            gt_dist, stats, R, v, step);
  return vidar_last_error();
}

int vidar_ray_stats_cam_f32(const float* sigma, const float* pix2vox, float* dist, float* stats, int F, int C, int Hs,
                            int Ws, float u0, float v0, float du, float dv, int Z, int Y, int X, int K, float step,
                            void* stream) {
  VIDAR_ENTER();
  int R = 0;
  if (cam_bad(F, C, Hs, Ws, u0, v0, du, dv, R) || rm_bad(F, R, Z, Y, X, K) || stats_misaligned(stats))
    return VIDAR_ERR_BAD_ARG;
  if (R == 0) return 0;
  VolDims v{F, Z, Y, X};
  const CameraRays cam{pix2vox, vidar_cam::CamGrid{C, Hs, Ws, u0, v0, du, dv}};
  rm_launch(ray_stats_cam_kernel, ray_stats_cam_any_kernel, R, K, (hipStream_t)stream, sigma, cam, dist, stats, R, v,
            step);
  return vidar_last_error();
}

int vidar_ray_occupancy_workspace_bytes(int F, int Z, int Y, int X, int64_t* bytes) {
  if (!bytes || F <= 0 || Z <= 0 || Y <= 0 || X <= 0) return VIDAR_ERR_BAD_ARG;
  *bytes = (int64_t)scatter_backward_workspace_bytes(2 * rm_cells(VolDims{F, Z, Y, X}), 2);
  return 0;
}

int vidar_ray_occupancy_f32(const float* sigma, const float* origin, const float* pts, const float* tindex, float* hit,
                            float* free_, int F, int R, int Z, int Y, int X, int K, float step, void* workspace,
                            size_t workspace_bytes, void* stream) {
  VIDAR_ENTER();
  if (rm_bad(F, R, Z, Y, X, K)) return VIDAR_ERR_BAD_ARG;
  return rm_occupancy(sigma, ListedRays{origin, pts, tindex}, hit, free_, R, K, VolDims{F, Z, Y, X}, step, workspace,
                      workspace_bytes, (hipStream_t)stream);
}

int vidar_ray_occupancy_cam_f32(const float* sigma, const float* pix2vox, float* hit, float* free_, int F, int C, int Hs,
                                int Ws, float u0, float v0, float du, float dv, int Z, int Y, int X, int K, float step,
                                void* workspace, size_t workspace_bytes, void* stream) {
  VIDAR_ENTER();
  int R = 0;
  if (cam_bad(F, C, Hs, Ws, u0, v0, du, dv, R) || rm_bad(F, R, Z, Y, X, K)) return VIDAR_ERR_BAD_ARG;
  const CameraRays cam{pix2vox, vidar_cam::CamGrid{C, Hs, Ws, u0, v0, du, dv}};
  return rm_occupancy(sigma, cam, hit, free_, R, K, VolDims{F, Z, Y, X}, step, workspace, workspace_bytes,
                      (hipStream_t)stream);
}

int vidar_sweep_evidence_f32(const float* origin, const float* pts, const float* tindex, float* hit, float* free_, int F,
                             int R, int Z, int Y, int X, int K, float step, void* workspace, size_t workspace_bytes,
                             void* stream) {
  VIDAR_ENTER();
  if (rm_bad(F, R, Z, Y, X, K)) return VIDAR_ERR_BAD_ARG;
  return rm_sweep_evidence(ListedRays{origin, pts, tindex}, hit, free_, R, K, VolDims{F, Z, Y, X}, step, workspace,
                           workspace_bytes, (hipStream_t)stream);
}

int vidar_point_occupancy_f32(const float* sigma, const float* origin, const float* pts, const float* tindex,
                              float* out, int F, int R, int Z, int Y, int X, int K, float step, float extent,
                              void* stream) {
  VIDAR_ENTER();
  if (rm_bad(F, R, Z, Y, X, K) || vidar_occ_at::bad_extent(extent)) return VIDAR_ERR_BAD_ARG;
  if (R == 0) return 0;
  if (!sigma || !origin || !pts || !tindex || !out) return VIDAR_ERR_BAD_ARG;
  VolDims v{F, Z, Y, X};
  rm_launch(point_occupancy_kernel, point_occupancy_any_kernel, R, K, (hipStream_t)stream, sigma, origin, pts, tindex,
            out, R, v, step, extent);
  return vidar_last_error();
}

int vidar_voxel_occupancy_f32(const float* sigma, const float* origin, float* hit, float* free_, int F, int Z, int Y,
                              int X, int K, float step, float extent, void* stream) {
  VIDAR_ENTER();
  // F == 0 is the empty problem here (the rays are the voxels); F*Z*Y*X must fit the 32-bit ray index
  if (F < 0 || rm_bad(F ? F : 1, 0, Z, Y, X, K) || vidar_occ_at::bad_extent(extent)) return VIDAR_ERR_BAD_ARG;
  VolDims v{F, Z, Y, X};
  if ((uint64_t)F * (uint64_t)Z * (uint64_t)Y * (uint64_t)X > (uint64_t)0x7fffffff - kThreads) return VIDAR_ERR_BAD_ARG;
  if (F == 0) return 0;
  if (!sigma || !origin || !hit || !free_) return VIDAR_ERR_BAD_ARG;
  const int R = (int)rm_cells(v);
  rm_launch(voxel_occupancy_kernel, voxel_occupancy_any_kernel, R, K, (hipStream_t)stream, sigma, VoxelRays{origin}, hit,
            free_, R, v, step, extent);
  return vidar_last_error();
}

int vidar_cam_rays_f32(const float* pix2vox, float* origin, float* pts, int F, int C, int Hs, int Ws, float u0,
                       float v0, float du, float dv, void* stream) {
  VIDAR_ENTER();
  int R = 0;
  if (cam_bad(F, C, Hs, Ws, u0, v0, du, dv, R)) return VIDAR_ERR_BAD_ARG;
  if (R == 0) return 0;
  const CameraRays cam{pix2vox, vidar_cam::CamGrid{C, Hs, Ws, u0, v0, du, dv}};
  hipLaunchKernelGGL(cam_rays_kernel, dim3((R + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, cam,
                     origin, pts, R);
  return vidar_last_error();
}

}  // extern "C"
