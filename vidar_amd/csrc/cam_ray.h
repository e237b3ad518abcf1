// Pixel -> ray of the camera-view march (vidar_ray_argmax_cam_f32 / vidar_cam_rays_f32, csrc/ray_march.hip).
//
// pix2vox [4,4] row-major maps the homogeneous pixel (u*d, v*d, d, 1) to voxel coordinates of one frame's volume.  It
// is the inverse of an affine camera matrix (last row 0 0 0 1), so only its first three rows are read:
//   origin    = image of (0, 0, 0, 1) = column 3                         (the camera centre)
//   end point = image of (u, v, 1, 1) = ((m0*u + m1*v) + m2) + m3 per row (the point at depth 1)
// Plain C++ on purpose: both kernels inline this one function, and tests/cam_ray_host.cpp compiles the same text for the
// host.  Every operation rounds on its own (no fused multiply-add), whatever the including file is compiled with, so
// the fused march and the materialised rays see the same bits.
#pragma once

#ifdef __HIPCC__
#define VIDAR_CAM_FN __host__ __device__ __forceinline__
#else
#define VIDAR_CAM_FN inline
#endif

namespace vidar_cam {

// pixel (x, y) of the [Hs, Ws] grid -> u = u0 + x*du, v = v0 + y*dv
struct CamGrid {
  int C, Hs, Ws;
  float u0, v0, du, dv;
};

struct CamRay {
  float ox, oy, oz;   // camera centre
  float px, py, pz;   // point at depth 1
};

VIDAR_CAM_FN CamRay pixel_ray(const float* __restrict__ m, const CamGrid& g, int x, int y) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const float u = g.u0 + (float)x * g.du;
  const float v = g.v0 + (float)y * g.dv;
  CamRay r;
  r.ox = m[3]; r.oy = m[7]; r.oz = m[11];
  r.px = ((m[0] * u + m[1] * v) + m[2]) + m[3];
  r.py = ((m[4] * u + m[5] * v) + m[6]) + m[7];
  r.pz = ((m[8] * u + m[9] * v) + m[10]) + m[11];
  return r;
}

// ray index r of [F, C, Hs, Ws] -> frame f, matrix slot f*C + c, pixel (x, y)
VIDAR_CAM_FN void split_ray_index(int r, const CamGrid& g, int& f, int& fc, int& x, int& y) {
  x = r % g.Ws;
  const int t = r / g.Ws;
  y = t % g.Hs;
  fc = t / g.Hs;
  f = fc / g.C;
}

}  // namespace vidar_cam
