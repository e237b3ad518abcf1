// TEST INFRASTRUCTURE.  Compiles vidar_amd/csrc/cam_ray.h (the pixel -> ray function that vidar_ray_argmax_cam_f32 and
// vidar_cam_rays_f32 inline) with g++ into a stand-alone program: the pixels are a plain loop and every buffer is a heap
// vector of exactly its size, so the CPU test-suite (tests/test_forecast_view_cpu.py) can compare the rays with fp64 on
// a machine without a GPU, under the host sanitizers when the toolchain has them.  Never used by the product.
//
//   cam_ray_host IN OUT
// IN : int32 F, C, Hs, Ws; float u0, v0, du, dv; float pix2vox[F * C * 16]
// OUT: float origin[F * C * 3]; float pts[F * C * Hs * Ws * 3]      (what cam_rays_kernel writes, in its order)
// The outputs start as NaN: what the loop does not write shows.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>

#include "cam_ray.h"

using namespace vidar_cam;

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 3;
  int32_t dims[4];
  float geom[4];
  if (fread(dims, sizeof(int32_t), 4, in) != 4 || fread(geom, sizeof(float), 4, in) != 4) return 4;
  const int F = dims[0], C = dims[1], Hs = dims[2], Ws = dims[3];
  if (F <= 0 || C <= 0 || Hs < 0 || Ws < 0 || (int64_t)F * C * Hs * Ws > (1 << 24)) return 4;
  std::vector<float> m((size_t)F * C * 16);
  if (fread(m.data(), sizeof(float), m.size(), in) != m.size()) return 4;
  fclose(in);

  const CamGrid g{C, Hs, Ws, geom[0], geom[1], geom[2], geom[3]};
  const int R = F * C * Hs * Ws;
  std::vector<float> origin((size_t)F * C * 3, NAN), pts((size_t)R * 3, NAN);
  for (int r = 0; r < R; ++r) {                      // cam_rays_kernel, one thread per r
    int f, fc, x, y;
    split_ray_index(r, g, f, fc, x, y);
    if (f != fc / C || fc < 0 || fc >= F * C || x < 0 || x >= Ws || y < 0 || y >= Hs) return 7;
    const std::vector<float> one(m.begin() + (size_t)fc * 16, m.begin() + (size_t)fc * 16 + 16);   // exactly one matrix
    const CamRay c = pixel_ray(one.data(), g, x, y);
    pts[(size_t)r * 3 + 0] = c.px; pts[(size_t)r * 3 + 1] = c.py; pts[(size_t)r * 3 + 2] = c.pz;
    if (x == 0 && y == 0) { origin[(size_t)fc * 3 + 0] = c.ox; origin[(size_t)fc * 3 + 1] = c.oy; origin[(size_t)fc * 3 + 2] = c.oz; }
  }
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 5;
  if (fwrite(origin.data(), sizeof(float), origin.size(), o) != origin.size()) return 6;
  if (!pts.empty() && fwrite(pts.data(), sizeof(float), pts.size(), o) != pts.size()) return 6;
  fclose(o);
  printf("%d rays\n", R);
  return 0;
}
