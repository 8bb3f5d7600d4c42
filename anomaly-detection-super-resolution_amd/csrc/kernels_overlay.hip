// kernels_overlay.hip - the overlay of an anomaly map and the outline of its mask on the image they were made from
// (srad_overlay_rgb; DESIGN.md "Maps and masks at source size").  One thread per pixel: one fp32 multiply picks the level of a
// 256-entry colour table, the blend is integer, and a mask pixel is contour when a pixel within Chebyshev distance r is 0 or
// outside the image.  Every output byte is defined by the inputs; no atomics, no workspace.
#include "srad_common.h"

namespace {

constexpr int kOverlayMaxRadius = 4;

__global__ __launch_bounds__(256) void overlay_rgb_kernel(const uint8_t* __restrict__ src, const float* __restrict__ maps,
                                                          const uint8_t* __restrict__ masks, const uint8_t* __restrict__ lut,
                                                          uint8_t* __restrict__ out, size_t total, int H, int W, int Cs, float scale,
                                                          int radius, int cr, int cg, int cb) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % W), y = (int)((i / W) % H);
  uint8_t* o = out + 3 * i;
  if (radius > 0 && masks[i]) {
    bool edge = y < radius || x < radius || y + radius >= H || x + radius >= W;     // the window leaves the image
    if (!edge) {
      const uint8_t* m = masks + i;
      for (int dy = -radius; dy <= radius && !edge; ++dy)
        for (int dx = -radius; dx <= radius; ++dx) edge |= m[(ptrdiff_t)dy * W + dx] == 0;
    }
    if (edge) {
      o[0] = (uint8_t)cr, o[1] = (uint8_t)cg, o[2] = (uint8_t)cb;
      return;
    }
  }
  const float q = maps[i] * scale;
  const int level = q >= 255.0f ? 255 : (q > 0.0f ? (int)q : 0);               // NaN fails both comparisons: level 0
  const uint8_t* t = lut + 4 * level;
  const int a = t[3];
  const uint8_t* p = src + i * Cs;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int v = Cs == 3 ? p[c] : p[0];
    o[c] = (uint8_t)((v * (255 - a) + t[c] * a + 127) / 255);
  }
}

}  // namespace

extern "C" int srad_overlay_rgb(const uint8_t* src, int n, int H, int W, int Cs, const float* maps, const uint8_t* masks, const uint8_t* lut,
                                float scale, int contour_radius, int contour_r, int contour_g, int contour_b, uint8_t* out, void* stream) {
  SRAD_REQUIRE(src && maps && masks && lut && out, "overlay_rgb: null argument");
  SRAD_REQUIRE(n >= 1 && H >= 1 && W >= 1, "overlay_rgb: sizes must be >= 1, got n=%d %dx%d", n, H, W);
  SRAD_REQUIRE(Cs == 1 || Cs == 3, "overlay_rgb: %d source channels, 1 or 3 are supported", Cs);
  SRAD_REQUIRE(contour_radius >= 0 && contour_radius <= kOverlayMaxRadius, "overlay_rgb: contour radius %d, 0 to %d are supported", contour_radius,
               kOverlayMaxRadius);
  SRAD_REQUIRE((contour_r | contour_g | contour_b) >= 0 && contour_r <= 255 && contour_g <= 255 && contour_b <= 255,
               "overlay_rgb: contour colour (%d, %d, %d), every value must be 0 .. 255", contour_r, contour_g, contour_b);
  SRAD_REQUIRE(scale == scale, "overlay_rgb: the scale is NaN");
  const size_t total = (size_t)n * H * W;
  SRAD_REQUIRE(!srad_byte_ranges_overlap(out, 3 * total, src, total * Cs) && !srad_byte_ranges_overlap(out, 3 * total, maps, 4 * total) &&
                   !srad_byte_ranges_overlap(out, 3 * total, masks, total) && !srad_byte_ranges_overlap(out, 3 * total, lut, 1024),
               "overlay_rgb: out overlaps an input");
  const unsigned long long blocks = (total + 255) / 256;
  SRAD_REQUIRE(blocks < (1ull << 31), "overlay_rgb: n=%d %dx%d needs more than 2^31 workgroups", n, H, W);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  SradProfScope prof(s, SRAD_K_OVERLAY, 0.0, (double)total * (Cs + 4 + 1 + 3));
  hipLaunchKernelGGL(overlay_rgb_kernel, dim3((unsigned)blocks), dim3(256), 0, s, src, maps, masks, lut, out, total, H, W, Cs, scale, contour_radius,
                     contour_r, contour_g, contour_b);
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}
