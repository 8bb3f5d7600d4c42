// kernels_map_smooth.hip - Gaussian smoothing of anomaly maps on gfx950, equal bit for bit to
//     scipy.ndimage.gaussian_filter(maps, (0, sigma, sigma), mode='reflect', truncate=t)
// when it is given scipy's weights, and the per-image maximum of the result in the same launch.
//
// What scipy does, restated: two separable passes of a symmetric filter, along H first, then along W on the H pass's output
// rounded to fp32.  Each output of a pass is an fp64 sum in a fixed order, every product and sum rounded on its own:
//     acc = x[i] * w[0];  for j = r down to 1: acc = acc + (x[i - j] + x[i + j]) * w[j];  out = (float)acc
// (scipy's symmetric correlate loop starts at the farthest tap and walks inward; the order decides the fp64 rounding)
// with half-sample reflection at the edges (d c b a | a b c d).  The file is compiled without FMA contraction, so the fp64
// operations are exactly those; the weights come from the host as kernel arguments (std::exp and numpy's exp differ in the last
// bit), so this side never computes one.
//
// One launch, one workgroup per tile of kTileH x kTileW outputs of one image:
//   1. the H pass for the tile's rows and its columns plus r halo columns on each side, straight from global memory (a wave reads
//      one row of 64 consecutive columns at a time, so the loads are coalesced and the row index is wave-uniform; each lane keeps
//      four rows' fp64 chains in flight and slides their inputs through registers), its fp32 result kept in LDS;
//   2. the W pass from LDS, the stores, and the tile's maximum: a wave reduction of order_key (pixel_sort.h; NaN is the largest
//      key) and one atomicMax per workgroup into a u32 per image.  A max does not depend on the order, so the result is
//      deterministic.  A last tiny kernel turns the keys back into floats (map_max.h, shared with kernels_map_baseline.hip).
#include "engine.h"
#include "../../include/srad.h"
#include "map_max.h"
#include <algorithm>
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int kMaxRadius = 128;
constexpr int kTileW = 128, kTileH = 16;
constexpr int kMidW = kTileW + 2 * kMaxRadius;          // 384 floats per LDS row: 24 KB for the tile at any radius

struct SmoothWeights {
  double w[kMaxRadius + 1];                              // w[0] centre, w[j] the weight at offsets +-j
};

__device__ __forceinline__ int reflect1(int i, int n) { return i < 0 ? -i - 1 : (i >= n ? 2 * n - 1 - i : i); }

__global__ __launch_bounds__(256) void smooth_maps_kernel(const float* __restrict__ maps, float* __restrict__ out,
                                                          uint32_t* __restrict__ max_key, int H, int W, int r, int tiles_x,
                                                          int tiles_y, SmoothWeights wt) {
  __shared__ float mid[kTileH * kMidW];
  __shared__ uint32_t wave_max[4];
  const int tx = blockIdx.x % tiles_x, t2 = blockIdx.x / tiles_x;
  const int ty = t2 % tiles_y, img = t2 / tiles_y;
  const int x0 = tx * kTileW, y0 = ty * kTileH;
  const int rows = min(kTileH, H - y0), cols = min(kTileW, W - x0);
  const int nc = cols + 2 * r;                           // mid column c holds image column x0 - r + c, reflected once
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const size_t plane = (size_t)H * W;
  const float* __restrict__ src = maps + (size_t)img * plane;
  const double w0 = wt.w[0];

  // 1. H pass: wave wv owns the tile rows 4 wv .. 4 wv + 3 and keeps their four fp64 chains in flight at once; the lanes walk the
  //    columns.  The rows slide through registers: at tap j (from r inward), lo[k] = x[gy0 + k - j] and hi[k] = x[gy0 + k + j],
  //    so each tap after the first loads two rows (gy0 + 3 - j and gy0 + j) for four outputs.  Row indices are wave-uniform; an
  //    index is clamped to
  //    [-r, H - 1 + r] and reflected once, which changes nothing for a row inside the image: a row past the image's end only
  //    computes a value that is never stored.
  const int row0 = wv * 4;
  if (row0 < rows) {
    const int gy0 = y0 + row0;
    auto row_of = [&](int i) { return (size_t)reflect1(min(i, H - 1 + r), H) * W; };
    for (int c = lane; c < nc; c += 64) {
      const float* __restrict__ col = src + reflect1(x0 - r + c, W);
      float lo[4], hi[4];
      double acc[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[k] = (double)col[row_of(gy0 + k)] * w0;
      if (r > 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          lo[k] = col[row_of(gy0 + k - r)];
          hi[k] = col[row_of(gy0 + k + r)];
        }
        for (int j = r;; --j) {
          const double wj = wt.w[j];
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[k] = acc[k] + ((double)lo[k] + (double)hi[k]) * wj;
          if (j == 1) break;
          lo[0] = lo[1]; lo[1] = lo[2]; lo[2] = lo[3];
          lo[3] = col[row_of(gy0 + 3 - (j - 1))];
          hi[3] = hi[2]; hi[2] = hi[1]; hi[1] = hi[0];
          hi[0] = col[row_of(gy0 + (j - 1))];
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (row0 + k < rows) mid[(row0 + k) * kMidW + c] = (float)acc[k];
    }
  }
  __syncthreads();

  // 2. W pass from LDS, four rows per wave again, the stores and the running maximum
  uint32_t kmax = 0u;                                    // below every key a float maps to
  float* __restrict__ dst = out + (size_t)img * plane;
  if (row0 < rows) {
    for (int c = lane; c < cols; c += 64) {
      const float* m = mid + row0 * kMidW + r + c;
      double acc[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[k] = (double)m[k * kMidW] * w0;
      for (int j = r; j >= 1; --j) {                      // farthest tap first, as scipy
        const double wj = wt.w[j];
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = acc[k] + ((double)m[k * kMidW - j] + (double)m[k * kMidW + j]) * wj;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (row0 + k < rows) {                           // rows past the image end hold no H-pass result
          const float v = (float)acc[k];
          dst[(size_t)(y0 + row0 + k) * W + x0 + c] = v;
          kmax = std::max(kmax, order_key(v));
        }
      }
    }
  }
  if (max_key != nullptr) {
    kmax = wave_max_u32(kmax);
    if (lane == 0) wave_max[wv] = kmax;
    __syncthreads();
    if (threadIdx.x == 0) {
      const uint32_t k = std::max(std::max(wave_max[0], wave_max[1]), std::max(wave_max[2], wave_max[3]));
      atomicMax(max_key + img, k);
    }
  }
}

int smooth_check_shape(const char* who, int n_img, int H, int W, int radius) {
  SRAD_REQUIRE(n_img >= 1 && H >= 1 && W >= 1 && (int64_t)n_img * H * W < ((int64_t)1 << 31),
               "%s: n_img x H x W = %d x %d x %d, each must be >= 1 and the product below 2^31", who, n_img, H, W);
  SRAD_REQUIRE(radius >= 0 && radius <= kMaxRadius, "%s: radius %d, must be in [0, %d]", who, radius, kMaxRadius);
  SRAD_REQUIRE(radius <= std::min(H, W), "%s: radius %d of a %dx%d map needs more than one reflection", who, radius, H, W);
  return SRAD_OK;
}

}  // namespace

extern "C" {

int srad_smooth_maps_workspace_bytes(int n_img, int H, int W, int radius, size_t* bytes) {
  SRAD_REQUIRE(bytes, "smooth_maps_workspace_bytes: bytes is NULL");
  SRAD_TRY(smooth_check_shape("smooth_maps_workspace_bytes", n_img, H, W, radius));
  *bytes = map_max_workspace_bytes(n_img);
  return SRAD_OK;
}

int srad_smooth_maps(const float* maps, int n_img, int H, int W, const double* weights_host, int radius, float* out,
                     float* img_max_out, void* workspace, size_t workspace_bytes, void* stream) {
  SRAD_REQUIRE(maps && out && weights_host && workspace, "smooth_maps: NULL maps, out, weights_host or workspace");
  SRAD_TRY(smooth_check_shape("smooth_maps", n_img, H, W, radius));
  const size_t n = (size_t)n_img * H * W;
  const uintptr_t a = reinterpret_cast<uintptr_t>(maps), b = reinterpret_cast<uintptr_t>(out);
  SRAD_REQUIRE(b + n * sizeof(float) <= a || a + n * sizeof(float) <= b, "smooth_maps: out overlaps maps");
  size_t need = 0;
  SRAD_TRY(srad_smooth_maps_workspace_bytes(n_img, H, W, radius, &need));
  SRAD_REQUIRE(workspace_bytes >= need, "smooth_maps: workspace %zu bytes, %zu needed", workspace_bytes, need);
  SmoothWeights wt{};
  for (int j = 0; j <= radius; ++j) wt.w[j] = weights_host[j];
  if (radius == 0) wt.w[0] = 1.0;                        // radius 0 copies: x * 1.0 == x for every float, NaN included
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  uint32_t* keys = img_max_out ? reinterpret_cast<uint32_t*>(workspace) : nullptr;
  if (keys) SRAD_CHECK_HIP(map_max_begin(keys, n_img, s));
  const int tiles_x = (W + kTileW - 1) / kTileW, tiles_y = (H + kTileH - 1) / kTileH;
  {
    // fp64 operations: 3 per tap and one for the centre, in the H pass for the halo columns too; bytes: read once, written once
    const double h_pass = (double)n_img * H * ((double)W + 2.0 * radius * tiles_x);
    SradProfScope prof(s, SRAD_K_SCORE, (3.0 * radius + 1.0) * (h_pass + (double)n), 8.0 * n);
    hipLaunchKernelGGL(smooth_maps_kernel, dim3((unsigned)((size_t)n_img * tiles_y * tiles_x)), dim3(256), 0, s, maps, out, keys,
                       H, W, radius, tiles_x, tiles_y, wt);
  }
  if (keys) map_max_finish(keys, img_max_out, n_img, s);
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

}  // extern "C"
