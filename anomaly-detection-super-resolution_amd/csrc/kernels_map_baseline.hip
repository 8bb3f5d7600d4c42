// kernels_map_baseline.hip - the per-pixel baseline of anomaly maps (DESIGN.md "Baseline"): the fp64 sums of defect-free maps
// (srad_map_stats_accumulate), the z-scores of maps against fitted planes (srad_map_normalize) and the leave-one-out z-scores
// of the maps the sums were made of (srad_map_normalize_loo).  include/srad.h has the definitions; this file follows them
// literally, one IEEE operation per operation of the definition: it is compiled without FMA contraction, the fp64 division
// and square root are the plain `/` and sqrt(), which this build rounds correctly, and the two maxima of the leave-one-out
// form are written as comparisons that keep a NaN, as numpy's maximum does.
//
// All three kernels are byte movers: one thread per four consecutive pixels of the flattened plane with 16-byte loads and
// stores (float4 maps, double2 sums) where H * W is a multiple of four and every pointer sits on 16 bytes, else the scalar
// instance; grid-stride, at most about 2048 workgroups.  No LDS, no private memory, no float atomics.
//   accumulate: a thread walks the images of its pixels, four images' loads issued before their dependent adds, the adds in
//               image order; the two sum planes are read and written once per call.
//   normalize : grid (plane, image): the planes (8 B per pixel, or 16 B of sums) are re-read per image and stay in the cache.
//               The per-image maximum goes the way of smooth_maps_kernel (map_max.h): a wave reduction of order_key and one
//               u32 atomicMax per wave - into one of kMaxSlots keys per image, each on a 64-byte line of its own, and only
//               where the wave's key is above what the slot already holds: with one key per image the waves of a 1024 px
//               map queued on one address for 25 times the kernel's own time.  out == maps is allowed: a thread reads its
//               pixels before it writes them.
#include "engine.h"
#include "../../include/srad.h"
#include "map_max.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int kMaxBlocks = 2048;
constexpr int kImgUnroll = 4;                              // images in flight per thread of the accumulation
constexpr int kMaxSlots = 16, kMaxStride = 16;             // keys per image of the maximum, and their distance in u32 (64 bytes)

template <int VEC>
__device__ __forceinline__ void load_f(const float* p, float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    const f32x4 q = *reinterpret_cast<const f32x4*>(p);
    v[0] = q[0], v[1] = q[1], v[2] = q[2], v[3] = q[3];
  } else {
    v[0] = *p;
  }
}
template <int VEC>
__device__ __forceinline__ void store_f(float* p, const float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    f32x4 q;
    q[0] = v[0], q[1] = v[1], q[2] = v[2], q[3] = v[3];
    *reinterpret_cast<f32x4*>(p) = q;
  } else {
    *p = v[0];
  }
}
template <int VEC>
__device__ __forceinline__ void load_d(const double* p, double (&v)[VEC]) {
  if constexpr (VEC == 4) {
    const double2 a = *reinterpret_cast<const double2*>(p), b = *reinterpret_cast<const double2*>(p + 2);
    v[0] = a.x, v[1] = a.y, v[2] = b.x, v[3] = b.y;
  } else {
    v[0] = *p;
  }
}
template <int VEC>
__device__ __forceinline__ void store_d(double* p, const double (&v)[VEC]) {
  if constexpr (VEC == 4) {
    *reinterpret_cast<double2*>(p) = make_double2(v[0], v[1]);
    *reinterpret_cast<double2*>(p + 2) = make_double2(v[2], v[3]);
  } else {
    *p = v[0];
  }
}

// s1 += sum_i m_i, s2 += sum_i m_i * m_i per pixel, sequentially in image order; `groups` = plane / VEC
template <int VEC>
__global__ __launch_bounds__(256) void map_stats_kernel(const float* __restrict__ maps, double* __restrict__ s1,
                                                        double* __restrict__ s2, int n_img, size_t plane, size_t groups) {
  for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (size_t)gridDim.x * 256) {
    const size_t px = g * VEC;
    double a[VEC], b[VEC];
    load_d<VEC>(s1 + px, a);
    load_d<VEC>(s2 + px, b);
    const float* __restrict__ p = maps + px;
    int i = 0;
    for (; i + kImgUnroll <= n_img; i += kImgUnroll) {
      float v[kImgUnroll][VEC];
#pragma unroll
      for (int k = 0; k < kImgUnroll; ++k) load_f<VEC>(p + (size_t)(i + k) * plane, v[k]);
#pragma unroll
      for (int k = 0; k < kImgUnroll; ++k) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          const double x = (double)v[k][e];
          a[e] = a[e] + x;
          b[e] = b[e] + x * x;                            // the product of two floats is exact in double
        }
      }
    }
    for (; i < n_img; ++i) {
      float v[VEC];
      load_f<VEC>(p + (size_t)i * plane, v);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const double x = (double)v[e];
        a[e] = a[e] + x;
        b[e] = b[e] + x * x;
      }
    }
    store_d<VEC>(s1 + px, a);
    store_d<VEC>(s2 + px, b);
  }
}

struct NormPlanes {
  const float *mu, *inv_sd;                                // apply
  const double *s1, *s2;                                   // leave-one-out
  double nm1, nm2, floor;                                  // N - 1, N - 2, the fitted floor
};

// blockIdx.x strides over the plane's pixel groups, blockIdx.y over the images.  maps and out may be the same pointer.
template <int VEC, bool LOO>
__global__ __launch_bounds__(256) void map_normalize_kernel(const float* maps, float* out, uint32_t* __restrict__ max_key,
                                                            NormPlanes pl, int n_img, size_t plane, size_t groups) {
  for (int img = blockIdx.y; img < n_img; img += gridDim.y) {
    const float* src = maps + (size_t)img * plane;
    float* dst = out + (size_t)img * plane;
    uint32_t kmax = 0u;                                    // below every key a float maps to
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (size_t)gridDim.x * 256) {
      const size_t px = g * VEC;
      float m[VEC], z[VEC];
      load_f<VEC>(src + px, m);
      if constexpr (LOO) {
        double s1[VEC], s2[VEC];
        load_d<VEC>(pl.s1 + px, s1);
        load_d<VEC>(pl.s2 + px, s2);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          const double x = (double)m[e];
          const double a = s1[e] - x;
          const double q = s2[e] - x * x;
          const double mean = a / pl.nm1;
          double t = q - a * a / pl.nm1;
          t = t < 0.0 ? 0.0 : t;                           // max(t, 0) that keeps a NaN
          const double var = t / pl.nm2;
          double sd = sqrt(var);
          sd = sd < pl.floor ? pl.floor : sd;              // max(sd, floor) that keeps a NaN
          z[e] = (float)((x - mean) / sd);
        }
      } else {
        float mu[VEC], inv[VEC];
        load_f<VEC>(pl.mu + px, mu);
        load_f<VEC>(pl.inv_sd + px, inv);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          const float d = m[e] - mu[e];
          z[e] = d * inv[e];
        }
      }
      store_f<VEC>(dst + px, z);
#pragma unroll
      for (int e = 0; e < VEC; ++e) kmax = std::max(kmax, order_key(z[e]));
    }
    if (max_key != nullptr) {                              // every lane of the wave is here: the loops have no early exit
      kmax = wave_max_u32(kmax);
      if ((threadIdx.x & 63) == 0) {
        uint32_t* slot = max_key + ((size_t)img * kMaxSlots + ((blockIdx.x * 4u + (threadIdx.x >> 6)) & (kMaxSlots - 1))) * kMaxStride;
        // a stale read only costs an atomic: the slot never decreases, so a key at or below what was read changes nothing
        if (kmax > *(volatile uint32_t*)slot) atomicMax(slot, kmax);
      }
    }
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int baseline_check_shape(const char* who, int n_img, int H, int W) {
  SRAD_REQUIRE(n_img >= 1 && H >= 1 && W >= 1 && (int64_t)n_img * H * W < ((int64_t)1 << 31),
               "%s: n_img x H x W = %d x %d x %d, each must be >= 1 and the product below 2^31", who, n_img, H, W);
  return SRAD_OK;
}

bool bytes_overlap(const void* p, size_t np, const void* q, size_t nq) { return srad_byte_ranges_overlap(p, np, q, nq); }

unsigned blocks_x(size_t groups) {
  const size_t b = (groups + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > (size_t)kMaxBlocks ? (size_t)kMaxBlocks : b));
}

// the launch shared by the two normalisations, after their own argument checks
template <bool LOO>
int normalize_launch(const char* who, const float* maps, int n_img, int H, int W, const NormPlanes& pl, float* out,
                     float* img_max_out, void* workspace, size_t workspace_bytes, void* stream) {
  const size_t plane = (size_t)H * W, n = plane * n_img;
  SRAD_REQUIRE(out == maps || !srad_ranges_overlap(maps, n, out, n), "%s: out overlaps maps (only out == maps is allowed)", who);
  uint32_t* keys = nullptr;
  if (img_max_out) {
    SRAD_REQUIRE(workspace, "%s: NULL workspace with img_max_out set", who);
    const size_t need = map_max_workspace_bytes(n_img, kMaxSlots, kMaxStride);
    SRAD_REQUIRE(workspace_bytes >= need, "%s: workspace %zu bytes, %zu needed", who, workspace_bytes, need);
    SRAD_REQUIRE(!bytes_overlap(img_max_out, (size_t)n_img * 4, out, n * 4) && !bytes_overlap(img_max_out, (size_t)n_img * 4, maps, n * 4),
                 "%s: img_max_out overlaps the maps", who);
    keys = reinterpret_cast<uint32_t*>(workspace);
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (keys) SRAD_CHECK_HIP(map_max_begin(keys, n_img, s, kMaxSlots, kMaxStride));
  const bool vec = plane % 4 == 0 && aligned16(maps) && aligned16(out) &&
                   (LOO ? aligned16(pl.s1) && aligned16(pl.s2) : aligned16(pl.mu) && aligned16(pl.inv_sd));
  const size_t groups = vec ? plane / 4 : plane;
  const unsigned bx = blocks_x(keys ? (groups + 3) / 4 : groups);       // with the maximum: four rounds per thread, a quarter of the atomics
  const unsigned by = (unsigned)std::max(1, std::min(n_img, kMaxBlocks / (int)bx));
  {
    // bytes: each map read and written once; the planes count once, the re-reads hit the cache
    SradProfScope prof(s, SRAD_K_SCORE, (LOO ? 12.0 : 2.0) * n, 8.0 * n + (LOO ? 16.0 : 8.0) * plane);
    if (vec) hipLaunchKernelGGL((map_normalize_kernel<4, LOO>), dim3(bx, by), dim3(256), 0, s, maps, out, keys, pl, n_img, plane, groups);
    else hipLaunchKernelGGL((map_normalize_kernel<1, LOO>), dim3(bx, by), dim3(256), 0, s, maps, out, keys, pl, n_img, plane, groups);
  }
  if (keys) map_max_finish(keys, img_max_out, n_img, s, kMaxSlots, kMaxStride);
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

}  // namespace

extern "C" {

int srad_map_stats_accumulate(const float* maps, int n_img, int H, int W, double* s1, double* s2, void* stream) {
  SRAD_REQUIRE(maps && s1 && s2, "map_stats_accumulate: NULL maps, s1 or s2");
  SRAD_TRY(baseline_check_shape("map_stats_accumulate", n_img, H, W));
  const size_t plane = (size_t)H * W, n = plane * n_img;
  SRAD_REQUIRE(!bytes_overlap(s1, plane * 8, s2, plane * 8) && !bytes_overlap(maps, n * 4, s1, plane * 8) &&
               !bytes_overlap(maps, n * 4, s2, plane * 8), "map_stats_accumulate: maps, s1 and s2 overlap");
  const bool vec = plane % 4 == 0 && aligned16(maps) && aligned16(s1) && aligned16(s2);
  const size_t groups = vec ? plane / 4 : plane;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  SradProfScope prof(s, SRAD_K_SCORE, 3.0 * n, 4.0 * n + 32.0 * plane);
  if (vec) hipLaunchKernelGGL(map_stats_kernel<4>, dim3(blocks_x(groups)), dim3(256), 0, s, maps, s1, s2, n_img, plane, groups);
  else hipLaunchKernelGGL(map_stats_kernel<1>, dim3(blocks_x(groups)), dim3(256), 0, s, maps, s1, s2, n_img, plane, groups);
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

int srad_map_normalize_workspace_bytes(int n_img, size_t* bytes) {
  SRAD_REQUIRE(bytes, "map_normalize_workspace_bytes: bytes is NULL");
  SRAD_REQUIRE(n_img >= 1, "map_normalize_workspace_bytes: n_img = %d, must be >= 1", n_img);
  *bytes = map_max_workspace_bytes(n_img, kMaxSlots, kMaxStride);
  return SRAD_OK;
}

int srad_map_normalize(const float* maps, int n_img, int H, int W, const float* mu, const float* inv_sd, float* out,
                       float* img_max_out, void* workspace, size_t workspace_bytes, void* stream) {
  SRAD_REQUIRE(maps && mu && inv_sd && out, "map_normalize: NULL maps, mu, inv_sd or out");
  SRAD_TRY(baseline_check_shape("map_normalize", n_img, H, W));
  const size_t plane = (size_t)H * W, n = plane * n_img;
  SRAD_REQUIRE(!srad_ranges_overlap(mu, plane, out, n) && !srad_ranges_overlap(inv_sd, plane, out, n),
               "map_normalize: out overlaps mu or inv_sd");
  const NormPlanes pl = {mu, inv_sd, nullptr, nullptr, 0.0, 0.0, 0.0};
  return normalize_launch<false>("map_normalize", maps, n_img, H, W, pl, out, img_max_out, workspace, workspace_bytes, stream);
}

int srad_map_normalize_loo(const float* maps, int n_img, int H, int W, const double* s1, const double* s2, int n_total,
                           double floor, float* out, float* img_max_out, void* workspace, size_t workspace_bytes, void* stream) {
  SRAD_REQUIRE(maps && s1 && s2 && out, "map_normalize_loo: NULL maps, s1, s2 or out");
  SRAD_TRY(baseline_check_shape("map_normalize_loo", n_img, H, W));
  SRAD_REQUIRE(n_total >= 3, "map_normalize_loo: n_total = %d, leave-one-out needs at least 3 images in the sums", n_total);
  SRAD_REQUIRE(floor > 0.0 && floor <= 1.7976931348623157e308, "map_normalize_loo: floor = %g, must be finite and > 0", floor);
  const size_t plane = (size_t)H * W, n = plane * n_img;
  SRAD_REQUIRE(!bytes_overlap(s1, plane * 8, out, n * 4) && !bytes_overlap(s2, plane * 8, out, n * 4),
               "map_normalize_loo: out overlaps s1 or s2");
  const NormPlanes pl = {nullptr, nullptr, s1, s2, (double)(n_total - 1), (double)(n_total - 2), floor};
  return normalize_launch<true>("map_normalize_loo", maps, n_img, H, W, pl, out, img_max_out, workspace, workspace_bytes, stream);
}

}  // extern "C"
