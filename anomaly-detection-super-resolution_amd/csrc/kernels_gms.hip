// kernels_gms.hip - gradient-magnitude similarity (GMSD, Xue et al. 2014; multi-scale as in RIAD, Zavrtanik et al. 2021):
// the per-pixel maps of the evaluator (srad_gms_maps, include/srad.h states the definition) and the loss kinds GMS / MSGMS
// with their gradient.  Memory-bound small-stencil work: no LDS in the map kernels, no atomics anywhere (the backward is a
// gather, so gradients are bit-reproducible).
//
// Maps: exact integers up to M = Gx^2 + Gy^2 (int64), then about 20 float64 operations and ONE rounding to fp32 per pixel.
//   gms_pyramid_kernel  u8 -> the int32 channel-sum planes of levels 1 .. L-1, both stacks (one thread per coarsest cell)
//   gms_level_kernel    the float64 planes d_l of levels 1 .. L-1 (21/64 of a plane in all)
//   gms_map_kernel      per output pixel: level 0 straight from the u8 stacks, the bilinear taps of the coarser planes, one store
// Loss (fp32): gms_loss_planes_kernel (clamped channel means and their 2x2-average pyramids), gms_loss_d_kernel (d per pixel
// of every level, block partial sums, the planes dd/dGx_a and dd/dGy_a), gms_loss_grad_kernel (per level-0 pixel: the adjoint
// of the reflect-padded Prewitt taps at every level, down the pool chain, out to the channels through the clamp).
#include "../../include/srad.h"
#include "srad_common.h"
#include "gms_loss.h"
#include <algorithm>
#include <math.h>

#pragma clang fp contract(off)     // every operation of the definition is one IEEE operation

namespace {

constexpr int kMaxLevels = 4;
constexpr double kGmsC = 0.0026;   // GMSD's 170 / 255^2, for gradient magnitudes in [0, 1] units

// numpy "reflect" by one pixel: -1 -> 1, n -> n - 2 (n >= 2); any other index is inside
__device__ __forceinline__ int reflect1(int i, int n) { return i < 0 ? 1 : (i >= n ? n - 2 : i); }

// The eight outer taps of the reflect-padded 3 x 3 neighbourhood of (y, x) in an h x w plane, as tap-pair differences.
template <class T, class At>
__device__ __forceinline__ void prewitt_sums(At at, int y, int x, int h, int w, T& gx, T& gy) {
  const int ym = reflect1(y - 1, h), yp = reflect1(y + 1, h), xm = reflect1(x - 1, w), xp = reflect1(x + 1, w);
  const T a = at(ym, xm), b = at(ym, x), c = at(ym, xp), d = at(y, xm), e = at(y, xp), f = at(yp, xm), g = at(yp, x), k = at(yp, xp);
  gx = ((c - a) + (e - d)) + (k - f);
  gy = ((f - a) + (g - b)) + (k - c);
}

// ---- maps --------------------------------------------------------------------------------------------------------
struct GmsMapGeo {
  int n, H, W;
  int32_t* ssr[kMaxLevels];      // channel-sum planes [n][H >> l][W >> l]; entry 0 unused (level 0 is read from the u8 stacks)
  int32_t* shr[kMaxLevels];
  double* d[kMaxLevels];         // d_l planes, entry 0 unused
  double ck2[kMaxLevels];        // 0.0026 * K_l^2, K_l = 3 * C * 255 * 4^l
};

template <int C>
__device__ __forceinline__ int chan_sum(const uint8_t* p) {
  if constexpr (C == 1) return p[0];
  else return (int)p[0] + (int)p[1] + (int)p[2];
}

// the block sum of level LV at cell (y, x) of one image; stores it (LV >= 1) and every finer level's sums on the way
template <int LV, int C>
__device__ __forceinline__ int pyramid_cell(const uint8_t* __restrict__ img, const GmsMapGeo& g, bool hr, int i, int y, int x) {
  if constexpr (LV == 0) {
    return chan_sum<C>(img + ((size_t)y * g.W + x) * C);
  } else {
    const int s = (pyramid_cell<LV - 1, C>(img, g, hr, i, 2 * y, 2 * x) + pyramid_cell<LV - 1, C>(img, g, hr, i, 2 * y, 2 * x + 1)) +
                  (pyramid_cell<LV - 1, C>(img, g, hr, i, 2 * y + 1, 2 * x) + pyramid_cell<LV - 1, C>(img, g, hr, i, 2 * y + 1, 2 * x + 1));
    const int h = g.H >> LV, w = g.W >> LV;
    (hr ? g.shr[LV] : g.ssr[LV])[((size_t)i * h + y) * w + x] = s;
    return s;
  }
}

// grid (cells of level L-1 over all images / 256, 2): blockIdx.y picks the stack
template <int C, int L>
__global__ __launch_bounds__(256) void gms_pyramid_kernel(const uint8_t* __restrict__ sr, const uint8_t* __restrict__ hr, GmsMapGeo g) {
  const int h = g.H >> (L - 1), w = g.W >> (L - 1);
  const size_t t = blockIdx.x * (size_t)256 + threadIdx.x;
  if (t >= (size_t)g.n * h * w) return;
  const int i = (int)(t / ((size_t)h * w));
  const int p = (int)(t - (size_t)i * h * w);
  const bool is_hr = blockIdx.y != 0;
  const uint8_t* img = (is_hr ? hr : sr) + (size_t)i * g.H * g.W * C;
  pyramid_cell<L - 1, C>(img, g, is_hr, i, p / w, p % w);
}

__device__ __forceinline__ int64_t prewitt_sq_i32(const int32_t* __restrict__ P, int y, int x, int h, int w) {
  int gx, gy;
  prewitt_sums<int>([&](int yy, int xx) { return P[(size_t)yy * w + xx]; }, y, x, h, w, gx, gy);
  return (int64_t)gx * gx + (int64_t)gy * gy;
}

__device__ __forceinline__ double gms_d(int64_t Ma, int64_t Mb, double ck2) {
  const double r = sqrt((double)Ma) - sqrt((double)Mb);
  return (r * r) / ((double)(Ma + Mb) + ck2);
}

// one thread per cell of the levels 1 .. L-1 of all images, level 1 first
template <int L>
__global__ __launch_bounds__(256) void gms_level_kernel(GmsMapGeo g) {
  size_t t = blockIdx.x * (size_t)256 + threadIdx.x;
  static_for<1, L>([&](auto lv) {
    constexpr int LV = decltype(lv)::value;
    const int h = g.H >> LV, w = g.W >> LV;
    const size_t cells = (size_t)g.n * h * w;
    if (t < cells) {
      const int i = (int)(t / ((size_t)h * w));
      const int p = (int)(t - (size_t)i * h * w);
      const size_t o = (size_t)i * h * w;
      const int64_t Ma = prewitt_sq_i32(g.ssr[LV] + o, p / w, p % w, h, w);
      const int64_t Mb = prewitt_sq_i32(g.shr[LV] + o, p / w, p % w, h, w);
      g.d[LV][t] = gms_d(Ma, Mb, g.ck2[LV]);
    }
    t -= cells;        // wraps past the last level for a thread that has done its cell: it matches no later level
  });
}

// bilinear sample (align_corners = False) of the hl x wl plane D at output pixel (y, x); inv_f = 1 / 2^l
__device__ __forceinline__ double bilinear_at(const double* __restrict__ D, int hl, int wl, int y, int x, double inv_f) {
  const double oy = ((double)y + 0.5) * inv_f - 0.5, ox = ((double)x + 0.5) * inv_f - 0.5;
  const double fy = floor(oy), fx = floor(ox);
  const double ty = oy - fy, tx = ox - fx;
  const int i0 = min(max((int)fy, 0), hl - 1), i1 = min(max((int)fy + 1, 0), hl - 1);
  const int j0 = min(max((int)fx, 0), wl - 1), j1 = min(max((int)fx + 1, 0), wl - 1);
  const double d00 = D[(size_t)i0 * wl + j0], d01 = D[(size_t)i0 * wl + j1], d10 = D[(size_t)i1 * wl + j0], d11 = D[(size_t)i1 * wl + j1];
  return (d00 * (1.0 - tx) + d01 * tx) * (1.0 - ty) + (d10 * (1.0 - tx) + d11 * tx) * ty;
}

template <int C>
__device__ __forceinline__ int64_t prewitt_sq_u8(const uint8_t* __restrict__ img, int y, int x, int H, int W) {
  int gx, gy;
  prewitt_sums<int>([&](int yy, int xx) { return chan_sum<C>(img + ((size_t)yy * W + xx) * C); }, y, x, H, W, gx, gy);
  return (int64_t)gx * gx + (int64_t)gy * gy;
}

template <int C, int L>
__global__ __launch_bounds__(256) void gms_map_kernel(const uint8_t* __restrict__ sr, const uint8_t* __restrict__ hr, GmsMapGeo g,
                                                      float* __restrict__ map_out, double inv_levels) {
  const size_t t = blockIdx.x * (size_t)256 + threadIdx.x;
  const size_t plane = (size_t)g.H * g.W;
  if (t >= (size_t)g.n * plane) return;
  const int i = (int)(t / plane);
  const int p = (int)(t - (size_t)i * plane);
  const int y = p / g.W, x = p - y * g.W;
  const size_t img = (size_t)i * plane * C;
  double acc = gms_d(prewitt_sq_u8<C>(sr + img, y, x, g.H, g.W), prewitt_sq_u8<C>(hr + img, y, x, g.H, g.W), g.ck2[0]);
  static_for<1, L>([&](auto lv) {
    constexpr int LV = decltype(lv)::value;
    const int hl = g.H >> LV, wl = g.W >> LV;
    acc = acc + bilinear_at(g.d[LV] + (size_t)i * hl * wl, hl, wl, y, x, 1.0 / (double)(1 << LV));
  });
  map_out[t] = (float)(acc * inv_levels);
}

int gms_map_geometry(const char* what, int n_img, int H, int W, int levels) {
  SRAD_REQUIRE(levels >= 1 && levels <= kMaxLevels, "%s: levels must be 1..4 (got %d)", what, levels);
  SRAD_REQUIRE(n_img > 0 && H > 0 && W > 0, "%s: bad argument", what);
  const int f = 1 << (levels - 1);
  SRAD_REQUIRE(H % f == 0 && W % f == 0 && (H >> (levels - 1)) >= 2 && (W >> (levels - 1)) >= 2,
               "%s: %d levels need H and W to be multiples of %d and at least %d (got %dx%d)", what, levels, f, 2 * f, H, W);
  SRAD_REQUIRE(((size_t)n_img * H * W + 255) / 256 < (1ull << 31), "%s: %d %dx%d images are too many pixels for one launch", what, n_img, H, W);
  return SRAD_OK;
}

// the workspace of the levels 1 .. L-1: per level two int32 planes and one float64 plane per image
size_t gms_map_layout(int n_img, int H, int W, int C, int levels, void* workspace, GmsMapGeo* g) {
  char* base = reinterpret_cast<char*>(workspace);
  size_t off = 0;
  if (g) { g->n = n_img; g->H = H; g->W = W; }
  for (int l = 0; l < kMaxLevels; ++l) {
    if (g) {
      g->ssr[l] = g->shr[l] = nullptr; g->d[l] = nullptr;
      const double K = 3.0 * C * 255.0 * (double)(1 << (2 * l));
      g->ck2[l] = kGmsC * K * K;
    }
    if (l == 0 || l >= levels) continue;
    const size_t cells = (size_t)n_img * (H >> l) * (W >> l);
    const size_t si = srad_align_up(cells * sizeof(int32_t), 256), sd = srad_align_up(cells * sizeof(double), 256);
    if (g) {
      g->ssr[l] = reinterpret_cast<int32_t*>(base + off);
      g->shr[l] = reinterpret_cast<int32_t*>(base + off + si);
      g->d[l] = reinterpret_cast<double*>(base + off + 2 * si);
    }
    off += 2 * si + sd;
  }
  return std::max<size_t>(off, 256);
}

template <int C>
void launch_gms_maps(const uint8_t* sr, const uint8_t* hr, const GmsMapGeo& g, int levels, float* map_out, hipStream_t s) {
  const size_t npix = (size_t)g.n * g.H * g.W;
  const dim3 grid((unsigned)((npix + 255) / 256));
  const double inv_levels = 1.0 / (double)levels;
  size_t coarse = 0;
  for (int l = 1; l < levels; ++l) coarse += (size_t)g.n * (g.H >> l) * (g.W >> l);
  const dim3 pgrid((unsigned)(((size_t)g.n * (g.H >> (levels - 1)) * (g.W >> (levels - 1)) + 255) / 256), 2);
  const dim3 lgrid((unsigned)((coarse + 255) / 256));
  switch (levels) {
    case 1:
      hipLaunchKernelGGL((gms_map_kernel<C, 1>), grid, dim3(256), 0, s, sr, hr, g, map_out, inv_levels);
      break;
    case 2:
      hipLaunchKernelGGL((gms_pyramid_kernel<C, 2>), pgrid, dim3(256), 0, s, sr, hr, g);
      hipLaunchKernelGGL(gms_level_kernel<2>, lgrid, dim3(256), 0, s, g);
      hipLaunchKernelGGL((gms_map_kernel<C, 2>), grid, dim3(256), 0, s, sr, hr, g, map_out, inv_levels);
      break;
    case 3:
      hipLaunchKernelGGL((gms_pyramid_kernel<C, 3>), pgrid, dim3(256), 0, s, sr, hr, g);
      hipLaunchKernelGGL(gms_level_kernel<3>, lgrid, dim3(256), 0, s, g);
      hipLaunchKernelGGL((gms_map_kernel<C, 3>), grid, dim3(256), 0, s, sr, hr, g, map_out, inv_levels);
      break;
    default:
      hipLaunchKernelGGL((gms_pyramid_kernel<C, 4>), pgrid, dim3(256), 0, s, sr, hr, g);
      hipLaunchKernelGGL(gms_level_kernel<4>, lgrid, dim3(256), 0, s, g);
      hipLaunchKernelGGL((gms_map_kernel<C, 4>), grid, dim3(256), 0, s, sr, hr, g, map_out, inv_levels);
      break;
  }
}

// ---- loss --------------------------------------------------------------------------------------------------------
constexpr int kLossNb = 1024;      // block partial sums of the forward, as kernels_loss.hip's LOSS_NB

struct GmsLossGeo {
  int B, C, H, W;
  float inv_range;
  float* xa[kMaxLevels];          // sr: the clamped channel mean (level 0) and its 2x2 averages, [B][H >> l][W >> l]
  float* xb[kMaxLevels];          // hr likewise
  float* pa[kMaxLevels];          // level weight * dd/dGx_a (Gx = the tap sum before the division by 3)
  float* qa[kMaxLevels];          // level weight * dd/dGy_a
  double wl[kMaxLevels];          // 1 / (L * B * h_l * w_l)
};

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

template <int LV>
__device__ __forceinline__ float loss_pyramid_cell(const float* __restrict__ t, const GmsLossGeo& g, bool hr, int b, int y, int x) {
  float v;
  if constexpr (LV == 0) {
    const size_t plane = (size_t)g.H * g.W;
    const float* p = t + (size_t)b * g.C * plane + (size_t)y * g.W + x;
    if (g.C == 1) v = clamp01(p[0] * g.inv_range);
    else v = ((clamp01(p[0] * g.inv_range) + clamp01(p[plane] * g.inv_range)) + clamp01(p[2 * plane] * g.inv_range)) * (1.0f / 3.0f);
  } else {
    v = ((loss_pyramid_cell<LV - 1>(t, g, hr, b, 2 * y, 2 * x) + loss_pyramid_cell<LV - 1>(t, g, hr, b, 2 * y, 2 * x + 1)) +
         (loss_pyramid_cell<LV - 1>(t, g, hr, b, 2 * y + 1, 2 * x) + loss_pyramid_cell<LV - 1>(t, g, hr, b, 2 * y + 1, 2 * x + 1))) * 0.25f;
  }
  const int h = g.H >> LV, w = g.W >> LV;
  (hr ? g.xb[LV] : g.xa[LV])[((size_t)b * h + y) * w + x] = v;
  return v;
}

// grid (cells of level L-1 over the batch / 256, 2): blockIdx.y picks sr or hr
template <int L>
__global__ __launch_bounds__(256) void gms_loss_planes_kernel(const float* __restrict__ sr, const float* __restrict__ hr, GmsLossGeo g) {
  const int h = g.H >> (L - 1), w = g.W >> (L - 1);
  const size_t t = blockIdx.x * (size_t)256 + threadIdx.x;
  if (t >= (size_t)g.B * h * w) return;
  const int b = (int)(t / ((size_t)h * w));
  const int p = (int)(t - (size_t)b * h * w);
  const bool is_hr = blockIdx.y != 0;
  loss_pyramid_cell<L - 1>(is_hr ? hr : sr, g, is_hr, b, p / w, p % w);
}

__device__ __forceinline__ void prewitt_f32(const float* __restrict__ P, int y, int x, int h, int w, float& gx, float& gy) {
  prewitt_sums<float>([&](int yy, int xx) { return P[(size_t)yy * w + xx]; }, y, x, h, w, gx, gy);
}

// per pixel of every level: d, its weighted share of the loss into the block partial sums, and the two derivative planes
template <int L>
__global__ __launch_bounds__(256) void gms_loss_d_kernel(GmsLossGeo g, double* __restrict__ partial) {
  __shared__ double red[256];
  size_t total = 0;
  static_for<0, L>([&](auto lv) { total += (size_t)g.B * (g.H >> decltype(lv)::value) * (g.W >> decltype(lv)::value); });
  double local = 0.0;
  for (size_t t0 = blockIdx.x * (size_t)256 + threadIdx.x; t0 < total; t0 += (size_t)gridDim.x * 256) {
    size_t t = t0;
    static_for<0, L>([&](auto lv) {
      constexpr int LV = decltype(lv)::value;
      const int h = g.H >> LV, w = g.W >> LV;
      const size_t cells = (size_t)g.B * h * w;
      if (t < cells) {
        const int b = (int)(t / ((size_t)h * w));
        const int p = (int)(t - (size_t)b * h * w);
        const size_t o = (size_t)b * h * w;
        float Gxa, Gya, Gxb, Gyb;
        prewitt_f32(g.xa[LV] + o, p / w, p % w, h, w, Gxa, Gya);
        prewitt_f32(g.xb[LV] + o, p / w, p % w, h, w, Gxb, Gyb);
        const float third = 1.0f / 3.0f;
        const float gxa = Gxa * third, gya = Gya * third, gxb = Gxb * third, gyb = Gyb * third;
        const float Ma = gxa * gxa + gya * gya, Mb = gxb * gxb + gyb * gyb;
        const float ga = sqrtf(Ma), gb = sqrtf(Mb);
        const float r = ga - gb, D = (Ma + Mb) + (float)kGmsC;
        local += (double)((r * r) / D) * g.wl[LV];
        // dd/dgx_a = 2 r gx_a (Mb + c + ga gb) / (ga D^2): every factor of the bracket is >= 0, nothing cancels; 0 where Ma == 0
        const float k = Ma > 0.0f ? (2.0f * r * ((Mb + (float)kGmsC) + ga * gb)) / (ga * D * D) * (third * (float)g.wl[LV]) : 0.0f;
        g.pa[LV][t] = k * gxa;
        g.qa[LV][t] = k * gya;
      }
      t -= cells;
    });
  }
  const double s = srad_block_sum(local, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ void gms_loss_finish_kernel(const double* __restrict__ partial, int nb, double* __restrict__ out2) {
  if (threadIdx.x || blockIdx.x) return;
  double s = 0.0;
  for (int i = 0; i < nb; ++i) s += partial[i];
  out2[0] = s;
  out2[1] = s;
}

// d loss / d x_LV[b, y, x] from level LV's own term: the adjoint of the Prewitt tap sums on the padded plane, folded back
// through the reflection (padded row -1 is row 1, row h is row h - 2; columns likewise)
template <int LV>
__device__ __forceinline__ float gms_level_grad(const GmsLossGeo& g, int b, int y, int x) {
  const int h = g.H >> LV, w = g.W >> LV;
  const float* __restrict__ P = g.pa[LV] + (size_t)b * h * w;
  const float* __restrict__ Q = g.qa[LV] + (size_t)b * h * w;
  auto at = [&](const float* __restrict__ A, int yy, int xx) { return (yy >= 0 && yy < h && xx >= 0 && xx < w) ? A[(size_t)yy * w + xx] : 0.0f; };
  float acc = 0.0f;
#pragma unroll
  for (int iy = 0; iy < 3; ++iy) {
    if ((iy == 1 && y != 1) || (iy == 2 && y != h - 2)) continue;
    const int Y = iy == 0 ? y : (iy == 1 ? -1 : h);
#pragma unroll
    for (int ix = 0; ix < 3; ++ix) {
      if ((ix == 1 && x != 1) || (ix == 2 && x != w - 2)) continue;
      const int X = ix == 0 ? x : (ix == 1 ? -1 : w);
#pragma unroll
      for (int d = -1; d <= 1; ++d) {
        acc += at(P, Y - d, X - 1) - at(P, Y - d, X + 1);
        acc += at(Q, Y - 1, X - d) - at(Q, Y + 1, X - d);
      }
    }
  }
  return acc;
}

// dsr (+)= weight * gscale * d loss / d sr, one thread per level-0 pixel
template <int L>
__global__ __launch_bounds__(256) void gms_loss_grad_kernel(const float* __restrict__ sr, GmsLossGeo g, float weight,
                                                            const float* __restrict__ gscale, float* __restrict__ dsr, int accumulate) {
  const size_t plane = (size_t)g.H * g.W;
  const size_t t = blockIdx.x * (size_t)256 + threadIdx.x;
  if (t >= (size_t)g.B * plane) return;
  const int b = (int)(t / plane);
  const int p = (int)(t - (size_t)b * plane);
  const int y = p / g.W, x = p - y * g.W;
  float gsum = 0.0f;
  static_for<0, L>([&](auto lv) {
    constexpr int LV = decltype(lv)::value;
    gsum += gms_level_grad<LV>(g, b, y >> LV, x >> LV) * (1.0f / (float)(1 << (2 * LV)));     // the 2x2 averages below level LV
  });
  const float cf = weight * (gscale ? gscale[0] : 1.0f) * g.inv_range * (g.C == 1 ? 1.0f : 1.0f / 3.0f);
  for (int c = 0; c < g.C; ++c) {
    const size_t idx = ((size_t)b * g.C + c) * plane + p;
    const float s = sr[idx] * g.inv_range;
    const float v = (s >= 0.0f && s <= 1.0f) ? gsum * cf : 0.0f;       // torch.clamp passes the bounds
    dsr[idx] = accumulate ? dsr[idx] + v : v;
  }
}

size_t gms_loss_layout(int levels, int B, int C, int H, int W, float rgb_range, void* workspace, GmsLossGeo* g) {
  char* base = reinterpret_cast<char*>(workspace);
  size_t off = kLossNb * sizeof(double);
  if (g) { g->B = B; g->C = C; g->H = H; g->W = W; g->inv_range = 1.0f / rgb_range; }
  for (int l = 0; l < kMaxLevels; ++l) {
    if (g) { g->xa[l] = g->xb[l] = g->pa[l] = g->qa[l] = nullptr; g->wl[l] = 0.0; }
    if (l >= levels) continue;
    const size_t cells = (size_t)B * (H >> l) * (W >> l);
    const size_t slab = srad_align_up(cells * sizeof(float), 256);
    if (g) {
      g->xa[l] = reinterpret_cast<float*>(base + off);
      g->xb[l] = reinterpret_cast<float*>(base + off + slab);
      g->pa[l] = reinterpret_cast<float*>(base + off + 2 * slab);
      g->qa[l] = reinterpret_cast<float*>(base + off + 3 * slab);
      g->wl[l] = 1.0 / ((double)levels * (double)cells);
    }
    off += 4 * slab;
  }
  return off;
}

}  // namespace

int srad_gms_loss_levels(int kind) { return kind == SRAD_LOSS_MSGMS ? 4 : 1; }

int srad_gms_loss_workspace_bytes(const char* what, int kind, int B, int C, int H, int W, size_t* bytes) {
  SRAD_REQUIRE(C == 1 || C == 3, "%s: the GMS losses take 1 or 3 channels (got %d)", what, C);
  if (kind == SRAD_LOSS_MSGMS)
    SRAD_REQUIRE(H % 8 == 0 && W % 8 == 0 && H >= 16 && W >= 16,
                 "%s: the four levels of MSGMS need H and W to be multiples of 8 and at least 16 (got %dx%d)", what, H, W);
  else
    SRAD_REQUIRE(H >= 2 && W >= 2, "%s: GMS needs H and W of at least 2 (got %dx%d)", what, H, W);
  SRAD_REQUIRE(((size_t)B * H * W + 255) / 256 < (1ull << 31), "%s: %d %dx%d images are too many pixels for one launch", what, B, H, W);
  *bytes = gms_loss_layout(srad_gms_loss_levels(kind), B, C, H, W, 1.0f, nullptr, nullptr);
  return SRAD_OK;
}

int srad_gms_loss_forward(int kind, const float* sr, const float* hr, int B, int C, int H, int W, float rgb_range, double* out2,
                          void* workspace, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int levels = srad_gms_loss_levels(kind);
  GmsLossGeo g;
  gms_loss_layout(levels, B, C, H, W, rgb_range, workspace, &g);
  double* partial = reinterpret_cast<double*>(workspace);
  size_t total = 0;
  for (int l = 0; l < levels; ++l) total += (size_t)B * (H >> l) * (W >> l);
  const int nb = (int)std::min<size_t>(kLossNb, (total + 255) / 256);
  const dim3 pgrid((unsigned)(((size_t)B * (H >> (levels - 1)) * (W >> (levels - 1)) + 255) / 256), 2);
  if (levels == 1) {
    hipLaunchKernelGGL(gms_loss_planes_kernel<1>, pgrid, dim3(256), 0, s, sr, hr, g);
    hipLaunchKernelGGL(gms_loss_d_kernel<1>, dim3(nb), dim3(256), 0, s, g, partial);
  } else {
    hipLaunchKernelGGL(gms_loss_planes_kernel<4>, pgrid, dim3(256), 0, s, sr, hr, g);
    hipLaunchKernelGGL(gms_loss_d_kernel<4>, dim3(nb), dim3(256), 0, s, g, partial);
  }
  hipLaunchKernelGGL(gms_loss_finish_kernel, dim3(1), dim3(64), 0, s, partial, nb, out2);
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

int srad_gms_loss_backward(int kind, const float* sr, int B, int C, int H, int W, float rgb_range, const float* gscale_dev,
                           float weight, float* dsr, int accumulate, void* workspace, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int levels = srad_gms_loss_levels(kind);
  GmsLossGeo g;
  gms_loss_layout(levels, B, C, H, W, rgb_range, workspace, &g);
  const dim3 grid((unsigned)(((size_t)B * H * W + 255) / 256));
  if (levels == 1) hipLaunchKernelGGL(gms_loss_grad_kernel<1>, grid, dim3(256), 0, s, sr, g, weight, gscale_dev, dsr, accumulate);
  else hipLaunchKernelGGL(gms_loss_grad_kernel<4>, grid, dim3(256), 0, s, sr, g, weight, gscale_dev, dsr, accumulate);
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

extern "C" {

int srad_gms_map_workspace_bytes(int n_img, int H, int W, int levels, size_t* bytes) {
  SRAD_REQUIRE(bytes, "gms_map_workspace_bytes: null argument");
  SRAD_TRY(gms_map_geometry("gms_map_workspace_bytes", n_img, H, W, levels));
  *bytes = gms_map_layout(n_img, H, W, 1, levels, nullptr, nullptr);
  return SRAD_OK;
}

int srad_gms_maps(const uint8_t* sr, const uint8_t* hr, int n_img, int H, int W, int C, int levels, float* map_out, void* workspace,
                  size_t workspace_bytes, void* stream) {
  SRAD_REQUIRE(sr && hr && map_out && workspace, "gms_maps: null argument");
  SRAD_REQUIRE(C == 1 || C == 3, "gms_maps: channels must be 1 or 3 (got %d)", C);
  SRAD_TRY(gms_map_geometry("gms_maps", n_img, H, W, levels));
  const size_t need = gms_map_layout(n_img, H, W, C, levels, nullptr, nullptr);
  SRAD_REQUIRE(workspace_bytes >= need, "gms_maps: workspace %zu bytes, %zu needed", workspace_bytes, need);
  GmsMapGeo g;
  gms_map_layout(n_img, H, W, C, levels, workspace, &g);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const double npix = (double)n_img * H * W;
  // bytes: the two u8 stacks read, the map written, and the coarser levels' planes written and read back (21/64 of 16 B, twice)
  SradProfScope prof(s, SRAD_K_SCORE, 60.0 * npix, (2.0 * C + 4.0 + (levels > 1 ? 10.5 : 0.0)) * npix);
  if (C == 1) launch_gms_maps<1>(sr, hr, g, levels, map_out, s);
  else launch_gms_maps<3>(sr, hr, g, levels, map_out, s);
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

}  // extern "C"
