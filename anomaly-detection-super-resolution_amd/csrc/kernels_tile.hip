// kernels_tile.hip - tiled inference (DESIGN.md "Tiled inference"): the cover of an LR image with overlapping tiles
// (srad_tile_plan, host only), the copy of the tiles out of the image (srad_tile_gather) and the blend of the network's tile
// outputs into the image's output (srad_tile_blend).  include/srad.h has the definitions; this file follows them literally.
//
// Both kernels are byte movers: one thread per output element - or per four of them along a row where every row start, tile
// origin and extent involved is a multiple of four elements and the pointers sit on 16 bytes (always so at scale 4 with aligned
// tensors), else the scalar instance - so a wave writes 256 or 1024 consecutive bytes, and reads consecutive bytes of one tile
// or image row.  The blend is in gather form: a thread walks the tiles that cover its pixel in tile order (y outer, x inner), so
// the order of the fp32 sums is fixed, nothing is atomic, and the loop counts depend on the pixel alone.  No array is indexed at
// run time: the four lanes of the vector instance are unrolled into registers.
//
// The file is compiled without FMA contraction: the feather mode's product and sum are two roundings, as the definition says.
// The divisions are plain `/`, which this build rounds correctly.
#include "srad_common.h"

#pragma clang fp contract(off)

namespace {

// origin of tile k of an axis with stride S whose last origin is `last` (= p - t): 0, S, 2S, ... below last, then last
__host__ __device__ __forceinline__ int tile_origin(int k, int S, int last) {
  const long long o = (long long)k * S;
  return o < last ? (int)o : last;
}
// padded coordinate i >= 0 -> source coordinate of an axis of n samples
__device__ __forceinline__ int tile_reflect(int i, int n) {
  if (i < n) return i;
  const int j = i % (2 * n);
  return j < n ? j : 2 * n - 1 - j;
}

struct GatherArgs {
  int C, h, w, ty, tx, S, ly, lx, ny, nx;   // ly, lx: the last origins
};

template <int VEC>
__global__ __launch_bounds__(256) void tile_gather_kernel(const float* __restrict__ x, float* __restrict__ tiles, GatherArgs a,
                                                          size_t total) {
  const int txv = a.tx / VEC;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const int xv = (int)(idx % txv);
    size_t r = idx / txv;
    const int u = (int)(r % a.ty);
    r /= a.ty;
    const int c = (int)(r % a.C);
    const size_t tile = r / a.C;
    const int kx = (int)(tile % a.nx);
    const size_t t2 = tile / a.nx;
    const int ky = (int)(t2 % a.ny);
    const size_t b = t2 / a.ny;
    const int sy = tile_reflect(tile_origin(ky, a.S, a.ly) + u, a.h);
    const int ix = tile_origin(kx, a.S, a.lx) + xv * VEC;
    const float* __restrict__ row = x + ((b * a.C + c) * a.h + sy) * (size_t)a.w;
    if constexpr (VEC == 4) {
      f32x4 v;
      if (ix + 3 < a.w) {                                    // the whole quad lies in the image: ix and w are multiples of 4
        v = *reinterpret_cast<const f32x4*>(row + ix);
      } else {
        v[0] = row[tile_reflect(ix, a.w)];
        v[1] = row[tile_reflect(ix + 1, a.w)];
        v[2] = row[tile_reflect(ix + 2, a.w)];
        v[3] = row[tile_reflect(ix + 3, a.w)];
      }
      *reinterpret_cast<f32x4*>(tiles + idx * 4) = v;
    } else {
      tiles[idx] = row[tile_reflect(ix, a.w)];
    }
  }
}

struct BlendArgs {
  int C, Hs, Ws, s, S, ty, tx, ly, lx, ny, nx, Ey, Ex, cap;   // Hs, Ws: the output's extents; Ey, Ex: a tile's; cap = O * s + 1
};

// tiles k_lo .. k_hi of an axis cover LR coordinate i (0 <= i < p); t = tile extent, last = p - t, count = tiles on the axis
__device__ __forceinline__ void tile_cover(int i, int S, int t, int last, int count, int& k_lo, int& k_hi) {
  k_hi = i >= last ? count - 1 : i / S;
  k_lo = i < t ? 0 : (i - t) / S + 1;
  if (k_lo > count - 1) k_lo = count - 1;
}

template <int VEC, int MODE>
__global__ __launch_bounds__(256) void tile_blend_kernel(const float* __restrict__ y, float* __restrict__ out, BlendArgs a,
                                                         size_t total) {
  const int wv = a.Ws / VEC;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const int X = (int)(idx % wv) * VEC;
    size_t r = idx / wv;
    const int Y = (int)(r % a.Hs);
    r /= a.Hs;
    const int c = (int)(r % a.C);
    const size_t b = r / a.C;
    int ky0, ky1, kx0, kx1;
    tile_cover(Y / a.s, a.S, a.ty, a.ly, a.ny, ky0, ky1);
    tile_cover(X / a.s, a.S, a.tx, a.lx, a.nx, kx0, kx1);     // the quad's pixels share their cover: tile edges are multiples of 4
    float acc[VEC], first[VEC];
    unsigned long long wsum[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.f, first[e] = 0.f, wsum[e] = 0;
    int n = 0;
    for (int ky = ky0; ky <= ky1; ++ky) {
      const int U = Y - tile_origin(ky, a.S, a.ly) * a.s;
      const unsigned ay = (unsigned)min(min(U + 1, a.Ey - U), a.cap);
      const size_t trow = (b * a.ny + ky) * a.nx;
      for (int kx = kx0; kx <= kx1; ++kx) {
        const int V = X - tile_origin(kx, a.S, a.lx) * a.s;
        const float* __restrict__ p = y + (((trow + kx) * a.C + c) * a.Ey + U) * (size_t)a.Ex + V;
        float v[VEC];
        if constexpr (VEC == 4) {
          const f32x4 q = *reinterpret_cast<const f32x4*>(p);
          v[0] = q[0], v[1] = q[1], v[2] = q[2], v[3] = q[3];
        } else {
          v[0] = *p;
        }
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          if constexpr (MODE == SRAD_TILE_BLEND_FEATHER) {
            const unsigned wgt = ay * (unsigned)min(min(V + e + 1, a.Ex - V - e), a.cap);     // <= 4095^2
            const float term = (float)wgt * v[e];
            acc[e] = n ? acc[e] + term : term;
            wsum[e] += wgt;
          } else {
            acc[e] = n ? acc[e] + v[e] : v[e];
          }
          if (n == 0) first[e] = v[e];
        }
        ++n;
      }
    }
    float res[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      if (n == 1) res[e] = first[e];                          // one covering tile: its value, in both modes
      else if constexpr (MODE == SRAD_TILE_BLEND_FEATHER) res[e] = acc[e] / (float)wsum[e];
      else res[e] = acc[e] / (float)n;
    }
    if constexpr (VEC == 4) {
      f32x4 q;
      q[0] = res[0], q[1] = res[1], q[2] = res[2], q[3] = res[3];
      *reinterpret_cast<f32x4*>(out + idx * 4) = q;
    } else {
      out[idx] = res[0];
    }
  }
}

int axis_plan(int n, int tile, int stride, int granule, int32_t* p, int32_t* t, int32_t* count) {
  const long long pad = ((long long)n + granule - 1) / granule * granule;
  if (pad > 0x7fffffffLL) return 1;
  *p = (int32_t)pad;
  *t = tile < *p ? tile : *p;
  const int last = *p - *t;
  *count = (last + stride - 1) / stride + 1;                   // len(range(0, last, stride)) + 1
  return 0;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

unsigned blocks_for(size_t total) {
  const size_t b = (total + 255) / 256, cap = (size_t)srad_cu_count() * 32;
  return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

}  // namespace

extern "C" int srad_tile_plan(int h, int w, int tile, int overlap, int granule, int scale, srad_tile_geom* geom) {
  SRAD_REQUIRE(geom, "tile_plan: null argument");
  SRAD_REQUIRE(h >= 1 && w >= 1, "tile_plan: the image must be at least 1 x 1, got %d x %d", h, w);
  SRAD_REQUIRE(tile >= 1, "tile_plan: tile must be >= 1, got %d", tile);
  SRAD_REQUIRE(overlap >= 0 && overlap < tile, "tile_plan: overlap must be in [0, tile), got overlap %d for tile %d", overlap, tile);
  SRAD_REQUIRE(granule >= 1 && tile % granule == 0, "tile_plan: tile %d is not a multiple of the granule %d", tile, granule);
  SRAD_REQUIRE(scale >= 1, "tile_plan: scale must be >= 1, got %d", scale);
  SRAD_REQUIRE((long long)overlap * scale <= 4094,
               "tile_plan: overlap * scale = %d * %d exceeds 4094 (the blend weights would not be exact fp32 integers)", overlap, scale);
  srad_tile_geom g = {h, w, tile, overlap, granule, scale, 0, 0, 0, 0, tile - overlap, 0, 0};
  SRAD_REQUIRE(!axis_plan(h, tile, g.stride, granule, &g.ph, &g.ty, &g.ny) && !axis_plan(w, tile, g.stride, granule, &g.pw, &g.tx, &g.nx),
               "tile_plan: the padded image %d x %d (granule %d) does not fit 32-bit sizes", h, w, granule);
  SRAD_REQUIRE((long long)g.ph * scale <= 0x7fffffffLL && (long long)g.pw * scale <= 0x7fffffffLL && (long long)g.ny * g.nx <= 0x7fffffffLL,
               "tile_plan: %d x %d at scale %d with %d x %d tiles does not fit 32-bit sizes", h, w, scale, g.ny, g.nx);
  *geom = g;
  return SRAD_OK;
}

extern "C" int srad_tile_origins(const srad_tile_geom* g, int32_t* oy, int32_t* ox) {
  SRAD_REQUIRE(g && oy && ox, "tile_origins: null argument");
  SRAD_REQUIRE(g->stride >= 1 && g->ny >= 1 && g->nx >= 1 && g->ph >= g->ty && g->pw >= g->tx, "tile_origins: not a plan of srad_tile_plan");
  for (int k = 0; k < g->ny; ++k) oy[k] = tile_origin(k, g->stride, g->ph - g->ty);
  for (int k = 0; k < g->nx; ++k) ox[k] = tile_origin(k, g->stride, g->pw - g->tx);
  return SRAD_OK;
}

// sizes of a batch over a plan: tiles = B * ny * nx < 2^31, and both tensors' element counts (64-bit offsets in the kernels)
static int tile_batch_check(const char* what, int B, int C, const srad_tile_geom& g, size_t* n_img, size_t* n_tiles) {
  SRAD_REQUIRE(B > 0 && C > 0, "%s: sizes must be positive, got B=%d C=%d", what, B, C);
  const unsigned long long tiles = (unsigned long long)B * g.ny * g.nx;       // B < 2^31, ny * nx < 2^31
  SRAD_REQUIRE(tiles < (1ull << 31), "%s: %d images of %d x %d tiles are 2^31 tiles or more", what, B, g.ny, g.nx);
  const unsigned long long s = g.scale, per_tile = (unsigned long long)g.ty * s * g.tx * s, per_img = (unsigned long long)g.h * s * g.w * s;
  SRAD_REQUIRE(per_tile < (1ull << 40) && per_img < (1ull << 40) && tiles * C < (1ull << 40) && (unsigned long long)B * C < (1ull << 40) &&
               tiles * C * per_tile < (1ull << 46) && (unsigned long long)B * C * per_img < (1ull << 46),
               "%s: B=%d C=%d with %d x %d tiles of %d x %d at scale %d is too large", what, B, C, g.ny, g.nx, g.ty, g.tx, g.scale);
  *n_img = (size_t)((unsigned long long)B * C * per_img);
  *n_tiles = (size_t)(tiles * C * per_tile);
  return SRAD_OK;
}

extern "C" int srad_tile_gather(const float* x, int B, int C, int h, int w, int tile, int overlap, int granule, float* tiles, void* stream) {
  SRAD_REQUIRE(x && tiles, "tile_gather: null argument");
  srad_tile_geom g;
  SRAD_TRY(srad_tile_plan(h, w, tile, overlap, granule, 1, &g));
  size_t n_img, n_tiles;
  SRAD_TRY(tile_batch_check("tile_gather", B, C, g, &n_img, &n_tiles));
  SRAD_REQUIRE(!srad_ranges_overlap(x, n_img, tiles, n_tiles), "tile_gather: tiles overlaps x");
  const GatherArgs a = {C, h, w, g.ty, g.tx, g.stride, g.ph - g.ty, g.pw - g.tx, g.ny, g.nx};
  const bool vec = g.tx % 4 == 0 && w % 4 == 0 && g.stride % 4 == 0 && a.lx % 4 == 0 && aligned16(x) && aligned16(tiles);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  SradProfScope prof(s, SRAD_K_MISC, 0.0, 8.0 * n_tiles);
  const size_t total = vec ? n_tiles / 4 : n_tiles;
  if (vec) hipLaunchKernelGGL(tile_gather_kernel<4>, dim3(blocks_for(total)), dim3(256), 0, s, x, tiles, a, total);
  else hipLaunchKernelGGL(tile_gather_kernel<1>, dim3(blocks_for(total)), dim3(256), 0, s, x, tiles, a, total);
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

extern "C" int srad_tile_blend(const float* y, int B, int C, int h, int w, int tile, int overlap, int granule, int scale, int mode,
                               float* out, void* stream) {
  SRAD_REQUIRE(y && out, "tile_blend: null argument");
  SRAD_REQUIRE(mode == SRAD_TILE_BLEND_MEAN || mode == SRAD_TILE_BLEND_FEATHER, "tile_blend: unknown mode %d (0 mean, 1 feather)", mode);
  srad_tile_geom g;
  SRAD_TRY(srad_tile_plan(h, w, tile, overlap, granule, scale, &g));
  size_t n_img, n_tiles;
  SRAD_TRY(tile_batch_check("tile_blend", B, C, g, &n_img, &n_tiles));
  SRAD_REQUIRE(!srad_ranges_overlap(out, n_img, y, n_tiles), "tile_blend: out overlaps y");
  const BlendArgs a = {C, h * scale, w * scale, scale, g.stride, g.ty, g.tx, g.ph - g.ty, g.pw - g.tx, g.ny, g.nx, g.ty * scale, g.tx * scale,
                       overlap * scale + 1};
  const bool vec = a.Ws % 4 == 0 && a.Ex % 4 == 0 && ((long long)g.stride * scale) % 4 == 0 && ((long long)a.lx * scale) % 4 == 0 &&
                   aligned16(y) && aligned16(out);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const double cover = (double)n_tiles / ((double)B * C * g.ph * scale * g.pw * scale);     // tiles read per output pixel, on average
  SradProfScope prof(s, SRAD_K_MISC, (mode ? 2.0 : 1.0) * cover * n_img, 4.0 * n_img * (1.0 + cover));
  const size_t total = vec ? n_img / 4 : n_img;
  const dim3 grid(blocks_for(total)), block(256);
  if (vec && mode) hipLaunchKernelGGL((tile_blend_kernel<4, SRAD_TILE_BLEND_FEATHER>), grid, block, 0, s, y, out, a, total);
  else if (vec) hipLaunchKernelGGL((tile_blend_kernel<4, SRAD_TILE_BLEND_MEAN>), grid, block, 0, s, y, out, a, total);
  else if (mode) hipLaunchKernelGGL((tile_blend_kernel<1, SRAD_TILE_BLEND_FEATHER>), grid, block, 0, s, y, out, a, total);
  else hipLaunchKernelGGL((tile_blend_kernel<1, SRAD_TILE_BLEND_MEAN>), grid, block, 0, s, y, out, a, total);
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}
