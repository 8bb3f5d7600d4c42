// pixel_pro.h - what the region code shares.  The fixed-point per-region overlap sum of AU-PRO (kernels_pixel_pro.hip) and the
// operating point (kernels_operating_point.hip): a pixel of a region of z pixels adds floor(2^64 / z) to a 128-bit numerator.
// The labelling's tile geometry and its entry for other files (kernels_region_table.hip): srad_label_roots.
#pragma once
#include "engine.h"
#include <stdint.h>

namespace {

// Prefix over the walk: the pro numerator as a 128-bit fixed-point number in units of 2^-64, kept as two u64 words with an
// explicit carry (hi:lo), and the ok-pixel count.  (An unsigned __int128 here lost the high-word update of a conditional copy
// in the unrolled scan loop on gfx950; two plain words do not depend on i128 lowering.)
struct alignas(16) Pref {
  uint64_t lo, hi, ok, pad;      // 32 bytes: LDS copies move as two 16-byte words
};
struct PrefAdd {
  __device__ Pref operator()(const Pref& a, const Pref& b) const {
    const uint64_t lo = a.lo + b.lo;
    return Pref{lo, a.hi + b.hi + (lo < a.lo ? 1ull : 0ull), a.ok + b.ok, 0};
  }
};

// p += floor(2^64 / z) for z >= 1: a 64-bit division, plus one when z divides 2^64 (a power of two); z == 1 adds 2^64 itself
__device__ __forceinline__ void pro_add(Pref& p, uint64_t key) {
  const uint32_t z = (uint32_t)key;
  if (z == 0u) {
    ++p.ok;
  } else if (z == 1u) {
    ++p.hi;
  } else {
    const uint64_t q = ~0ull / z + ((z & (z - 1u)) == 0u ? 1ull : 0ull);
    p.lo += q;
    p.hi += p.lo < q ? 1ull : 0ull;
  }
}

// The labelling's geometry: one 32 x 32 tile per block.
constexpr int kLabT = 32, kLabPx = kLabT * kLabT;
constexpr uint32_t kNoParent = 0xFFFFFFFFu;                                  // ok pixel; no index reaches it (n < 2^31)

struct LabGeom {
  int H, W, tiles_x, tiles_y;
};
inline LabGeom lab_geom(int H, int W) { return LabGeom{H, W, (W + kLabT - 1) / kLabT, (H + kLabT - 1) / kLabT}; }

// block -> (first pixel of its image, tile origin)
__device__ __forceinline__ void lab_tile(const LabGeom& g, int64_t& base, int& y0, int& x0) {
  int b = blockIdx.x;
  const int tx = b % g.tiles_x;
  b /= g.tiles_x;
  const int ty = b % g.tiles_y;
  base = (int64_t)(b / g.tiles_y) * g.H * g.W;
  y0 = ty * kLabT;
  x0 = tx * kLabT;
}

// n = n_img x H x W of an [n_img, H, W] stack, refused outside [1, 2^31) (a pixel index is a u32 with 0xFFFFFFFF to spare)
inline int check_shape(int n_img, int H, int W, const char* who, int64_t& n) {
  SRAD_REQUIRE(n_img >= 1 && H >= 1 && W >= 1 && (int64_t)H * W <= INT32_MAX && (int64_t)H * W * n_img <= INT32_MAX,
               "%s: n_img x H x W = %d x %d x %d, must be in [1, 2^31)", who, n_img, H, W);
  n = (int64_t)n_img * H * W;
  return SRAD_OK;
}

}  // namespace

// The labelling of kernels_pixel_pro.hip, stages 1a - 1c, on stream s: parent[i] = the root (its component's smallest linear
// index over the whole stack) of every pixel with masks[i] != 0, kNoParent elsewhere.  parent, size: n u32 each; size is
// scratch afterwards except at a root, where it holds the component's pixel count.  tile_root (n u32, or NULL): a copy of parent
// as stage 1a left it - each pixel's root within its own 32 x 32 tile (lab_tile), a pixel of that tile.  The shape is the
// caller's to check (check_shape).
int srad_label_roots(const uint8_t* masks, int n_img, int H, int W, uint32_t* parent, uint32_t* size, uint32_t* tile_root,
                     hipStream_t s);
