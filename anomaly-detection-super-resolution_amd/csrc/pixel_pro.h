// pixel_pro.h - the fixed-point per-region overlap sum shared by AU-PRO (kernels_pixel_pro.hip) and the operating point
// (kernels_operating_point.hip): a pixel of a region of z pixels adds floor(2^64 / z) to a 128-bit numerator.
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

// n = n_img x H x W of an [n_img, H, W] stack, refused outside [1, 2^31) (a pixel index is a u32 with 0xFFFFFFFF to spare)
inline int check_shape(int n_img, int H, int W, const char* who, int64_t& n) {
  SRAD_REQUIRE(n_img >= 1 && H >= 1 && W >= 1 && (int64_t)H * W <= INT32_MAX && (int64_t)H * W * n_img <= INT32_MAX,
               "%s: n_img x H x W = %d x %d x %d, must be in [1, 2^31)", who, n_img, H, W);
  n = (int64_t)n_img * H * W;
  return SRAD_OK;
}

}  // namespace
