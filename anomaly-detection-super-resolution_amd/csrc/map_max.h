// map_max.h - the per-image maximum of float32 maps, shared by the kernels that write maps (kernels_map_smooth.hip,
// kernels_map_baseline.hip): a kernel reduces order_key (pixel_sort.h; NaN is the largest key, -0.0 == +0.0) over each wave
// with wave_max_u32 and combines the waves with one u32 atomicMax per wave or workgroup into a key per image; a last tiny
// kernel turns the keys back into floats.  A max does not depend on the order, so the result is deterministic.  The keys
// live in the caller's workspace: map_max_workspace_bytes, cleared by map_max_begin, converted by map_max_finish.
#pragma once
#include "engine.h"
#include "pixel_sort.h"
#include <algorithm>

namespace {

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = std::max(v, (uint32_t)__shfl_xor((int)v, o));
  return v;
}

// An image's key may be spread over `slots` u32, `stride` u32 apart (image i, slot j at keys[(i * slots + j) * stride]), so that
// many waves do not queue on one address; a kernel with one atomic per workgroup tile keeps the default, one key per image.
// order_key back to the float: kNanKey -> NaN, keys with the top bit set were non-negative floats, the others negative ones
__global__ __launch_bounds__(256) void map_max_finish_kernel(const uint32_t* __restrict__ keys, float* __restrict__ img_max, int n,
                                                             int slots, int stride) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint32_t k = 0u;
  for (int j = 0; j < slots; ++j) k = std::max(k, keys[((size_t)i * slots + j) * stride]);
  img_max[i] = k == kNanKey ? __uint_as_float(0x7FC00000u) : __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

inline size_t map_max_workspace_bytes(int n_img, int slots = 1, int stride = 1) {
  return srad_align_up((size_t)n_img * slots * stride * sizeof(uint32_t), 256);
}

// keys = 0, below every key a float maps to
inline hipError_t map_max_begin(uint32_t* keys, int n_img, hipStream_t s, int slots = 1, int stride = 1) {
  return hipMemsetAsync(keys, 0, (size_t)n_img * slots * stride * sizeof(uint32_t), s);
}

inline void map_max_finish(const uint32_t* keys, float* img_max_out, int n_img, hipStream_t s, int slots = 1, int stride = 1) {
  hipLaunchKernelGGL(map_max_finish_kernel, dim3((unsigned)((n_img + 255) / 256)), dim3(256), 0, s, keys, img_max_out, n_img, slots, stride);
}

}  // namespace
