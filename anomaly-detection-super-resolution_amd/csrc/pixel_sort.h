// pixel_sort.h - the device sort of the sort-based pixel metrics (kernels_pixel_auc.hip, kernels_pixel_pro.hip,
// kernels_pixel_pr.hip, through tie_scan.h, which holds their workspace layout, the three-pass driver and the scan of the sorted
// keys).
//
// LSD radix sort of u64 keys on 11-bit digits: a pass is a per-tile LDS histogram (tile = 8192 keys), an exclusive scan of the
// [digit][tile] count matrix, and a stable scatter.  A caller picks the digits with the shifts it passes: the AUC sorts its 33-bit
// keys at shifts 0 / 11 / 22 (so does precision-recall), AU-PRO sorts the high 32 bits of its keys at 32 / 43 / 54 and lets the
// low word ride along.  Also here, and used by kernels_operating_point.hip and kernels_map_smooth.hip as well: the
// order-preserving u32 of a float (and its descending twin), and the 256-thread block scan every scan is built from.
#pragma once
#include "engine.h"
#include <algorithm>

namespace {

constexpr int kDigitBits = 11, kDigits = 1 << kDigitBits, kPasses = 3;
constexpr int kSortWaves = 4, kSortRounds = 32, kSortTile = 64 * kSortWaves * kSortRounds;   // 8192 keys per sort tile
constexpr int kScanItems = 16, kScanTile = 256 * kScanItems;                                 // 4096 values per scan tile
constexpr uint32_t kNanKey = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t order_key(float f) {
  uint32_t b = __float_as_uint(f);
  if ((b & 0x7FFFFFFFu) > 0x7F800000u) return kNanKey;
  if (b == 0x80000000u) b = 0u;                                  // -0.0 == +0.0
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
// order_key upside down: ascending keys walk the floats from the highest down; a NaN still sorts last.
__device__ __forceinline__ uint32_t desc_key(float f) {
  const uint32_t k = order_key(f);
  return k == kNanKey ? kNanKey : ~k;
}

// order_key back to its float (of the two zeros, +0.0)
__device__ __forceinline__ float key_to_float(uint32_t key) {
  if (key == kNanKey) return __uint_as_float(0x7FC00000u);
  return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

// Block-wide scan over 256 threads (Hillis-Steele in LDS): returns the exclusive prefix, `total` = the whole block's.
template <typename T, typename Op>
__device__ __forceinline__ T block_scan_excl(T v, T identity, Op op, T* sh, T& total) {
  const int tid = threadIdx.x;
  T x = v;
  sh[tid] = x;
  __syncthreads();
#pragma unroll
  for (int o = 1; o < 256; o <<= 1) {
    const T y = tid >= o ? sh[tid - o] : identity;
    __syncthreads();
    x = op(x, y);
    sh[tid] = x;
    __syncthreads();
  }
  total = sh[255];
  const T ex = tid > 0 ? sh[tid - 1] : identity;
  __syncthreads();                                               // sh may be reused right away
  return ex;
}
struct AddOp { template <typename T> __device__ T operator()(T a, T b) const { return a + b; } };
struct MaxOp { template <typename T> __device__ T operator()(T a, T b) const { return a > b ? a : b; } };

// counts[d * n_tiles + tile] = keys of the tile whose digit (at `shift`) is d
__global__ __launch_bounds__(256) void radix_hist_kernel(const uint64_t* __restrict__ keys, uint32_t* __restrict__ counts, int64_t n,
                                                         int shift, int n_tiles) {
  __shared__ uint32_t h[kDigits];
  for (int d = threadIdx.x; d < kDigits; d += 256) h[d] = 0u;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * kSortTile, end = std::min<int64_t>(n, base + kSortTile);
  for (int64_t i = base + threadIdx.x; i < end; i += 256) atomicAdd(&h[(uint32_t)(keys[i] >> shift) & (kDigits - 1)], 1u);
  __syncthreads();
  for (int d = threadIdx.x; d < kDigits; d += 256) counts[(size_t)d * n_tiles + blockIdx.x] = h[d];
}

// Exclusive scan of a u32 array in place: per-tile sums, one block scanning the tile sums, per-tile scans plus their offset.
__global__ __launch_bounds__(256) void scan_reduce_kernel(const uint32_t* __restrict__ v, uint32_t* __restrict__ tsum, int64_t m) {
  __shared__ uint32_t sh[256];
  const int64_t b = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
  uint32_t s = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k)
    if (b + k < m) s += v[b + k];
  uint32_t total;
  block_scan_excl<uint32_t>(s, 0u, AddOp{}, sh, total);
  if (threadIdx.x == 0) tsum[blockIdx.x] = total;
}
__global__ __launch_bounds__(256) void scan_top_kernel(uint32_t* __restrict__ tsum, int nt) {
  __shared__ uint32_t sh[256];
  uint32_t carry = 0;
  for (int c0 = 0; c0 < nt; c0 += 256) {
    const int t = c0 + threadIdx.x;
    const uint32_t v = t < nt ? tsum[t] : 0u;
    uint32_t total;
    const uint32_t ex = block_scan_excl<uint32_t>(v, 0u, AddOp{}, sh, total);
    if (t < nt) tsum[t] = carry + ex;
    carry += total;
  }
}
__global__ __launch_bounds__(256) void scan_apply_kernel(uint32_t* __restrict__ v, const uint32_t* __restrict__ tsum, int64_t m) {
  __shared__ uint32_t sh[256];
  const int64_t b = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
  uint32_t x[kScanItems], s = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    x[k] = b + k < m ? v[b + k] : 0u;
    s += x[k];
  }
  uint32_t total;
  uint32_t run = tsum[blockIdx.x] + block_scan_excl<uint32_t>(s, 0u, AddOp{}, sh, total);
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    if (b + k < m) v[b + k] = run;
    run += x[k];
  }
}

// Stable scatter of one tile: key i of the tile goes to offs[d][tile] + (keys of digit d before it in the tile).  Round r,
// wave w, lane l holds tile key (r * 4 + w) * 64 + l, so (round, wave, lane) order is input order.
__global__ __launch_bounds__(256) void radix_scatter_kernel(const uint64_t* __restrict__ src, uint64_t* __restrict__ dst,
                                                            const uint32_t* __restrict__ offs, int64_t n, int shift, int n_tiles) {
  __shared__ uint32_t run[kDigits];                              // next free position of each digit
  __shared__ uint32_t wcnt[kSortWaves][kDigits];                 // keys of each digit in each wave of the current round
  const int tile = blockIdx.x, lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int d = threadIdx.x; d < kDigits; d += 256) {
    run[d] = offs[(size_t)d * n_tiles + tile];
#pragma unroll
    for (int w = 0; w < kSortWaves; ++w) wcnt[w][d] = 0u;
  }
  __syncthreads();
  const uint64_t lanes_below = (1ull << lane) - 1ull;
  const int64_t base = (int64_t)tile * kSortTile;
  for (int r = 0; r < kSortRounds; ++r) {
    if (base + (int64_t)r * 64 * kSortWaves >= n) break;         // block-uniform
    const int64_t i = base + (int64_t)(r * kSortWaves + wave) * 64 + lane;
    const bool valid = i < n;
    const uint64_t k = valid ? src[i] : 0ull;
    const uint32_t d = (uint32_t)(k >> shift) & (kDigits - 1);
    uint64_t same = __builtin_amdgcn_ballot_w64(valid);          // lanes of the wave with the same digit
#pragma unroll
    for (int bit = 0; bit < kDigitBits; ++bit) {
      const bool set = (d >> bit) & 1u;
      const uint64_t bb = __builtin_amdgcn_ballot_w64(set);
      same &= set ? bb : ~bb;
    }
    const uint32_t rank = (uint32_t)__popcll(same & lanes_below), cnt = (uint32_t)__popcll(same);
    const bool leader = valid && rank == 0;
    if (leader) wcnt[wave][d] = cnt;
    __syncthreads();
    if (valid) {
      uint32_t pos = run[d] + rank;
      for (int w = 0; w < wave; ++w) pos += wcnt[w][d];
      if (pos < (uint64_t)n) dst[pos] = k;
    }
    __syncthreads();
    if (leader) {
      atomicAdd(&run[d], cnt);
      wcnt[wave][d] = 0u;
    }
    __syncthreads();
  }
}

// One stable radix pass of `n` keys src -> dst on the digit at `shift`: histogram, count-matrix scan, scatter (5 launches).
// offs: the [digit][tile] matrix (kDigits x n_sort_tiles u32), tsum: one u32 per count tile.
inline void radix_sort_pass(const uint64_t* src, uint64_t* dst, uint32_t* offs, uint32_t* tsum, int64_t n, int shift,
                            int n_sort_tiles, hipStream_t s) {
  const int64_t m = (int64_t)kDigits * n_sort_tiles;
  const int n_count_tiles = (int)((m + kScanTile - 1) / kScanTile);
  hipLaunchKernelGGL(radix_hist_kernel, dim3(n_sort_tiles), dim3(256), 0, s, src, offs, n, shift, n_sort_tiles);
  hipLaunchKernelGGL(scan_reduce_kernel, dim3(n_count_tiles), dim3(256), 0, s, offs, tsum, m);
  hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(256), 0, s, tsum, n_count_tiles);
  hipLaunchKernelGGL(scan_apply_kernel, dim3(n_count_tiles), dim3(256), 0, s, offs, tsum, m);
  hipLaunchKernelGGL(radix_scatter_kernel, dim3(n_sort_tiles), dim3(256), 0, s, src, dst, offs, n, shift, n_sort_tiles);
}

}  // namespace
