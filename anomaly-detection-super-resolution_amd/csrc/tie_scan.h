// tie_scan.h - what the sort-based pixel metrics (kernels_pixel_auc.hip, kernels_pixel_pro.hip, kernels_pixel_pr.hip) share
// beyond the sort itself: the workspace of a metric over sorted keys, the three-pass sort driver, and the tie-group scan of the
// sorted keys.
//
// The scan.  Walking the sorted keys, a metric keeps a prefix P::Prefix whose every component never decreases (P::add).  Keys
// with equal P::group(key) form a tie group; group kNanKey (NaN scores, sorted last) is left out and counted.  A key is its
// group's head if its predecessor's group differs, its end if its successor's does.  At each group end the metric is handed
//     at_end(prefix just before the head of this group, prefix through this end, number of group ends before this one, this key)
// and the values it returns (P::Acc) are summed: per thread in key order, then by the block's scan tree, then over tiles by
// the metric's own finish kernel.  "The prefix just before the head of my group" is the prefix before the last head at or
// before me; because the prefix never decreases, that is a running maximum (P::Max, "the later position") of the prefix before
// each head, with P::Prefix{} (nothing before the first key) below all of them.  It is carried on three levels: across the
// 256 threads of a scan tile (thread t: keys t * 16 .. t * 16 + 15), across scan tiles, and across the 256-tile chunks of the
// one-block tile scan.  A thread or a tile in which no group starts (has_head == 0) hands on what it received.
//
// A policy P provides: Prefix, Add, Max (functors over Prefix; Prefix{} is the identity of both), Acc (summed with +, Acc{} is
// zero), static uint32_t group(uint64_t key), static void add(Prefix&, uint64_t key), Args (what the host passes to the visiting
// pass), a device constructor P(const Args&), and Acc at_end(const Prefix& before_head, const Prefix& through_end, int64_t idx,
// uint64_t key of the group end).  Acc may be a struct with its own + and +=.
//
// Launches: tie_tile_counts_kernel<P> (per tile), tie_tiles_scan_kernel<P> (one block), tie_visit_kernel<P> (per tile), then
// the metric's finish kernel over the TieTile<P> records.
#pragma once
#include "pixel_sort.h"

namespace {

// ---------------------------------------------------------------- workspace and sort of a metric over n sorted u64 keys
struct SortedKeysLayout {
  int n_sort_tiles, n_scan_tiles;
  int64_t m;                                                     // entries of the [digit][tile] count matrix
  size_t keys_a, keys_b, offs, tsum, tiles, total;
};
inline SortedKeysLayout sorted_keys_layout(int64_t n, size_t tile_bytes) {
  SortedKeysLayout L{};
  L.n_sort_tiles = (int)((n + kSortTile - 1) / kSortTile);
  L.n_scan_tiles = (int)((n + kScanTile - 1) / kScanTile);
  L.m = (int64_t)kDigits * L.n_sort_tiles;
  const int64_t n_count_tiles = (L.m + kScanTile - 1) / kScanTile;
  size_t o = 0;
  L.keys_a = o; o += srad_align_up((size_t)n * 8, 256);
  L.keys_b = o; o += srad_align_up((size_t)n * 8, 256);
  L.offs = o;   o += srad_align_up((size_t)L.m * 4, 256);
  L.tsum = o;   o += srad_align_up((size_t)n_count_tiles * 4, 256);
  L.tiles = o;  o += srad_align_up((size_t)L.n_scan_tiles * tile_bytes, 256);
  L.total = o;
  return L;
}

// Sorts the keys at ws + L.keys_a on the kPasses digits from `first_shift` up, ping-ponging with keys_b; returns the buffer
// that holds the sorted keys.
inline uint64_t* radix_sort_keys(char* ws, const SortedKeysLayout& L, int64_t n, int first_shift, hipStream_t s) {
  uint64_t* src = reinterpret_cast<uint64_t*>(ws + L.keys_a);
  uint64_t* dst = reinterpret_cast<uint64_t*>(ws + L.keys_b);
  for (int p = 0; p < kPasses; ++p) {
    // key bytes: read twice (histogram, scatter), written once; the count matrix: written, scanned (read + written), read
    SradProfScope prof(s, SRAD_K_SCORE, 0.0, 24.0 * n + 16.0 * L.m);
    radix_sort_pass(src, dst, reinterpret_cast<uint32_t*>(ws + L.offs), reinterpret_cast<uint32_t*>(ws + L.tsum), n,
                    first_shift + p * kDigitBits, L.n_sort_tiles, s);
    std::swap(src, dst);
  }
  return src;
}

// ---------------------------------------------------------------- the tie-group scan, in scan tiles of 4096 keys
template <typename P>
struct TieTile {
  typename P::Prefix sum;        // over the tile's non-NaN keys
  typename P::Prefix head;       // prefix (within the tile) just before the tile's last group head; meaningful when has_head
  typename P::Prefix off;        // prefix before the tile
  typename P::Prefix lt_in;      // prefix just before the last group head before the tile
  uint32_t nan, ends, has_head, end_off;   // end_off: group ends before the tile
  typename P::Acc acc;
};

template <typename P>
__device__ __forceinline__ bool tie_is_head(const uint64_t* keys, int64_t i, uint32_t g) {
  return i == 0 || P::group(keys[i - 1]) != g;
}
template <typename P>
__device__ __forceinline__ bool tie_is_end(const uint64_t* keys, int64_t i, int64_t n, uint32_t g) {
  return i == n - 1 || P::group(keys[i + 1]) != g;
}

// A thread's 16 keys: their sum, the prefix (within the thread) just before its last head, its NaN and group-end counts.
template <typename P>
struct TieRun {
  typename P::Prefix own, head;
  uint32_t nan, ends, has_head;
};
template <typename P>
__device__ __forceinline__ TieRun<P> tie_thread_run(const uint64_t* keys, int64_t b, int64_t n) {
  TieRun<P> t{};
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    const int64_t i = b + k;
    if (i >= n) break;
    const uint64_t key = keys[i];
    const uint32_t g = P::group(key);
    if (g == kNanKey) {
      ++t.nan;
      continue;
    }
    if (tie_is_head<P>(keys, i, g)) {
      t.head = t.own;
      t.has_head = 1u;
    }
    P::add(t.own, key);
    if (tie_is_end<P>(keys, i, n, g)) ++t.ends;
  }
  return t;
}

template <typename P>
__global__ __launch_bounds__(256) void tie_tile_counts_kernel(const uint64_t* __restrict__ keys, TieTile<P>* __restrict__ tiles,
                                                              int64_t n) {
  using Prefix = typename P::Prefix;
  __shared__ Prefix shp[256];
  __shared__ uint32_t sh[256];
  const TieRun<P> t = tie_thread_run<P>(keys, (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems, n);
  TieTile<P>& o = tiles[blockIdx.x];
  Prefix tsum;
  const Prefix ex = block_scan_excl<Prefix>(t.own, Prefix{}, typename P::Add{}, shp, tsum);
  if (threadIdx.x == 0) o.sum = tsum;
  // the last head's prefix is the block-wide max, i.e. the inclusive max-scan at thread 255 (kept out of a Prefix-typed total,
  // which the compiler sends to scratch when Prefix is AU-PRO's 32-byte Pref)
  const Prefix hv = t.has_head ? typename P::Add{}(ex, t.head) : Prefix{};
  Prefix unused;
  const Prefix hex = block_scan_excl<Prefix>(hv, Prefix{}, typename P::Max{}, shp, unused);
  if (threadIdx.x == 255) o.head = typename P::Max{}(hex, hv);
  uint32_t tnan, tends, thas;
  block_scan_excl<uint32_t>(t.nan, 0u, AddOp{}, sh, tnan);
  block_scan_excl<uint32_t>(t.ends, 0u, AddOp{}, sh, tends);
  block_scan_excl<uint32_t>(t.has_head, 0u, MaxOp{}, sh, thas);
  if (threadIdx.x == 0) {
    o.nan = tnan;
    o.ends = tends;
    o.has_head = thas;
  }
}

// one block: the prefix before each tile, the prefix before the last head before each tile, the group ends before each tile
template <typename P>
__global__ __launch_bounds__(256) void tie_tiles_scan_kernel(TieTile<P>* __restrict__ tiles, int nt) {
  using Prefix = typename P::Prefix;
  __shared__ Prefix shp[256];
  __shared__ uint32_t sh[256];
  Prefix carry{}, lt_carry{};
  uint32_t end_carry = 0;
  for (int c0 = 0; c0 < nt; c0 += 256) {
    const int t = c0 + threadIdx.x;
    TieTile<P> x{};
    if (t < nt) x = tiles[t];
    Prefix stot, htot;
    const Prefix off = typename P::Add{}(carry, block_scan_excl<Prefix>(x.sum, Prefix{}, typename P::Add{}, shp, stot));
    const Prefix hv = x.has_head ? typename P::Add{}(off, x.head) : Prefix{};
    const Prefix lt = typename P::Max{}(lt_carry, block_scan_excl<Prefix>(hv, Prefix{}, typename P::Max{}, shp, htot));
    uint32_t etot;
    const uint32_t eoff = end_carry + block_scan_excl<uint32_t>(x.ends, 0u, AddOp{}, sh, etot);
    if (t < nt) {
      tiles[t].off = off;
      tiles[t].lt_in = lt;
      tiles[t].end_off = eoff;
    }
    carry = typename P::Add{}(carry, stot);
    lt_carry = typename P::Max{}(lt_carry, htot);
    end_carry += etot;
  }
}

// Each group end in the tile is handed to the metric; the tile's sum of what it returns goes to tiles[].acc.
template <typename P>
__global__ __launch_bounds__(256) void tie_visit_kernel(const uint64_t* __restrict__ keys, TieTile<P>* __restrict__ tiles, int64_t n,
                                                        typename P::Args args) {
  using Prefix = typename P::Prefix;
  using Acc = typename P::Acc;
  __shared__ Prefix shp[256];
  __shared__ uint32_t sh[256];
  __shared__ Acc sha[256];
  const P p(args);
  const int64_t b = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
  const Prefix off = tiles[blockIdx.x].off, lt_in = tiles[blockIdx.x].lt_in;
  const uint32_t end_off = tiles[blockIdx.x].end_off;
  const TieRun<P> t = tie_thread_run<P>(keys, b, n);
  Prefix tot;
  Prefix cur = typename P::Add{}(off, block_scan_excl<Prefix>(t.own, Prefix{}, typename P::Add{}, shp, tot));   // before this thread's keys
  Prefix lt = typename P::Max{}(
      lt_in, block_scan_excl<Prefix>(t.has_head ? typename P::Add{}(cur, t.head) : Prefix{}, Prefix{}, typename P::Max{}, shp, tot));
  uint32_t etot;
  int64_t idx = (int64_t)end_off + block_scan_excl<uint32_t>(t.ends, 0u, AddOp{}, sh, etot);   // group ends before its next end
  Acc acc{};
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    const int64_t i = b + k;
    if (i >= n) break;
    const uint64_t key = keys[i];
    const uint32_t g = P::group(key);
    if (g == kNanKey) continue;
    if (tie_is_head<P>(keys, i, g)) lt = cur;
    P::add(cur, key);
    if (tie_is_end<P>(keys, i, n, g)) {
      acc += p.at_end(lt, cur, idx, key);
      ++idx;
    }
  }
  Acc atot;
  block_scan_excl<Acc>(acc, Acc{}, AddOp{}, sha, atot);
  if (threadIdx.x == 0) tiles[blockIdx.x].acc = atot;
}

// The three launches over `n_scan_tiles` tiles; the metric's finish kernel follows on the same stream.
template <typename P>
inline void tie_scan_launch(const uint64_t* keys, TieTile<P>* tiles, int64_t n, int n_scan_tiles, const typename P::Args& args,
                            hipStream_t s) {
  hipLaunchKernelGGL(tie_tile_counts_kernel<P>, dim3(n_scan_tiles), dim3(256), 0, s, keys, tiles, n);
  hipLaunchKernelGGL(tie_tiles_scan_kernel<P>, dim3(1), dim3(256), 0, s, tiles, n_scan_tiles);
  hipLaunchKernelGGL(tie_visit_kernel<P>, dim3(n_scan_tiles), dim3(256), 0, s, keys, tiles, n, args);
}

}  // namespace
