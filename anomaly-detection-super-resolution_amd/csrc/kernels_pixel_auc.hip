// kernels_pixel_auc.hip - exact pixel-level ROC-AUC on gfx950: sklearn.metrics.roc_auc_score of a float32 score per pixel
// against a binary ground-truth mask, as the Mann-Whitney U with ties counted one half (the statistic srad_roc_auc computes on
// the host for a few hundred image scores).  A pixel split has 10^6 - 10^8 elements, so the ranking is a device sort.
//
// 1. Each score becomes an order-preserving u32 (sign flip; -0.0 -> +0.0; every NaN -> 0xFFFFFFFF, which no number maps to),
//    the label its low bit: a 33-bit key in a u64, so within a tie the negatives come before the positives.
// 2. LSD radix sort of the keys, 3 passes of 11-bit digits.  A pass is a per-tile LDS histogram (tile = 8192 keys), an exclusive
//    scan of the [digit][tile] count matrix, and a stable scatter: a tile is walked in rounds of 4 x 64 consecutive keys, a key's
//    rank among the equal digits of its wave comes from 11 ballots, and the waves of a round are ordered through LDS counters.
// 3. One scan of the sorted keys.  For a positive at sorted position i, every negative of its tie group sits before it, so
//        2 * (negatives below its score) + (negatives equal to it) = neg_before(i) + neg_before(start of its tie group),
//    with neg_before(start of the group) = a running max of neg_before over group heads (neg_before never decreases).
//    twice_U sums that over the positives.  All counts are integers: the result is exact and does not depend on input order.
//
// NaN scores sort last and are left out of n_pos, n_neg and twice_U; n_nan counts them, and the host side refuses them.
#include "engine.h"
#include "../../include/srad.h"
#include <algorithm>
#include <math.h>

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

__global__ __launch_bounds__(256) void auc_keys_kernel(const float* __restrict__ scores, const uint8_t* __restrict__ labels,
                                                       uint64_t* __restrict__ keys, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    keys[i] = ((uint64_t)order_key(scores[i]) << 1) | (labels[i] != 0 ? 1u : 0u);
}

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

// ---- the Mann-Whitney scan over the sorted keys, in scan tiles of 4096 (thread t: keys t * 16 .. t * 16 + 15) ----
struct AucTile {
  uint32_t neg, pos, nan;
  int32_t last_head;     // neg_before (within the tile) at the tile's last group head, -1 if no group starts in the tile
  uint32_t neg_off;      // negatives before the tile
  uint32_t lt_in;        // neg_before at the last group head before the tile
  uint64_t twice_u;
};
__device__ __forceinline__ bool is_head(const uint64_t* keys, int64_t i, uint64_t k) {
  return i == 0 || (keys[i - 1] >> 1) != (k >> 1);
}

__global__ __launch_bounds__(256) void auc_tile_counts_kernel(const uint64_t* __restrict__ keys, AucTile* __restrict__ tiles, int64_t n) {
  __shared__ uint32_t sh[256];
  __shared__ int32_t shi[256];
  const int64_t b = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
  uint32_t neg = 0, pos = 0, nan = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    if (b + k < n) {
      const uint64_t key = keys[b + k];
      if ((uint32_t)(key >> 1) == kNanKey) ++nan;
      else if (key & 1u) ++pos;
      else ++neg;
    }
  }
  uint32_t tneg, tpos, tnan;
  uint32_t e = block_scan_excl<uint32_t>(neg, 0u, AddOp{}, sh, tneg);
  block_scan_excl<uint32_t>(pos, 0u, AddOp{}, sh, tpos);
  block_scan_excl<uint32_t>(nan, 0u, AddOp{}, sh, tnan);
  int32_t last = -1;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    if (b + k < n) {
      const uint64_t key = keys[b + k];
      if ((uint32_t)(key >> 1) != kNanKey) {
        if (is_head(keys, b + k, key)) last = (int32_t)e;
        if (!(key & 1u)) ++e;
      }
    }
  }
  int32_t tlast;
  block_scan_excl<int32_t>(last, -1, MaxOp{}, shi, tlast);
  if (threadIdx.x == 0) {
    AucTile t{};
    t.neg = tneg; t.pos = tpos; t.nan = tnan; t.last_head = tlast;
    tiles[blockIdx.x] = t;
  }
}

// one block: negatives before each tile (sum scan) and neg_before at the last group head before each tile (max scan)
__global__ __launch_bounds__(256) void auc_tiles_scan_kernel(AucTile* __restrict__ tiles, int nt) {
  __shared__ uint32_t sh[256];
  uint32_t neg_carry = 0, lt_carry = 0;
  for (int c0 = 0; c0 < nt; c0 += 256) {
    const int t = c0 + threadIdx.x;
    const AucTile x = t < nt ? tiles[t] : AucTile{0, 0, 0, -1, 0, 0, 0};
    uint32_t ntot;
    const uint32_t off = neg_carry + block_scan_excl<uint32_t>(x.neg, 0u, AddOp{}, sh, ntot);
    const uint32_t hv = x.last_head >= 0 ? off + (uint32_t)x.last_head : 0u;
    uint32_t htot;
    const uint32_t lt = std::max(lt_carry, block_scan_excl<uint32_t>(hv, 0u, MaxOp{}, sh, htot));
    if (t < nt) { tiles[t].neg_off = off; tiles[t].lt_in = lt; }
    neg_carry += ntot;
    lt_carry = std::max(lt_carry, htot);
  }
}

__global__ __launch_bounds__(256) void auc_tile_u_kernel(const uint64_t* __restrict__ keys, AucTile* __restrict__ tiles, int64_t n) {
  __shared__ uint32_t sh[256];
  __shared__ uint64_t shu[256];
  const int64_t b = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
  const uint32_t off = tiles[blockIdx.x].neg_off, lt_in = tiles[blockIdx.x].lt_in;
  uint32_t neg = 0, hv = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    if (b + k < n) {
      const uint64_t key = keys[b + k];
      if ((uint32_t)(key >> 1) != kNanKey && !(key & 1u)) ++neg;
    }
  }
  uint32_t tot;
  uint32_t e = off + block_scan_excl<uint32_t>(neg, 0u, AddOp{}, sh, tot);     // neg_before of this thread's first key
  {
    uint32_t ee = e;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
      if (b + k < n) {
        const uint64_t key = keys[b + k];
        if ((uint32_t)(key >> 1) != kNanKey) {
          if (is_head(keys, b + k, key)) hv = ee;
          if (!(key & 1u)) ++ee;
        }
      }
    }
  }
  uint32_t htot;
  uint32_t lt = std::max(lt_in, block_scan_excl<uint32_t>(hv, 0u, MaxOp{}, sh, htot));
  uint64_t u = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    if (b + k < n) {
      const uint64_t key = keys[b + k];
      if ((uint32_t)(key >> 1) != kNanKey) {
        if (is_head(keys, b + k, key)) lt = e;
        if (key & 1u) u += (uint64_t)e + lt;
        else ++e;
      }
    }
  }
  uint64_t utot;
  block_scan_excl<uint64_t>(u, 0ull, AddOp{}, shu, utot);
  if (threadIdx.x == 0) tiles[blockIdx.x].twice_u = utot;
}

__global__ __launch_bounds__(256) void auc_finish_kernel(const AucTile* __restrict__ tiles, int nt, uint64_t* __restrict__ counts,
                                                         double* __restrict__ auc) {
  __shared__ uint64_t sh[256];
  uint64_t pos = 0, neg = 0, nan = 0, u = 0;
  for (int t = threadIdx.x; t < nt; t += 256) {
    pos += tiles[t].pos; neg += tiles[t].neg; nan += tiles[t].nan; u += tiles[t].twice_u;
  }
  uint64_t tp, tn, tx, tu;
  block_scan_excl<uint64_t>(pos, 0ull, AddOp{}, sh, tp);
  block_scan_excl<uint64_t>(neg, 0ull, AddOp{}, sh, tn);
  block_scan_excl<uint64_t>(nan, 0ull, AddOp{}, sh, tx);
  block_scan_excl<uint64_t>(u, 0ull, AddOp{}, sh, tu);
  if (threadIdx.x == 0) {
    counts[0] = tp; counts[1] = tn; counts[2] = tx; counts[3] = tu;
    *auc = (tp == 0 || tn == 0) ? NAN : (double)tu / (2.0 * (double)tp * (double)tn);
  }
}

struct AucLayout {
  int n_sort_tiles, n_scan_tiles, n_count_tiles;
  int64_t m;                                                     // entries of the [digit][tile] count matrix
  size_t keys_a, keys_b, offs, tsum, tiles, total;
};
AucLayout auc_layout(int64_t n) {
  AucLayout L{};
  L.n_sort_tiles = (int)((n + kSortTile - 1) / kSortTile);
  L.n_scan_tiles = (int)((n + kScanTile - 1) / kScanTile);
  L.m = (int64_t)kDigits * L.n_sort_tiles;
  L.n_count_tiles = (int)((L.m + kScanTile - 1) / kScanTile);
  size_t o = 0;
  L.keys_a = o; o += srad_align_up((size_t)n * 8, 256);
  L.keys_b = o; o += srad_align_up((size_t)n * 8, 256);
  L.offs = o;   o += srad_align_up((size_t)L.m * 4, 256);
  L.tsum = o;   o += srad_align_up((size_t)L.n_count_tiles * 4, 256);
  L.tiles = o;  o += srad_align_up((size_t)L.n_scan_tiles * sizeof(AucTile), 256);
  L.total = o;
  return L;
}

}  // namespace

extern "C" {

int srad_pixel_auc_workspace_bytes(int64_t n, size_t* bytes) {
  SRAD_REQUIRE(bytes && n > 0 && n <= INT32_MAX, "pixel_auc_workspace_bytes: bad argument (n = %lld)", (long long)n);
  *bytes = auc_layout(n).total;
  return SRAD_OK;
}

int srad_pixel_roc_auc(const float* scores, const uint8_t* labels, int64_t n, uint64_t* counts_out, double* auc_out, void* workspace,
                       size_t workspace_bytes, void* stream) {
  SRAD_REQUIRE(scores && labels && counts_out && auc_out && workspace, "pixel_roc_auc: bad argument");
  SRAD_REQUIRE(n > 0 && n <= INT32_MAX, "pixel_roc_auc: n = %lld, must be in [1, 2^31)", (long long)n);
  const AucLayout L = auc_layout(n);
  SRAD_REQUIRE(workspace_bytes >= L.total, "pixel_roc_auc: workspace %zu bytes, %zu needed", workspace_bytes, L.total);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  char* ws = reinterpret_cast<char*>(workspace);
  uint64_t* ka = reinterpret_cast<uint64_t*>(ws + L.keys_a);
  uint64_t* kb = reinterpret_cast<uint64_t*>(ws + L.keys_b);
  uint32_t* offs = reinterpret_cast<uint32_t*>(ws + L.offs);
  uint32_t* tsum = reinterpret_cast<uint32_t*>(ws + L.tsum);
  AucTile* tiles = reinterpret_cast<AucTile*>(ws + L.tiles);
  {
    SradProfScope prof(s, SRAD_K_SCORE, 0.0, 13.0 * n);
    const unsigned g = (unsigned)std::min<int64_t>((n + 255) / 256, 8192);
    hipLaunchKernelGGL(auc_keys_kernel, dim3(g), dim3(256), 0, s, scores, labels, ka, n);
  }
  uint64_t* src = ka;
  uint64_t* dst = kb;
  for (int p = 0; p < kPasses; ++p) {
    // key bytes: read twice (histogram, scatter), written once; the count matrix: written, scanned (read + written), read
    SradProfScope prof(s, SRAD_K_SCORE, 0.0, 24.0 * n + 16.0 * L.m);
    const int shift = p * kDigitBits;
    hipLaunchKernelGGL(radix_hist_kernel, dim3(L.n_sort_tiles), dim3(256), 0, s, src, offs, n, shift, L.n_sort_tiles);
    hipLaunchKernelGGL(scan_reduce_kernel, dim3(L.n_count_tiles), dim3(256), 0, s, offs, tsum, L.m);
    hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(256), 0, s, tsum, L.n_count_tiles);
    hipLaunchKernelGGL(scan_apply_kernel, dim3(L.n_count_tiles), dim3(256), 0, s, offs, tsum, L.m);
    hipLaunchKernelGGL(radix_scatter_kernel, dim3(L.n_sort_tiles), dim3(256), 0, s, src, dst, offs, n, shift, L.n_sort_tiles);
    std::swap(src, dst);
  }
  {
    SradProfScope prof(s, SRAD_K_SCORE, 0.0, 16.0 * n);
    hipLaunchKernelGGL(auc_tile_counts_kernel, dim3(L.n_scan_tiles), dim3(256), 0, s, src, tiles, n);
    hipLaunchKernelGGL(auc_tiles_scan_kernel, dim3(1), dim3(256), 0, s, tiles, L.n_scan_tiles);
    hipLaunchKernelGGL(auc_tile_u_kernel, dim3(L.n_scan_tiles), dim3(256), 0, s, src, tiles, n);
    hipLaunchKernelGGL(auc_finish_kernel, dim3(1), dim3(256), 0, s, tiles, L.n_scan_tiles, counts_out, auc_out);
  }
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

}  // extern "C"
