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
#include "pixel_sort.h"
#include <algorithm>
#include <math.h>

namespace {

__global__ __launch_bounds__(256) void auc_keys_kernel(const float* __restrict__ scores, const uint8_t* __restrict__ labels,
                                                       uint64_t* __restrict__ keys, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    keys[i] = ((uint64_t)order_key(scores[i]) << 1) | (labels[i] != 0 ? 1u : 0u);
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
    radix_sort_pass(src, dst, offs, tsum, n, p * kDigitBits, L.n_sort_tiles, s);
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
