// kernels_pixel_auc.hip - exact pixel-level ROC-AUC on gfx950: sklearn.metrics.roc_auc_score of a float32 score per pixel
// against a binary ground-truth mask, as the Mann-Whitney U with ties counted one half (the statistic srad_roc_auc computes on
// the host for a few hundred image scores).  A pixel split has 10^6 - 10^8 elements, so the ranking is a device sort.
//
// 1. Each score becomes an order-preserving u32 (sign flip; -0.0 -> +0.0; every NaN -> 0xFFFFFFFF, which no number maps to),
//    the label its low bit: a 33-bit key in a u64.
// 2. LSD radix sort of the keys, 3 passes of 11-bit digits at shifts 0 / 11 / 22 (pixel_sort.h), so the scores ascend and the
//    label bit orders the keys of a tie (an order the scan does not rely on).
// 3. The tie-group scan of the sorted keys (tie_scan.h) with the prefix (negatives, positives) and the keys of one score as a
//    group.  A group g with pos_g positives and neg_g negatives, above neg_below_g negatives of lower score, adds
//        pos_g * (2 * neg_below_g + neg_g) = (pos at its end - pos before its head) * (neg before its head + neg at its end)
//    to twice_U.  All counts are integers: the result is exact and does not depend on input order.
//
// NaN scores sort last and are left out of n_pos, n_neg and twice_U; n_nan counts them, and the host side refuses them.
#include "engine.h"
#include "../../include/srad.h"
#include "tie_scan.h"
#include <algorithm>
#include <math.h>

namespace {

__global__ __launch_bounds__(256) void auc_keys_kernel(const float* __restrict__ scores, const uint8_t* __restrict__ labels,
                                                       uint64_t* __restrict__ keys, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    keys[i] = ((uint64_t)order_key(scores[i]) << 1) | (labels[i] != 0 ? 1u : 0u);
}

// The Mann-Whitney sum as a tie_scan.h policy.  Prefix: negatives << 32 | positives so far; both stay below 2^31, so the words
// never carry into each other and the larger u64 is the later position.
struct AucScan {
  using Prefix = uint64_t;
  using Add = AddOp;
  using Max = MaxOp;
  using Acc = uint64_t;
  struct Args {};
  __device__ explicit AucScan(const Args&) {}
  static __device__ __forceinline__ uint32_t group(uint64_t key) { return (uint32_t)(key >> 1); }
  static __device__ __forceinline__ void add(Prefix& p, uint64_t key) { p += (key & 1u) ? 1ull : 1ull << 32; }
  __device__ __forceinline__ Acc at_end(Prefix before_head, Prefix through_end, int64_t, uint64_t) const {
    return (uint64_t)((uint32_t)through_end - (uint32_t)before_head) * ((before_head >> 32) + (through_end >> 32));
  }
};
using AucTile = TieTile<AucScan>;

__global__ __launch_bounds__(256) void auc_finish_kernel(const AucTile* __restrict__ tiles, int nt, uint64_t* __restrict__ counts,
                                                         double* __restrict__ auc) {
  __shared__ uint64_t sh[256];
  uint64_t sum = 0, nan = 0, u = 0;
  for (int t = threadIdx.x; t < nt; t += 256) {
    sum += tiles[t].sum; nan += tiles[t].nan; u += tiles[t].acc;
  }
  uint64_t ts, tx, tu;
  block_scan_excl<uint64_t>(sum, 0ull, AddOp{}, sh, ts);
  block_scan_excl<uint64_t>(nan, 0ull, AddOp{}, sh, tx);
  block_scan_excl<uint64_t>(u, 0ull, AddOp{}, sh, tu);
  if (threadIdx.x == 0) {
    const uint64_t tp = (uint32_t)ts, tn = ts >> 32;
    counts[0] = tp; counts[1] = tn; counts[2] = tx; counts[3] = tu;
    *auc = (tp == 0 || tn == 0) ? NAN : (double)tu / (2.0 * (double)tp * (double)tn);
  }
}

}  // namespace

extern "C" {

int srad_pixel_auc_workspace_bytes(int64_t n, size_t* bytes) {
  SRAD_REQUIRE(bytes && n > 0 && n <= INT32_MAX, "pixel_auc_workspace_bytes: bad argument (n = %lld)", (long long)n);
  *bytes = sorted_keys_layout(n, sizeof(AucTile)).total;
  return SRAD_OK;
}

int srad_pixel_roc_auc(const float* scores, const uint8_t* labels, int64_t n, uint64_t* counts_out, double* auc_out, void* workspace,
                       size_t workspace_bytes, void* stream) {
  SRAD_REQUIRE(scores && labels && counts_out && auc_out && workspace, "pixel_roc_auc: bad argument");
  SRAD_REQUIRE(n > 0 && n <= INT32_MAX, "pixel_roc_auc: n = %lld, must be in [1, 2^31)", (long long)n);
  const SortedKeysLayout L = sorted_keys_layout(n, sizeof(AucTile));
  SRAD_REQUIRE(workspace_bytes >= L.total, "pixel_roc_auc: workspace %zu bytes, %zu needed", workspace_bytes, L.total);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  char* ws = reinterpret_cast<char*>(workspace);
  AucTile* tiles = reinterpret_cast<AucTile*>(ws + L.tiles);
  {
    SradProfScope prof(s, SRAD_K_SCORE, 0.0, 13.0 * n);
    const unsigned g = (unsigned)std::min<int64_t>((n + 255) / 256, 8192);
    hipLaunchKernelGGL(auc_keys_kernel, dim3(g), dim3(256), 0, s, scores, labels, reinterpret_cast<uint64_t*>(ws + L.keys_a), n);
  }
  const uint64_t* sorted = radix_sort_keys(ws, L, n, 0, s);
  {
    SradProfScope prof(s, SRAD_K_SCORE, 0.0, 16.0 * n);
    tie_scan_launch<AucScan>(sorted, tiles, n, L.n_scan_tiles, AucScan::Args{}, s);
    hipLaunchKernelGGL(auc_finish_kernel, dim3(1), dim3(256), 0, s, tiles, L.n_scan_tiles, counts_out, auc_out);
  }
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

}  // extern "C"
