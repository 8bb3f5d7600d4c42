// kernels_pixel_pr.hip - exact pixel-level precision-recall on gfx950: sklearn.metrics.average_precision_score and the best F1
// over all thresholds (F1-max) of a float32 score per pixel against a binary ground-truth mask, and the curve itself.  The
// definition the code follows is DESIGN.md "Precision-recall".
//
// 1. Keys: (desc_key(score) << 1) | label, 33 bits in a u64, so an ascending sort walks the scores from the highest down (a NaN
//    keeps 0xFFFFFFFF, which no number maps to, and sorts last).
// 2. LSD radix sort of the keys, 3 passes of 11-bit digits at shifts 0 / 11 / 22 (pixel_sort.h).
// 3. The tie-group scan of the sorted keys (tie_scan.h) with the prefix (false positives, true positives) and the keys of one
//    score as a group.  The prefix through the end of a group is (tp, fp) of "predict iff score >= this score": one point of the
//    curve, precision tp / (tp + fp) and recall tp / P.  A group end adds
//        (tp at its end - tp before its head) * tp / (tp + fp)          (P times sklearn's (R_k - R_k-1) * P_k)
//    to the AP sum, in float64, and offers itself as the best-F1 point.  F1 = 2 tp / (tp + fp + P), and two points are compared
//    by cross-multiplying in u64, so the best point is exact and does not depend on input order; an exact tie goes to the earlier
//    group end, the higher threshold.
//
// NaN scores are left out of every count and counted in n_nan; the host side refuses them.
#include "engine.h"
#include "../../include/srad.h"
#include "tie_scan.h"
#include <algorithm>
#include <math.h>

namespace {

__global__ __launch_bounds__(256) void pr_keys_kernel(const float* __restrict__ scores, const uint8_t* __restrict__ labels,
                                                      uint64_t* __restrict__ keys, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    keys[i] = ((uint64_t)desc_key(scores[i]) << 1) | (labels[i] != 0 ? 1u : 0u);
}

// The float32 bits that desc_key maps to `k` (a zero comes back as +0.0).
__device__ __forceinline__ uint32_t desc_key_bits(uint32_t k) {
  const uint32_t o = ~k;                                         // order_key
  return (o & 0x80000000u) ? (o ^ 0x80000000u) : ~o;
}

// What the group ends of a stretch of the walk add up to: the AP sum, and the best-F1 point among them as (tp, den = tp + fp + P,
// the number of group ends before it, the score key).  den < 2^32 (tp + fp <= n < 2^31, P < 2^31), and a point has den >= 1, so
// den == 0 is "no point": PrAcc{} is the zero of +.
struct PrAcc {
  double ap;
  uint32_t tp, den, idx, key;
};
// F1_a vs F1_b as tp_a * den_b vs tp_b * den_a, both below 2^63; distinct points have distinct idx, so the order is total and +
// is associative and commutative in the point it keeps.
__device__ __forceinline__ PrAcc operator+(const PrAcc& a, const PrAcc& b) {
  const uint64_t fa = (uint64_t)a.tp * b.den, fb = (uint64_t)b.tp * a.den;
  const bool take_b = a.den == 0u || (b.den != 0u && (fb > fa || (fb == fa && b.idx < a.idx)));
  return PrAcc{a.ap + b.ap, take_b ? b.tp : a.tp, take_b ? b.den : a.den, take_b ? b.idx : a.idx, take_b ? b.key : a.key};
}
__device__ __forceinline__ PrAcc& operator+=(PrAcc& a, const PrAcc& b) { return a = a + b; }

// Prefix: false positives << 32 | true positives so far; both stay below 2^31, so the words never carry into each other and the
// larger u64 is the later position (as AucScan).  P, the positives of the whole walk, is the last tile's off + sum, which the
// one-block tile scan has written before the visiting pass starts.
struct PrScan {
  using Prefix = uint64_t;
  using Add = AddOp;
  using Max = MaxOp;
  using Acc = PrAcc;
  struct Args {
    const uint64_t *last_off, *last_sum;   // of the last scan tile, on the device
    double *precision, *recall;
    float* score;
    int64_t cap;
  };
  Args a;
  uint32_t n_pos;
  __device__ explicit PrScan(const Args& args) : a(args), n_pos((uint32_t)(*args.last_off + *args.last_sum)) {}
  static __device__ __forceinline__ uint32_t group(uint64_t key) { return (uint32_t)(key >> 1); }
  static __device__ __forceinline__ void add(Prefix& p, uint64_t key) { p += (key & 1u) ? 1ull : 1ull << 32; }
  __device__ __forceinline__ PrAcc at_end(Prefix before_head, Prefix through_end, int64_t idx, uint64_t key) const {
    const uint32_t tp = (uint32_t)through_end, fp = (uint32_t)(through_end >> 32), tp0 = (uint32_t)before_head;
    const double pred = (double)(tp + fp);                       // >= 1: the group has a key
    if (a.precision && idx < a.cap) {
      a.precision[idx] = (double)tp / pred;
      a.recall[idx] = (double)tp / (double)n_pos;
      a.score[idx] = __uint_as_float(desc_key_bits(group(key)));
    }
    return PrAcc{(double)(tp - tp0) * (double)tp / pred, tp, tp + fp + n_pos, (uint32_t)idx, group(key)};
  }
};
using PrTile = TieTile<PrScan>;

// one block: the tiles' sums in a fixed order (thread t takes tiles t, t + 256, ... in turn, then the block's tree)
__global__ __launch_bounds__(256) void pr_finish_kernel(const PrTile* __restrict__ tiles, int nt, uint64_t* __restrict__ counts,
                                                        double* __restrict__ ap) {
  __shared__ uint64_t sh[256];
  __shared__ PrAcc sha[256];
  uint64_t sum = 0, nan = 0, ends = 0;
  PrAcc acc{};
  for (int t = threadIdx.x; t < nt; t += 256) {
    sum += tiles[t].sum; nan += tiles[t].nan; ends += tiles[t].ends;
    acc += tiles[t].acc;
  }
  uint64_t ts, tx, te;
  PrAcc ta;
  block_scan_excl<uint64_t>(sum, 0ull, AddOp{}, sh, ts);
  block_scan_excl<uint64_t>(nan, 0ull, AddOp{}, sh, tx);
  block_scan_excl<uint64_t>(ends, 0ull, AddOp{}, sh, te);
  block_scan_excl<PrAcc>(acc, PrAcc{}, AddOp{}, sha, ta);
  if (threadIdx.x == 0) {
    const uint64_t n_pos = (uint32_t)ts, n_neg = ts >> 32;
    const bool any = ta.den != 0u;
    counts[0] = n_pos; counts[1] = n_neg; counts[2] = tx; counts[3] = te;
    counts[4] = ta.tp;
    counts[5] = any ? (uint64_t)ta.den - ta.tp - n_pos : 0ull;
    counts[6] = any ? desc_key_bits(ta.key) : 0u;
    *ap = n_pos == 0 ? NAN : ta.ap / (double)n_pos;
  }
}

}  // namespace

extern "C" {

int srad_pixel_pr_workspace_bytes(int64_t n, size_t* bytes) {
  SRAD_REQUIRE(bytes && n > 0 && n <= INT32_MAX, "pixel_pr_workspace_bytes: bad argument (n = %lld)", (long long)n);
  *bytes = sorted_keys_layout(n, sizeof(PrTile)).total;
  return SRAD_OK;
}

int srad_pixel_pr(const float* scores, const uint8_t* labels, int64_t n, uint64_t* counts_out, double* ap_out,
                  double* curve_precision, double* curve_recall, float* curve_score, int64_t curve_cap, void* workspace,
                  size_t workspace_bytes, void* stream) {
  SRAD_REQUIRE(scores && labels && counts_out && ap_out && workspace, "pixel_pr: NULL scores, labels, counts_out, ap_out or workspace");
  SRAD_REQUIRE(n > 0 && n <= INT32_MAX, "pixel_pr: n = %lld, must be in [1, 2^31)", (long long)n);
  SRAD_REQUIRE((curve_precision == nullptr) == (curve_recall == nullptr) && (curve_precision == nullptr) == (curve_score == nullptr) &&
                   curve_cap >= 0,
               "pixel_pr: curve_precision, curve_recall and curve_score must all be given or all be NULL, curve_cap >= 0");
  const SortedKeysLayout L = sorted_keys_layout(n, sizeof(PrTile));
  SRAD_REQUIRE(workspace_bytes >= L.total, "pixel_pr: workspace %zu bytes, %zu needed", workspace_bytes, L.total);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  char* ws = reinterpret_cast<char*>(workspace);
  PrTile* tiles = reinterpret_cast<PrTile*>(ws + L.tiles);
  if (!curve_precision) curve_cap = 0;
  {
    SradProfScope prof(s, SRAD_K_SCORE, 0.0, 13.0 * n);
    const unsigned g = (unsigned)std::min<int64_t>((n + 255) / 256, 8192);
    hipLaunchKernelGGL(pr_keys_kernel, dim3(g), dim3(256), 0, s, scores, labels, reinterpret_cast<uint64_t*>(ws + L.keys_a), n);
  }
  const uint64_t* sorted = radix_sort_keys(ws, L, n, 0, s);
  {
    SradProfScope prof(s, SRAD_K_SCORE, 0.0, 16.0 * n);
    const PrTile* last = tiles + (L.n_scan_tiles - 1);
    tie_scan_launch<PrScan>(sorted, tiles, n, L.n_scan_tiles,
                            PrScan::Args{&last->off, &last->sum, curve_precision, curve_recall, curve_score, curve_cap}, s);
    hipLaunchKernelGGL(pr_finish_kernel, dim3(1), dim3(256), 0, s, tiles, L.n_scan_tiles, counts_out, ap_out);
  }
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

}  // extern "C"
