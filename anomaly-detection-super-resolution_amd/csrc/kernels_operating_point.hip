// kernels_operating_point.hip - a threshold for the anomaly maps and the operating point it gives, on gfx950.  The definitions
// the code follows are DESIGN.md "Operating point".
//
// 1. srad_select_kth: the value of ascending rank k of n float32 scores, exactly, by radix select over order_key(score)
//    (pixel_sort.h; -0.0 == +0.0, a NaN keeps 0xFFFFFFFF and sorts last).  Three passes over the scores, on the key's top 11,
//    middle 11 and low 10 bits; each pass counts the digits of the keys that carry the prefix chosen so far (LDS histogram per
//    block, then one global integer atomic per non-empty bin and block), and a one-block kernel picks the digit that holds the
//    rank and updates {prefix, residual rank, keys below} in the workspace.  Nothing is moved, nothing n-sized is stored, and
//    the host never waits between the passes.  The maps have huge tie groups (most pixels are exactly 0.0), so before the LDS
//    atomic a wave peels its two leading digits: the lanes that share the digit of the first active lane add once, together.
//    All sums are integers, so the result does not depend on the schedule.
// 2. srad_operating_point: pred = score > t; with min_area > 1 the 8-connected components of pred (srad_mask_regions itself)
//    smaller than min_area are removed; with masks their regions give |region| and R; one counting pass (a block per 8192-pixel
//    chunk of one image, block sums, then one block over the block sums) gives tp, fp, fn, the NaN count, the surviving pixels
//    per image and the 128-bit fixed-point per-region overlap numerator of AU-PRO (pixel_pro.h).
#include "engine.h"
#include "../../include/srad.h"
#include "pixel_sort.h"
#include "pixel_pro.h"
#include <algorithm>
#include <math.h>

namespace {

// ---------------------------------------------------------------- 1. radix select
__host__ __device__ constexpr int sel_bits(int pass) { return pass == 2 ? 10 : 11; }                 // digit widths, from the top
__host__ __device__ constexpr int sel_shift(int pass) { return pass == 0 ? 21 : (pass == 1 ? 10 : 0); }
constexpr int kSelBins = 2048;
constexpr int kSelPerBlock = 4096, kSelMaxBlocks = 512;       // at most 512 blocks add into one global bin

struct SelState {
  uint32_t prefix, rank, n_nan, pad;
  uint64_t below;
};
struct SelLayout {
  size_t hist, state, total;
};
SelLayout sel_layout() {
  SelLayout L{};
  L.hist = 0;
  L.state = srad_align_up((size_t)3 * kSelBins * 4, 256);
  L.total = L.state + srad_align_up(sizeof(SelState), 256);
  return L;
}

// h[d] += 1 for every active lane, called by whole waves.  Two rounds peel the digit of the first lane still active: its lanes
// add their count once.  What is left (few lanes, unless the data has no ties) adds lane by lane.
__device__ __forceinline__ void hist_add(uint32_t* h, bool active, uint32_t d) {
  const int lane = threadIdx.x & 63;
  uint64_t rem = __builtin_amdgcn_ballot_w64(active);
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    if (rem == 0ull) break;                                    // wave-uniform
    const int lead = __ffsll((unsigned long long)rem) - 1;
    const uint32_t d0 = (uint32_t)__shfl((int)d, lead);
    const uint64_t same = __builtin_amdgcn_ballot_w64(active && d == d0);
    if (lane == lead) atomicAdd(&h[d0], (uint32_t)__popcll(same));
    if (d == d0) active = false;
    rem &= ~same;
  }
  if (active) atomicAdd(&h[d], 1u);
}

// hist[d] += keys whose bits above `shift + bits` equal the prefix (pass 0: every key) and whose digit at `shift` is d
__global__ __launch_bounds__(256) void select_hist_kernel(const float* __restrict__ scores, int64_t n, int pass,
                                                          uint32_t* __restrict__ hist, SelState* __restrict__ st) {
  __shared__ uint32_t h[kSelBins];
  for (int d = threadIdx.x; d < kSelBins; d += 256) h[d] = 0u;
  const int shift = sel_shift(pass), bits = sel_bits(pass);
  const uint32_t dmask = (1u << bits) - 1u, prefix = pass ? st->prefix : 0u;
  __syncthreads();
  uint32_t nan = 0;
  for (int64_t base = (int64_t)blockIdx.x * 1024; base < n; base += (int64_t)gridDim.x * 1024) {   // block-uniform trip count
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t i = base + j * 256 + threadIdx.x;
      v[j] = i < n ? scores[i] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t i = base + j * 256 + threadIdx.x;
      const uint32_t key = order_key(v[j]);
      // the bits above the digit, in two shifts that both stay below 32
      const bool match = i < n && (pass == 0 || ((key >> shift) >> bits) == prefix);
      if (pass == 0 && i < n && key == kNanKey) ++nan;
      hist_add(h, match, (key >> shift) & dmask);
    }
  }
  __syncthreads();
  for (int d = threadIdx.x; d < kSelBins; d += 256)
    if (h[d]) atomicAdd(&hist[d], h[d]);
  if (nan) atomicAdd(&st->n_nan, nan);
}

// One block: the digit whose bin holds the rank.  Thread t sums bins t * per .. t * per + per - 1 (per = 8 or 4).
__global__ __launch_bounds__(256) void select_pick_kernel(const uint32_t* __restrict__ hist, SelState* __restrict__ st, int pass,
                                                          uint32_t k, float* __restrict__ value_out,
                                                          unsigned long long* __restrict__ counts_out) {
  __shared__ uint32_t sh[256];
  const int bits = sel_bits(pass), per = (1 << bits) / 256;
  const uint32_t rank = pass ? st->rank : k, prefix = pass ? st->prefix : 0u;
  const uint64_t below = pass ? st->below : 0ull;
  uint32_t c[8], s = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    c[j] = j < per ? hist[threadIdx.x * per + j] : 0u;
    s += c[j];
  }
  uint32_t total;
  // the barriers inside the scan order every thread's reads of *st above before the one write below
  uint32_t run = block_scan_excl<uint32_t>(s, 0u, AddOp{}, sh, total);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (j < per && rank >= run && rank < run + c[j]) {                      // true in exactly one (thread, j): rank < total
      const uint32_t key = (prefix << bits) | (uint32_t)(threadIdx.x * per + j);
      st->prefix = key;
      st->rank = rank - run;
      st->below = below + run;
      if (pass == 2) {
        const bool is_nan = key == kNanKey;
        *value_out = key_to_float(key);
        counts_out[0] = st->n_nan;
        counts_out[1] = below + run;
        counts_out[2] = is_nan ? 0ull : c[j];                               // the NaN are counted once, in n_nan
      }
    }
    run += c[j];
  }
}

// ---------------------------------------------------------------- 2. operating point
constexpr int kOpChunk = 8192;                                  // pixels of one image per counting block

struct OpPart {
  uint64_t tp, fp, fn, nan, lo, hi;
};
struct OpLayout {
  int chunks;                                                   // counting blocks per image
  size_t size, rws, rcounts, parts, total;
};
OpLayout op_layout(int n_img, int H, int W, int64_t n) {
  OpLayout L{};
  L.chunks = (int)(((int64_t)H * W + kOpChunk - 1) / kOpChunk);
  size_t o = 0;
  L.size = o;    o += srad_align_up((size_t)n * 4, 256);         // region sizes: of the prediction, then of the masks
  L.rws = o;     o += srad_align_up((size_t)n * 4, 256);         // srad_mask_regions' own workspace
  L.rcounts = o; o += 256;
  L.parts = o;   o += srad_align_up((size_t)n_img * L.chunks * sizeof(OpPart), 256);
  L.total = o;
  return L;
}

__global__ __launch_bounds__(256) void op_threshold_kernel(const float* __restrict__ scores, float t, uint8_t* __restrict__ pred,
                                                           int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    pred[i] = scores[i] > t ? 1 : 0;                             // false for a NaN score
}

// size[i] = pixels of the predicted component of pixel i, 0 off the prediction
__global__ __launch_bounds__(256) void op_drop_small_kernel(uint8_t* __restrict__ pred, const uint32_t* __restrict__ size,
                                                            uint32_t min_area, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    pred[i] = size[i] >= min_area ? 1 : 0;
}

// Block b counts chunk b % chunks of image b / chunks.  masks / region_size are NULL together (no ground truth: every pixel ok).
__global__ __launch_bounds__(256) void op_count_kernel(const float* __restrict__ scores, const uint8_t* __restrict__ masks,
                                                       const uint8_t* __restrict__ pred, const uint32_t* __restrict__ region_size,
                                                       int64_t HW, int chunks, OpPart* __restrict__ parts,
                                                       uint32_t* __restrict__ img_pred) {
  __shared__ Pref shp[256];
  __shared__ uint32_t sh[256];
  const int img = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
  const int64_t p0 = (int64_t)chunk * kOpChunk, p1 = std::min<int64_t>(HW, p0 + kOpChunk), base = (int64_t)img * HW;
  uint32_t tp = 0, fp = 0, fn = 0, nan = 0, np = 0;
  Pref pro{};
  for (int64_t p = p0 + threadIdx.x; p < p1; p += 256) {
    const int64_t i = base + p;
    const float v = scores[i];
    const bool is_pred = pred[i] != 0, defect = masks && masks[i] != 0;
    np += is_pred;
    if (v != v) {                                                // a NaN is in no count; it is never predicted
      ++nan;
      continue;
    }
    tp += is_pred && defect;
    fp += is_pred && !defect;
    fn += !is_pred && defect;
    if (is_pred && defect) pro_add(pro, region_size[i]);         // |region| >= 1 on a defect pixel
  }
  uint32_t ttp, tfp, tfn, tnan, tnp;
  Pref tpro;
  block_scan_excl<uint32_t>(tp, 0u, AddOp{}, sh, ttp);
  block_scan_excl<uint32_t>(fp, 0u, AddOp{}, sh, tfp);
  block_scan_excl<uint32_t>(fn, 0u, AddOp{}, sh, tfn);
  block_scan_excl<uint32_t>(nan, 0u, AddOp{}, sh, tnan);
  block_scan_excl<uint32_t>(np, 0u, AddOp{}, sh, tnp);
  block_scan_excl<Pref>(pro, Pref{}, PrefAdd{}, shp, tpro);
  if (threadIdx.x == 0) {
    parts[blockIdx.x] = OpPart{ttp, tfp, tfn, tnan, tpro.lo, tpro.hi};
    if (chunks == 1) img_pred[img] = tnp;
    else if (tnp) atomicAdd(&img_pred[img], tnp);                // zeroed before; integer adds, one per block
  }
}

// one block: counts_out = {tp, fp, fn, tn, n_nan, n_regions, pro_hi, pro_lo}
__global__ __launch_bounds__(256) void op_finish_kernel(const OpPart* __restrict__ parts, int n_parts, int64_t n,
                                                        const unsigned long long* __restrict__ region_counts,
                                                        unsigned long long* __restrict__ counts_out) {
  __shared__ Pref shp[256];
  __shared__ uint64_t shu[256];
  uint64_t tp = 0, fp = 0, fn = 0, nan = 0;
  Pref pro{};
  for (int b = threadIdx.x; b < n_parts; b += 256) {
    const OpPart x = parts[b];
    tp += x.tp;
    fp += x.fp;
    fn += x.fn;
    nan += x.nan;
    pro = PrefAdd{}(pro, Pref{x.lo, x.hi, 0, 0});
  }
  uint64_t ttp, tfp, tfn, tnan;
  Pref tpro;
  block_scan_excl<uint64_t>(tp, 0ull, AddOp{}, shu, ttp);
  block_scan_excl<uint64_t>(fp, 0ull, AddOp{}, shu, tfp);
  block_scan_excl<uint64_t>(fn, 0ull, AddOp{}, shu, tfn);
  block_scan_excl<uint64_t>(nan, 0ull, AddOp{}, shu, tnan);
  block_scan_excl<Pref>(pro, Pref{}, PrefAdd{}, shp, tpro);
  if (threadIdx.x == 0) {
    counts_out[0] = ttp;
    counts_out[1] = tfp;
    counts_out[2] = tfn;
    counts_out[3] = (uint64_t)n - tnan - ttp - tfp - tfn;
    counts_out[4] = tnan;
    counts_out[5] = region_counts ? region_counts[0] : 0ull;
    counts_out[6] = tpro.hi;
    counts_out[7] = tpro.lo;
  }
}

}  // namespace

extern "C" {

int srad_select_kth_workspace_bytes(int64_t n, size_t* bytes) {
  SRAD_REQUIRE(n > 0 && n <= INT32_MAX, "select_kth_workspace_bytes: n = %lld, must be in [1, 2^31)", (long long)n);
  SRAD_REQUIRE(bytes, "select_kth_workspace_bytes: bytes is NULL");
  *bytes = sel_layout().total;
  return SRAD_OK;
}

int srad_select_kth(const float* scores, int64_t n, int64_t k, float* value_out, uint64_t* counts_out, void* workspace,
                    size_t workspace_bytes, void* stream) {
  SRAD_REQUIRE(scores && value_out && counts_out && workspace, "select_kth: NULL scores, value_out, counts_out or workspace");
  SRAD_REQUIRE(n > 0 && n <= INT32_MAX, "select_kth: n = %lld, must be in [1, 2^31)", (long long)n);
  SRAD_REQUIRE(k >= 0 && k < n, "select_kth: rank k = %lld, must be in [0, n = %lld)", (long long)k, (long long)n);
  const SelLayout L = sel_layout();
  SRAD_REQUIRE(workspace_bytes >= L.total, "select_kth: workspace %zu bytes, %zu needed", workspace_bytes, L.total);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  char* ws = reinterpret_cast<char*>(workspace);
  uint32_t* hist = reinterpret_cast<uint32_t*>(ws + L.hist);
  SelState* st = reinterpret_cast<SelState*>(ws + L.state);
  const unsigned grid = (unsigned)std::min<int64_t>((n + kSelPerBlock - 1) / kSelPerBlock, kSelMaxBlocks);
  SradProfScope prof(s, SRAD_K_SCORE, 0.0, 12.0 * n);           // the scores, three times
  SRAD_CHECK_HIP(hipMemsetAsync(ws, 0, L.total, s));
  for (int p = 0; p < 3; ++p) {
    hipLaunchKernelGGL(select_hist_kernel, dim3(grid), dim3(256), 0, s, scores, n, p, hist + p * kSelBins, st);
    hipLaunchKernelGGL(select_pick_kernel, dim3(1), dim3(256), 0, s, hist + p * kSelBins, st, p, (uint32_t)k, value_out,
                       reinterpret_cast<unsigned long long*>(counts_out));
  }
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

int srad_operating_point_workspace_bytes(int n_img, int H, int W, size_t* bytes) {
  int64_t n;
  SRAD_TRY(check_shape(n_img, H, W, "operating_point_workspace_bytes", n));
  SRAD_REQUIRE(bytes, "operating_point_workspace_bytes: bytes is NULL");
  *bytes = op_layout(n_img, H, W, n).total;
  return SRAD_OK;
}

int srad_operating_point(const float* scores, const uint8_t* masks, int n_img, int H, int W, float threshold, int min_area,
                         uint8_t* pred_out, uint32_t* img_pred_out, uint64_t* counts_out, void* workspace, size_t workspace_bytes,
                         void* stream) {
  SRAD_REQUIRE(scores && pred_out && img_pred_out && counts_out && workspace,
               "operating_point: NULL scores, pred_out, img_pred_out, counts_out or workspace");
  SRAD_REQUIRE(threshold == threshold, "operating_point: the threshold is NaN");
  SRAD_REQUIRE(min_area >= 1, "operating_point: min_area = %d, must be >= 1", min_area);
  int64_t n;
  SRAD_TRY(check_shape(n_img, H, W, "operating_point", n));
  const OpLayout L = op_layout(n_img, H, W, n);
  SRAD_REQUIRE(workspace_bytes >= L.total, "operating_point: workspace %zu bytes, %zu needed", workspace_bytes, L.total);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  char* ws = reinterpret_cast<char*>(workspace);
  uint32_t* size = reinterpret_cast<uint32_t*>(ws + L.size);
  uint64_t* rcounts = reinterpret_cast<uint64_t*>(ws + L.rcounts);
  OpPart* parts = reinterpret_cast<OpPart*>(ws + L.parts);
  const size_t rws_bytes = srad_align_up((size_t)n * 4, 256);
  const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 8192);
  {
    SradProfScope prof(s, SRAD_K_SCORE, 0.0, 5.0 * n);
    hipLaunchKernelGGL(op_threshold_kernel, dim3(grid), dim3(256), 0, s, scores, threshold, pred_out, n);
  }
  if (min_area > 1) {
    SRAD_TRY(srad_mask_regions(pred_out, n_img, H, W, size, rcounts, ws + L.rws, rws_bytes, stream));
    SradProfScope prof(s, SRAD_K_SCORE, 0.0, 6.0 * n);
    hipLaunchKernelGGL(op_drop_small_kernel, dim3(grid), dim3(256), 0, s, pred_out, size, (uint32_t)min_area, n);
  }
  if (masks) SRAD_TRY(srad_mask_regions(masks, n_img, H, W, size, rcounts, ws + L.rws, rws_bytes, stream));
  {
    SradProfScope prof(s, SRAD_K_SCORE, 0.0, (masks ? 10.0 : 5.0) * n);
    const int n_parts = n_img * L.chunks;
    if (L.chunks > 1) SRAD_CHECK_HIP(hipMemsetAsync(img_pred_out, 0, (size_t)n_img * 4, s));
    hipLaunchKernelGGL(op_count_kernel, dim3(n_parts), dim3(256), 0, s, scores, masks, pred_out, masks ? size : nullptr,
                       (int64_t)H * W, L.chunks, parts, img_pred_out);
    hipLaunchKernelGGL(op_finish_kernel, dim3(1), dim3(256), 0, s, parts, n_parts, n,
                       masks ? reinterpret_cast<const unsigned long long*>(rcounts) : nullptr,
                       reinterpret_cast<unsigned long long*>(counts_out));
  }
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

}  // extern "C"
