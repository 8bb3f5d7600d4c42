// kernels_region_table.hip - the table of defect regions on gfx950: one record per 8-connected component of each image's mask
// (area, bounding box, coordinate sums, overlap with a second mask, peak score and where it is).  The definitions the code
// follows are DESIGN.md "Defect regions".
//
// 1. The labelling of kernels_pixel_pro.hip, stages 1a - 1c (srad_label_roots): parent[i] = the root of pixel i, the smallest
//    linear index of its component.  A copy of parent[] as the tile stage left it is kept: each pixel's root within its own
//    32 x 32 tile, which is a pixel of that tile and so names an LDS slot.
// 2. Rank: record k belongs to the k-th root in linear order, i.e. by image and then by the region's first pixel in raster order.
//    An exclusive scan of the flag parent[i] == i over all pixels: counts per 4096-pixel tile, one block over the tile counts
//    (it also writes R and min(R, cap)), and a pass that stores the rank at each root (into the labelling's size words, which
//    are free by then) and has the root's thread write the record's starting values.
// 3. Accumulate: a block per 32 x 32 tile.  A thread folds its four pixels in registers while they share a tile root; a wave
//    then folds the lanes that share the tile root of its first active lane with shuffles (one region filling the tile: four
//    LDS updates per field and tile, not 1024); what is left updates the slot of its tile root in LDS.  After a barrier every
//    non-empty slot adds its sums into the record of its region: one global atomic per (tile, tile-local component) and field,
//    never one per pixel.  The sums of coordinates are kept tile-relative in u32 and widened at the flush.
// 4. Decode: the peak was kept as a u64 maximum of order_key(score) << 32 | ~index, so among equal scores (-0.0 == +0.0) the
//    smallest index wins; one thread per record turns it into (peak, peak_y, peak_x).
//
// Every accumulation is an integer sum, minimum or maximum: the table has the same bits on every call.  A NaN score inside a
// region is counted, never a peak; the host side refuses it.
#include "engine.h"
#include "../../include/srad.h"
#include "pixel_sort.h"
#include "pixel_pro.h"
#include <algorithm>
#include <limits.h>

namespace {

// srad_region_record while it is accumulated: the u64 peak key lies where peak_y and peak_x will be
struct RecAcc {
  int32_t image;
  uint32_t area;
  int32_t y0, x0, y1, x1;
  unsigned long long sum_y, sum_x;
  uint32_t overlap, peak;
  unsigned long long key;
};
static_assert(sizeof(RecAcc) == 56 && sizeof(srad_region_record) == 56, "record layout");
static_assert(offsetof(RecAcc, key) == offsetof(srad_region_record, peak_y), "the key overlays peak_y, peak_x");
static_assert(offsetof(RecAcc, sum_y) == offsetof(srad_region_record, sum_y), "record layout");

constexpr int kRankItems = 16, kRankTile = 256 * kRankItems;                 // 4096 pixels per rank tile
constexpr uint32_t kNanBits = 0x7FC00000u;

struct RtLayout {
  int n_rank_tiles;
  size_t parent, rank, tile_root, tsum, total;
};
RtLayout rt_layout(int64_t n) {
  RtLayout L{};
  L.n_rank_tiles = (int)((n + kRankTile - 1) / kRankTile);
  size_t o = 0;
  L.parent = o;    o += srad_align_up((size_t)n * 4, 256);
  L.rank = o;      o += srad_align_up((size_t)n * 4, 256);                   // the labelling's size words, then the ranks
  L.tile_root = o; o += srad_align_up((size_t)n * 4, 256);
  L.tsum = o;      o += srad_align_up((size_t)L.n_rank_tiles * 4, 256);
  L.total = o;
  return L;
}

// ---------------------------------------------------------------- 2. rank of the roots
// bit k: pixel b + k is a root (an ok pixel holds kNoParent, which is no index)
__device__ __forceinline__ uint32_t root_bits(const uint32_t* __restrict__ parent, int64_t b, int64_t n) {
  uint32_t bits = 0;
#pragma unroll
  for (int k = 0; k < kRankItems; ++k)
    if (b + k < n && parent[b + k] == (uint32_t)(b + k)) bits |= 1u << k;
  return bits;
}

__global__ __launch_bounds__(256) void rank_count_kernel(const uint32_t* __restrict__ parent, int64_t n, uint32_t* __restrict__ tsum) {
  __shared__ uint32_t sh[256];
  const int64_t b = (int64_t)blockIdx.x * kRankTile + (int64_t)threadIdx.x * kRankItems;
  uint32_t total;
  block_scan_excl<uint32_t>((uint32_t)__popc(root_bits(parent, b, n)), 0u, AddOp{}, sh, total);
  if (threadIdx.x == 0) tsum[blockIdx.x] = total;
}

// one block: tsum -> its exclusive scan; counts = {R, (NaN count, zeroed before), min(R, cap)}
__global__ __launch_bounds__(256) void rank_top_kernel(uint32_t* __restrict__ tsum, int nt, int64_t cap,
                                                       unsigned long long* __restrict__ counts) {
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
  if (threadIdx.x == 0) {
    counts[0] = carry;
    counts[2] = std::min<unsigned long long>(carry, (unsigned long long)cap);
  }
}

// rank[root] = its rank; the records that will be written start empty
__global__ __launch_bounds__(256) void rank_apply_kernel(const uint32_t* __restrict__ parent, int64_t n, const uint32_t* __restrict__ tsum,
                                                         uint32_t* __restrict__ rank, RecAcc* __restrict__ rec, int64_t cap, int64_t HW) {
  __shared__ uint32_t sh[256];
  const int64_t b = (int64_t)blockIdx.x * kRankTile + (int64_t)threadIdx.x * kRankItems;
  const uint32_t bits = root_bits(parent, b, n);
  uint32_t total;
  uint32_t run = tsum[blockIdx.x] + block_scan_excl<uint32_t>((uint32_t)__popc(bits), 0u, AddOp{}, sh, total);
#pragma unroll
  for (int k = 0; k < kRankItems; ++k) {
    if (!((bits >> k) & 1u)) continue;
    rank[b + k] = run;
    if ((int64_t)run < cap) rec[run] = RecAcc{(int32_t)((b + k) / HW), 0u, INT_MAX, INT_MAX, -1, -1, 0ull, 0ull, 0u, 0u, 0ull};
    ++run;
  }
}

// ---------------------------------------------------------------- 3. accumulate
struct MinOp { template <typename T> __device__ T operator()(T a, T b) const { return a < b ? a : b; } };

template <typename T, typename Op>
__device__ __forceinline__ T wave_all(T v, Op op) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o));
  return v;
}

// What a thread, then a wave, holds of one tile-local component; coordinates are tile-relative.
struct Agg {
  uint32_t cnt, y0, x0, y1, x1, sy, sx, ov;
  unsigned long long pk;
};
__device__ __forceinline__ Agg agg_empty() { return Agg{0u, (uint32_t)kLabT, (uint32_t)kLabT, 0u, 0u, 0u, 0u, 0u, 0ull}; }

struct AggLds {
  uint32_t cnt[kLabPx], y0[kLabPx], x0[kLabPx], y1[kLabPx], x1[kLabPx], sy[kLabPx], sx[kLabPx], ov[kLabPx];
  unsigned long long pk[kLabPx];
};
__device__ __forceinline__ void lds_add(AggLds& t, int slot, const Agg& a) {
  atomicAdd(&t.cnt[slot], a.cnt);
  atomicMin(&t.y0[slot], a.y0);
  atomicMin(&t.x0[slot], a.x0);
  atomicMax(&t.y1[slot], a.y1);
  atomicMax(&t.x1[slot], a.x1);
  atomicAdd(&t.sy[slot], a.sy);
  atomicAdd(&t.sx[slot], a.sx);
  if (a.ov) atomicAdd(&t.ov[slot], a.ov);
  if (a.pk) atomicMax(&t.pk[slot], a.pk);
}

// One 32 x 32 tile per block, the tiles and the thread -> pixel map of mask_local_kernel.
__global__ __launch_bounds__(256) void region_accumulate_kernel(const uint8_t* __restrict__ masks, const float* __restrict__ scores,
                                                                const uint8_t* __restrict__ other, LabGeom g,
                                                                const uint32_t* __restrict__ tile_root, const uint32_t* __restrict__ parent,
                                                                const uint32_t* __restrict__ rank, RecAcc* __restrict__ rec, int64_t cap,
                                                                unsigned long long* __restrict__ counts) {
  __shared__ AggLds t;
  __shared__ uint32_t n_nan;
  int64_t base;
  int y0, x0;
  lab_tile(g, base, y0, x0);
#pragma unroll
  for (int j = 0; j < kLabPx / 256; ++j) {
    const int li = threadIdx.x + 256 * j;
    t.cnt[li] = 0u;
    t.y0[li] = (uint32_t)kLabT;
    t.x0[li] = (uint32_t)kLabT;
    t.y1[li] = 0u;
    t.x1[li] = 0u;
    t.sy[li] = 0u;
    t.sx[li] = 0u;
    t.ov[li] = 0u;
    t.pk[li] = 0ull;
  }
  if (threadIdx.x == 0) n_nan = 0u;
  __syncthreads();

  int cur = -1;                                                  // the slot `a` belongs to
  Agg a = agg_empty();
  uint32_t nan = 0;
#pragma unroll
  for (int j = 0; j < kLabPx / 256; ++j) {
    const int li = threadIdx.x + 256 * j, ly = li / kLabT, lx = li % kLabT, y = y0 + ly, x = x0 + lx;
    if (y >= g.H || x >= g.W) continue;
    const int64_t gi = base + (int64_t)y * g.W + x;
    if (!masks[gi]) continue;
    const uint32_t l = tile_root[gi] - (uint32_t)base, lry = l / (uint32_t)g.W;
    const int slot = (int)(lry - (uint32_t)y0) * kLabT + (int)(l - lry * (uint32_t)g.W - (uint32_t)x0);
    if (slot != cur) {
      if (cur >= 0) lds_add(t, cur, a);
      cur = slot;
      a = agg_empty();
    }
    ++a.cnt;
    a.y0 = min(a.y0, (uint32_t)ly);
    a.x0 = min(a.x0, (uint32_t)lx);
    a.y1 = max(a.y1, (uint32_t)ly);
    a.x1 = max(a.x1, (uint32_t)lx);
    a.sy += (uint32_t)ly;
    a.sx += (uint32_t)lx;
    if (other && other[gi]) ++a.ov;
    if (scores) {
      const uint32_t k = order_key(scores[gi]);
      if (k == kNanKey) ++nan;
      else a.pk = max(a.pk, ((unsigned long long)k << 32) | (uint32_t)~(uint32_t)gi);
    }
  }
  // The lanes that share the slot of the first active lane fold into one update (wave-uniform branches).
  bool active = cur >= 0;
  const uint64_t any = __builtin_amdgcn_ballot_w64(active);
  if (any != 0ull) {
    const int lane = threadIdx.x & 63, lead = __ffsll((unsigned long long)any) - 1;
    const int s0 = __shfl(cur, lead);
    const bool member = active && cur == s0;
    if (__popcll(__builtin_amdgcn_ballot_w64(member)) > 1) {
      const Agg m = member ? a : agg_empty();
      Agg w;
      w.cnt = wave_all(m.cnt, AddOp{});
      w.y0 = wave_all(m.y0, MinOp{});
      w.x0 = wave_all(m.x0, MinOp{});
      w.y1 = wave_all(m.y1, MaxOp{});
      w.x1 = wave_all(m.x1, MaxOp{});
      w.sy = wave_all(m.sy, AddOp{});
      w.sx = wave_all(m.sx, AddOp{});
      w.ov = wave_all(m.ov, AddOp{});
      w.pk = wave_all(m.pk, MaxOp{});
      if (lane == lead) lds_add(t, s0, w);
      if (member) active = false;
    }
  }
  if (active) lds_add(t, cur, a);
  if (nan) atomicAdd(&n_nan, nan);
  __syncthreads();

  // one update of its region's record per non-empty slot
#pragma unroll
  for (int j = 0; j < kLabPx / 256; ++j) {
    const int li = threadIdx.x + 256 * j;
    const uint32_t c = t.cnt[li];
    if (c == 0u) continue;
    const int64_t gi = base + (int64_t)(y0 + li / kLabT) * g.W + x0 + li % kLabT;
    const uint32_t k = rank[parent[gi]];
    if ((int64_t)k >= cap) continue;
    RecAcc* r = rec + k;
    atomicAdd(&r->area, c);
    atomicMin(&r->y0, y0 + (int)t.y0[li]);
    atomicMin(&r->x0, x0 + (int)t.x0[li]);
    atomicMax(&r->y1, y0 + (int)t.y1[li]);
    atomicMax(&r->x1, x0 + (int)t.x1[li]);
    atomicAdd(&r->sum_y, (unsigned long long)c * (unsigned)y0 + t.sy[li]);
    atomicAdd(&r->sum_x, (unsigned long long)c * (unsigned)x0 + t.sx[li]);
    if (t.ov[li]) atomicAdd(&r->overlap, t.ov[li]);
    if (t.pk[li]) atomicMax(&r->key, t.pk[li]);
  }
  if (threadIdx.x == 0 && n_nan) atomicAdd(&counts[1], (unsigned long long)n_nan);
}

// ---------------------------------------------------------------- 4. decode the peak
__global__ __launch_bounds__(256) void region_decode_kernel(RecAcc* __restrict__ rec, const unsigned long long* __restrict__ counts,
                                                            int64_t HW, int W) {
  const int64_t m = (int64_t)counts[2];
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < m; k += (int64_t)gridDim.x * blockDim.x) {
    const unsigned long long key = rec[k].key;
    const int32_t image = rec[k].image;
    srad_region_record* out = reinterpret_cast<srad_region_record*>(rec + k);
    if (key == 0ull) {                                           // no scores, or NaN scores only: no finite score has key 0
      rec[k].peak = kNanBits;
      out->peak_y = -1;
      out->peak_x = -1;
    } else {
      const int64_t p = (int64_t)(uint32_t)~(uint32_t)key - (int64_t)image * HW;
      rec[k].peak = __float_as_uint(key_to_float((uint32_t)(key >> 32)));
      out->peak_y = (int32_t)(p / W);
      out->peak_x = (int32_t)(p % W);
    }
  }
}

}  // namespace

extern "C" {

int srad_region_table_workspace_bytes(int n_img, int H, int W, size_t* bytes) {
  int64_t n;
  SRAD_TRY(check_shape(n_img, H, W, "region_table_workspace_bytes", n));
  SRAD_REQUIRE(bytes, "region_table_workspace_bytes: bytes is NULL");
  *bytes = rt_layout(n).total;
  return SRAD_OK;
}

int srad_region_table(const uint8_t* masks, const float* scores, const uint8_t* other, int n_img, int H, int W,
                      srad_region_record* records_out, int64_t cap, uint64_t* counts_out, void* workspace, size_t workspace_bytes,
                      void* stream) {
  SRAD_REQUIRE(masks && counts_out && workspace, "region_table: NULL masks, counts_out or workspace");
  SRAD_REQUIRE(cap >= 0, "region_table: cap = %lld, must be >= 0", (long long)cap);
  SRAD_REQUIRE(records_out || cap == 0, "region_table: NULL records_out with cap = %lld", (long long)cap);
  int64_t n;
  SRAD_TRY(check_shape(n_img, H, W, "region_table", n));
  const RtLayout L = rt_layout(n);
  SRAD_REQUIRE(workspace_bytes >= L.total, "region_table: workspace %zu bytes, %zu needed", workspace_bytes, L.total);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  char* ws = reinterpret_cast<char*>(workspace);
  uint32_t* parent = reinterpret_cast<uint32_t*>(ws + L.parent);
  uint32_t* rank = reinterpret_cast<uint32_t*>(ws + L.rank);
  uint32_t* tile_root = reinterpret_cast<uint32_t*>(ws + L.tile_root);
  uint32_t* tsum = reinterpret_cast<uint32_t*>(ws + L.tsum);
  unsigned long long* counts = reinterpret_cast<unsigned long long*>(counts_out);
  RecAcc* rec = reinterpret_cast<RecAcc*>(records_out);
  const LabGeom g = lab_geom(H, W);
  const unsigned n_tiles = (unsigned)((int64_t)n_img * g.tiles_x * g.tiles_y);
  // the labelling (masks 3 times, parent and sizes as in launch_regions), the copy, parent twice more for the rank, then masks,
  // tile roots and, where given, scores and the other mask once
  SradProfScope prof(s, SRAD_K_SCORE, 0.0, 3.0 * n + 16.0 * n + 8.0 * n + 8.0 * n + 5.0 * n + (scores ? 4.0 * n : 0.0) + (other ? 1.0 * n : 0.0));
  SRAD_CHECK_HIP(hipMemsetAsync(counts, 0, 3 * sizeof(unsigned long long), s));
  SRAD_TRY(srad_label_roots(masks, n_img, H, W, parent, rank, tile_root, s));
  hipLaunchKernelGGL(rank_count_kernel, dim3(L.n_rank_tiles), dim3(256), 0, s, parent, n, tsum);
  hipLaunchKernelGGL(rank_top_kernel, dim3(1), dim3(256), 0, s, tsum, L.n_rank_tiles, cap, counts);
  hipLaunchKernelGGL(rank_apply_kernel, dim3(L.n_rank_tiles), dim3(256), 0, s, parent, n, tsum, rank, rec, cap, (int64_t)H * W);
  hipLaunchKernelGGL(region_accumulate_kernel, dim3(n_tiles), dim3(256), 0, s, masks, scores, other, g, tile_root, parent, rank, rec,
                     cap, counts);                                // with cap == 0 too: the NaN count
  if (cap > 0) {
    const unsigned grid = (unsigned)std::min<int64_t>((std::min<int64_t>(cap, n) + 255) / 256, 1024);
    hipLaunchKernelGGL(region_decode_kernel, dim3(grid), dim3(256), 0, s, rec, counts, (int64_t)H * W, W);
  }
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

}  // extern "C"
