// kernels_pixel_pro.hip - AU-PRO on gfx950: the area under the per-region overlap curve up to a false-positive rate L, divided
// by L (Bergmann et al., "The MVTec Anomaly Detection Dataset", IJCV 2021), of float32 scores [n, H, W] against ground-truth
// masks [n, H, W] (nonzero = defect).  The definition the code follows is DESIGN.md "AU-PRO".
//
// 1. Regions: the 8-connected components of each image's mask, by union-find whose links always point to the smaller linear
//    index, so a root is its component's minimum index whatever the schedule.
//    a. mask_local: a 32 x 32 tile is labelled in LDS (atomicMin union-find over tile-local indices), each tile-local component
//       is counted in LDS, and the tile writes parent[] = the global index of each pixel's local root and, at a local root, the
//       component's pixel count.
//    b. mask_merge: the pixels of a tile's left column and top row union with their 8-neighbours in the tiles to the left and
//       above, atomicMin on the global parent[].  Other workgroups (on other XCDs, behind other L2s) link concurrently, so
//       parent[] is read with agent-scope atomic loads.
//    c. mask_flatten (own launch): parent[g] = root, and each local root adds its count to the root's size word - one atomic
//       per (tile, component), never one per pixel.
//    d. mask_sizes: the size of every pixel's region (0 for ok pixels) and the counts {regions, ok pixels, defect pixels}.
//    Neighbours are taken in (image, y, x) coordinates: nothing connects across a row end or an image end.
// 2. Keys: (~order_key(score)) << 32 | region size.  An ascending sort of the high words walks the scores from highest down
//    (a NaN keeps 0xFFFFFFFF, which no number maps to, and sorts last).  Three radix passes at shifts 32 / 43 / 54 (pixel_sort.h);
//    the sort is stable, so the region size rides along in the low word.
// 3. The tie-group scan of the sorted keys (tie_scan.h), with the pixels of one score as a group.  The prefix: an ok pixel adds
//    1 to the fpr numerator (u64); a pixel of region r adds floor(2^64 / |r|) to the pro numerator, a 128-bit fixed-point sum.
//    Integer addition is associative, so the curve does not depend on the order of the pixels inside a tie group or of the
//    images; the error against the exact rational is below n 2^-64 / R.  The curve's points are the ends of tie groups, and the
//    predecessor of a group end is the previous group end, i.e. the prefix just before its own group's head, which is what the
//    scan hands over.  Each segment's trapezoid (and the one interpolated at L) is computed in float64, and the areas are
//    reduced in a fixed tree order.
//
// NaN scores are left out of the curve and counted in n_nan; the host side refuses them.
#include "engine.h"
#include "../../include/srad.h"
#include "tie_scan.h"
#include "pixel_pro.h"
#include <algorithm>
#include <math.h>

namespace {

// ---------------------------------------------------------------- 1. regions
constexpr int kLabPer = kLabPx / 256;                                       // 4 pixels per thread (kLabT, LabGeom: pixel_pro.h)

__device__ __forceinline__ int lds_find(int* lab, int x) {
  int p = __hip_atomic_load(&lab[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  while (p != x) {
    x = p;
    p = __hip_atomic_load(&lab[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  return x;
}
// Link the larger root under the smaller.  If b stopped being a root before the atomicMin landed, `old` is its new parent and
// b now points at min(old, a): union a with old in the next round, so no link is lost.
__device__ void lds_union(int* lab, int a, int b) {
  for (;;) {
    a = lds_find(lab, a);
    b = lds_find(lab, b);
    if (a == b) return;
    if (a > b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(&lab[b], a);
    if (old == b) return;
    b = old;
  }
}

__device__ __forceinline__ uint32_t ld_agent(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t g_find(const uint32_t* parent, uint32_t x) {
  uint32_t p = ld_agent(&parent[x]);
  while (p != x) {
    x = p;
    p = ld_agent(&parent[x]);
  }
  return x;
}
__device__ void g_union(uint32_t* parent, uint32_t a, uint32_t b) {                 // lds_union on the global parent[]
  for (;;) {
    a = g_find(parent, a);
    b = g_find(parent, b);
    if (a == b) return;
    if (a > b) {
      const uint32_t t = a;
      a = b;
      b = t;
    }
    const uint32_t old = __hip_atomic_fetch_min(&parent[b], a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == b) return;
    b = old;
  }
}

// One 32 x 32 tile per block; thread t holds tile pixels t, t + 256, t + 512, t + 768 (row-major in the tile).
__global__ __launch_bounds__(256) void mask_local_kernel(const uint8_t* __restrict__ masks, LabGeom g, uint32_t* __restrict__ parent,
                                                         uint32_t* __restrict__ size) {
  __shared__ int lab[kLabPx];
  __shared__ uint32_t cnt[kLabPx];
  __shared__ uint8_t dm[kLabPx];
  int64_t base;
  int y0, x0;
  lab_tile(g, base, y0, x0);
  bool def[kLabPer];
#pragma unroll
  for (int j = 0; j < kLabPer; ++j) {
    const int li = threadIdx.x + 256 * j, y = y0 + li / kLabT, x = x0 + li % kLabT;
    def[j] = y < g.H && x < g.W && masks[base + (int64_t)y * g.W + x] != 0;
    dm[li] = def[j];
    lab[li] = def[j] ? li : -1;
    cnt[li] = 0u;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kLabPer; ++j) {
    const int li = threadIdx.x + 256 * j, ly = li / kLabT, lx = li % kLabT;
    if (!def[j]) continue;
    if (lx > 0 && dm[li - 1]) lds_union(lab, li, li - 1);                          // W
    if (ly > 0) {
      if (lx > 0 && dm[li - kLabT - 1]) lds_union(lab, li, li - kLabT - 1);        // NW
      if (dm[li - kLabT]) lds_union(lab, li, li - kLabT);                          // N
      if (lx < kLabT - 1 && dm[li - kLabT + 1]) lds_union(lab, li, li - kLabT + 1);  // NE
    }
  }
  __syncthreads();
  int root[kLabPer];
#pragma unroll
  for (int j = 0; j < kLabPer; ++j) {
    root[j] = def[j] ? lds_find(lab, threadIdx.x + 256 * j) : -1;
    if (def[j]) atomicAdd(&cnt[root[j]], 1u);
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kLabPer; ++j) {
    const int li = threadIdx.x + 256 * j, y = y0 + li / kLabT, x = x0 + li % kLabT;
    if (y >= g.H || x >= g.W) continue;
    const int64_t gi = base + (int64_t)y * g.W + x;
    const int r = root[j];
    parent[gi] = def[j] ? (uint32_t)(base + (int64_t)(y0 + r / kLabT) * g.W + x0 + r % kLabT) : kNoParent;
    size[gi] = (def[j] && r == li) ? cnt[li] : 0u;
  }
}

// One 64-thread block per tile: threads 0..31 take the tile's left column (neighbours x - 1, y - 1 .. y + 1), threads 32..63 its
// top row (neighbours x - 1 .. x + 1, y - 1).  Together they cover every 8-adjacent pair that crosses a tile border.
__global__ __launch_bounds__(64) void mask_merge_kernel(const uint8_t* __restrict__ masks, LabGeom g, uint32_t* __restrict__ parent) {
  int64_t base;
  int y0, x0;
  lab_tile(g, base, y0, x0);
  const bool col = threadIdx.x < kLabT;
  const int y = col ? y0 + (int)threadIdx.x : y0, x = col ? x0 : x0 + (int)threadIdx.x - kLabT;
  if ((col ? x0 : y0) == 0 || y >= g.H || x >= g.W) return;
  const int64_t p = base + (int64_t)y * g.W + x;
  if (!masks[p]) return;
  for (int k = -1; k <= 1; ++k) {
    const int ny = col ? y + k : y - 1, nx = col ? x - 1 : x + k;
    if (ny < 0 || ny >= g.H || nx < 0 || nx >= g.W) continue;
    const int64_t q = base + (int64_t)ny * g.W + nx;
    if (masks[q]) g_union(parent, (uint32_t)p, (uint32_t)q);
  }
}

// All links are in place: point every defect pixel at its root, and add each non-root local root's count into the root's size
// word.  Only roots receive adds, and a non-root's own count is read only by its own thread.
__global__ __launch_bounds__(256) void mask_flatten_kernel(const uint8_t* __restrict__ masks, uint32_t* __restrict__ parent,
                                                           uint32_t* __restrict__ size, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if (!masks[i]) continue;
    const uint32_t p = ld_agent(&parent[i]);
    if (p == (uint32_t)i) continue;
    const uint32_t r = g_find(parent, p);
    if (r != p) __hip_atomic_store(&parent[i], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t c = size[i];
    if (c) atomicAdd(&size[r], c);
  }
}

// Every pixel's region size (0 for ok pixels): into `out` (may be `size` itself: only a root's word is read, and a root's thread
// writes back the value it holds), or with `scores` into the sort keys.  counts (zeroed before) += {regions, ok, defect}.
__global__ __launch_bounds__(256) void mask_sizes_kernel(const uint8_t* __restrict__ masks, const uint32_t* __restrict__ parent,
                                                         const uint32_t* size, int64_t n, uint32_t* out, const float* __restrict__ scores,
                                                         uint64_t* __restrict__ keys, unsigned long long* __restrict__ counts) {
  __shared__ uint32_t sh[256];
  uint32_t reg = 0, ok = 0, defect = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    uint32_t z = 0u;
    if (masks[i]) {
      const uint32_t r = parent[i];
      z = size[r];
      ++defect;
      reg += r == (uint32_t)i;
    } else {
      ++ok;
    }
    if (keys) keys[i] = ((uint64_t)desc_key(scores[i]) << 32) | z;
    else out[i] = z;
  }
  uint32_t treg, tok, tdef;
  block_scan_excl<uint32_t>(reg, 0u, AddOp{}, sh, treg);
  block_scan_excl<uint32_t>(ok, 0u, AddOp{}, sh, tok);
  block_scan_excl<uint32_t>(defect, 0u, AddOp{}, sh, tdef);
  if (threadIdx.x == 0) {
    atomicAdd(&counts[0], (unsigned long long)treg);
    atomicAdd(&counts[1], (unsigned long long)tok);
    atomicAdd(&counts[2], (unsigned long long)tdef);
  }
}

// ---------------------------------------------------------------- 3. the curve, as a tie_scan.h policy
// Pref, PrefAdd and pro_add (the 128-bit fixed-point pro numerator and the ok-pixel count) live in pixel_pro.h.
__device__ __forceinline__ bool pw_less(const Pref& a, const Pref& b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }
struct PrefMax {      // componentwise: both parts never decrease along the walk, so this is the value at the later position
  __device__ Pref operator()(const Pref& a, const Pref& b) const {
    const bool b_more = pw_less(a, b);
    return Pref{b_more ? b.lo : a.lo, b_more ? b.hi : a.hi, a.ok > b.ok ? a.ok : b.ok, 0};
  }
};

// (fpr, pro) of a prefix, each clipped at 1
__device__ __forceinline__ void pro_point(const Pref& p, double n_ok, double n_reg, double& f, double& r) {
  f = fmin(1.0, (double)p.ok / n_ok);
  r = fmin(1.0, ((double)p.hi + (double)p.lo * 0x1p-64) / n_reg);
}
// The part of the trapezoid (f0, p0) - (f1, p1) at fpr <= L; pro is interpolated at L in the one segment that crosses it.
__device__ __forceinline__ double seg_area(double f0, double p0, double f1, double p1, double L) {
  if (f1 <= L) return (f1 - f0) * (p0 + p1) * 0.5;
  if (f0 < L) {
    const double pl = p0 + (p1 - p0) * (L - f0) / (f1 - f0);
    return (L - f0) * (p0 + pl) * 0.5;
  }
  return 0.0;
}

// Each group end: its curve point, the segment from the previous group end, the curve write.
struct ProScan {
  using Prefix = Pref;
  using Add = PrefAdd;
  using Max = PrefMax;
  using Acc = double;
  struct Args {
    const unsigned long long* counts;      // {regions, ok pixels}, on the device
    double L;
    double *curve_fpr, *curve_pro;
    int64_t cap;
  };
  Args a;
  double n_reg, n_ok;
  __device__ explicit ProScan(const Args& args) : a(args), n_reg((double)args.counts[0]), n_ok((double)args.counts[1]) {}
  static __device__ __forceinline__ uint32_t group(uint64_t key) { return (uint32_t)(key >> 32); }
  static __device__ __forceinline__ void add(Pref& p, uint64_t key) { pro_add(p, key); }
  __device__ __forceinline__ double at_end(const Pref& before_head, const Pref& through_end, int64_t idx, uint64_t) const {
    double f0, p0, f1, p1;
    pro_point(before_head, n_ok, n_reg, f0, p0);
    pro_point(through_end, n_ok, n_reg, f1, p1);
    if (a.curve_fpr && idx + 1 < a.cap) {
      a.curve_fpr[idx + 1] = f1;
      a.curve_pro[idx + 1] = p1;
    }
    return seg_area(f0, p0, f1, p1, a.L);
  }
};
using ProTile = TieTile<ProScan>;

// one block: the areas in a fixed order, the last segment to (1, 1), the end points of the curve, the counts
__global__ __launch_bounds__(256) void pro_finish_kernel(const ProTile* __restrict__ tiles, int nt, unsigned long long* __restrict__ counts,
                                                         double L, double* __restrict__ aupro, double* __restrict__ curve_fpr,
                                                         double* __restrict__ curve_pro, int64_t cap) {
  __shared__ Pref shp[256];
  __shared__ uint64_t shu[256];
  __shared__ double shd[256];
  Pref sum{};
  uint64_t nan = 0, ends = 0;
  double area = 0.0;
  for (int t = threadIdx.x; t < nt; t += 256) {
    sum = PrefAdd{}(sum, tiles[t].sum);
    nan += tiles[t].nan;
    ends += tiles[t].ends;
    area += tiles[t].acc;
  }
  Pref tsum;
  uint64_t tnan, tends;
  double tarea;
  block_scan_excl<Pref>(sum, Pref{}, PrefAdd{}, shp, tsum);
  block_scan_excl<uint64_t>(nan, 0ull, AddOp{}, shu, tnan);
  block_scan_excl<uint64_t>(ends, 0ull, AddOp{}, shu, tends);
  block_scan_excl<double>(area, 0.0, AddOp{}, shd, tarea);
  if (threadIdx.x == 0) {
    const uint64_t n_reg = counts[0], n_ok = counts[1];
    double f0, p0;
    pro_point(tsum, (double)n_ok, (double)n_reg, f0, p0);
    tarea += seg_area(f0, p0, 1.0, 1.0, L);
    counts[3] = tnan;
    counts[4] = tends + 2;
    *aupro = (n_reg == 0 || n_ok == 0) ? NAN : tarea / L;
    if (curve_fpr && cap > 0) {
      curve_fpr[0] = 0.0;
      curve_pro[0] = 0.0;
    }
    if (curve_fpr && (int64_t)tends + 1 < cap) {
      curve_fpr[tends + 1] = 1.0;
      curve_pro[tends + 1] = 1.0;
    }
  }
}

// ---------------------------------------------------------------- host side
// Stages 1a - 1d.  parent: n u32 of workspace; size: n u32 (the output, or workspace when `keys` is given).
int launch_regions(const uint8_t* masks, int n_img, int H, int W, int64_t n, uint32_t* parent, uint32_t* size,
                   unsigned long long* counts, const float* scores, uint64_t* keys, hipStream_t s) {
  const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 8192);
  // masks read 4 times (local, merge borders, flatten, sizes); parent written, read twice, rewritten in part; sizes written,
  // read, written (or the 8-byte keys written, and the scores read)
  SradProfScope prof(s, SRAD_K_SCORE, 0.0, 4.0 * n + 16.0 * n + (keys ? 16.0 * n : 8.0 * n));
  SRAD_CHECK_HIP(hipMemsetAsync(counts, 0, 3 * sizeof(unsigned long long), s));
  SRAD_TRY(srad_label_roots(masks, n_img, H, W, parent, size, nullptr, s));
  hipLaunchKernelGGL(mask_sizes_kernel, dim3(std::min(grid, 1024u)), dim3(256), 0, s, masks, parent, size, n, size, scores, keys,
                     counts);
  return SRAD_OK;
}

}  // namespace

// Stages 1a - 1c (declared in pixel_pro.h).
int srad_label_roots(const uint8_t* masks, int n_img, int H, int W, uint32_t* parent, uint32_t* size, uint32_t* tile_root,
                     hipStream_t s) {
  const int64_t n = (int64_t)n_img * H * W;
  const LabGeom g = lab_geom(H, W);
  const unsigned n_tiles = (unsigned)((int64_t)n_img * g.tiles_x * g.tiles_y);
  const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 8192);
  hipLaunchKernelGGL(mask_local_kernel, dim3(n_tiles), dim3(256), 0, s, masks, g, parent, size);
  if (tile_root) SRAD_CHECK_HIP(hipMemcpyAsync(tile_root, parent, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
  hipLaunchKernelGGL(mask_merge_kernel, dim3(n_tiles), dim3(64), 0, s, masks, g, parent);
  hipLaunchKernelGGL(mask_flatten_kernel, dim3(grid), dim3(256), 0, s, masks, parent, size, n);
  return SRAD_OK;
}

extern "C" {

int srad_mask_regions_workspace_bytes(int n_img, int H, int W, size_t* bytes) {
  int64_t n;
  SRAD_TRY(check_shape(n_img, H, W, "mask_regions_workspace_bytes", n));
  SRAD_REQUIRE(bytes, "mask_regions_workspace_bytes: bytes is NULL");
  *bytes = srad_align_up((size_t)n * 4, 256);
  return SRAD_OK;
}

int srad_mask_regions(const uint8_t* masks, int n_img, int H, int W, uint32_t* region_size_out, uint64_t* counts_out,
                      void* workspace, size_t workspace_bytes, void* stream) {
  SRAD_REQUIRE(masks && region_size_out && counts_out && workspace, "mask_regions: NULL masks, region_size_out, counts_out or workspace");
  int64_t n;
  SRAD_TRY(check_shape(n_img, H, W, "mask_regions", n));
  const size_t need = srad_align_up((size_t)n * 4, 256);
  SRAD_REQUIRE(workspace_bytes >= need, "mask_regions: workspace %zu bytes, %zu needed", workspace_bytes, need);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  SRAD_TRY(launch_regions(masks, n_img, H, W, n, reinterpret_cast<uint32_t*>(workspace), region_size_out,
                          reinterpret_cast<unsigned long long*>(counts_out), nullptr, nullptr, s));
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

int srad_pixel_pro_workspace_bytes(int n_img, int H, int W, size_t* bytes) {
  int64_t n;
  SRAD_TRY(check_shape(n_img, H, W, "pixel_pro_workspace_bytes", n));
  SRAD_REQUIRE(bytes, "pixel_pro_workspace_bytes: bytes is NULL");
  *bytes = sorted_keys_layout(n, sizeof(ProTile)).total;
  return SRAD_OK;
}

int srad_pixel_pro(const float* scores, const uint8_t* masks, int n_img, int H, int W, double fpr_limit, uint64_t* counts_out,
                   double* aupro_out, double* curve_fpr, double* curve_pro, int64_t curve_cap, void* workspace,
                   size_t workspace_bytes, void* stream) {
  SRAD_REQUIRE(scores && masks && counts_out && aupro_out && workspace,
               "pixel_pro: NULL scores, masks, counts_out, aupro_out or workspace");
  SRAD_REQUIRE(fpr_limit > 0.0 && fpr_limit <= 1.0, "pixel_pro: fpr_limit = %g, must be in (0, 1]", fpr_limit);
  SRAD_REQUIRE((curve_fpr == nullptr) == (curve_pro == nullptr) && curve_cap >= 0,
               "pixel_pro: curve_fpr and curve_pro must both be given or both be NULL, curve_cap >= 0");
  int64_t n;
  SRAD_TRY(check_shape(n_img, H, W, "pixel_pro", n));
  const SortedKeysLayout L = sorted_keys_layout(n, sizeof(ProTile));
  SRAD_REQUIRE(workspace_bytes >= L.total, "pixel_pro: workspace %zu bytes, %zu needed", workspace_bytes, L.total);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  char* ws = reinterpret_cast<char*>(workspace);
  ProTile* tiles = reinterpret_cast<ProTile*>(ws + L.tiles);
  unsigned long long* counts = reinterpret_cast<unsigned long long*>(counts_out);
  if (!curve_fpr) curve_cap = 0;
  // the second key buffer is free until the first radix pass scatters into it: it holds parent[] and the region sizes
  uint32_t* parent = reinterpret_cast<uint32_t*>(ws + L.keys_b);
  SRAD_TRY(launch_regions(masks, n_img, H, W, n, parent, parent + n, counts, scores, reinterpret_cast<uint64_t*>(ws + L.keys_a), s));
  const uint64_t* sorted = radix_sort_keys(ws, L, n, 32, s);
  {
    SradProfScope prof(s, SRAD_K_SCORE, 0.0, 16.0 * n);
    tie_scan_launch<ProScan>(sorted, tiles, n, L.n_scan_tiles, ProScan::Args{counts, fpr_limit, curve_fpr, curve_pro, curve_cap}, s);
    hipLaunchKernelGGL(pro_finish_kernel, dim3(1), dim3(256), 0, s, tiles, L.n_scan_tiles, counts, fpr_limit, aupro_out, curve_fpr,
                       curve_pro, curve_cap);
  }
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

}  // extern "C"
