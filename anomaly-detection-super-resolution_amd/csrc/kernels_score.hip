// kernels_score.hip - reconstruction-error scorer on gfx950 (reference src/evaluate.py:204-265,
// src/metrics.py:15-108, src/trainer.py:45-47).  HBM/L2-bound integer + fp work, no MFMA.
//
// SSIM window sweep: the reference evaluates ssim_numpy once per (image pair, window size) with a
// Python loop over every pixel (O(H W ws^2)).  Here each image pair gets five float64 summed-area
// tables (x, y, x*x, y*y, x*y of the luminance planes) built once; any window size is then 4 table
// look-ups per quantity and pixel, and numpy's "reflect" padding becomes at most 3 x 3 rectangles of
// the unpadded table (a window that hangs over an edge covers the reflected rows/columns a second
// time).  The per-pixel SSIM arithmetic is done in fp32 in the reference's operation order.
#include "engine.h"
#include "../../include/srad.h"
#include <algorithm>
#include <math.h>
#include <stdlib.h>
#include <type_traits>
#include <vector>

namespace {

constexpr int kQ = 5;            // x, y, xx, yy, xy
constexpr int kEvalPix = 1024;   // pixels per workgroup in the evaluation kernel

__device__ __forceinline__ float luma_of(const uint8_t* px, int C) {
  // hr.astype(float32) / 255.0, then tensordot with [65.738, 129.057, 25.064] / 256 (metrics.py:37-39)
  if (C == 1) return (float)px[0] / 255.0f;
  const float c0 = 65.738f / 256.0f, c1 = 129.057f / 256.0f, c2 = 25.064f / 256.0f;
  const float r = (float)px[0] / 255.0f, g = (float)px[1] / 255.0f, b = (float)px[2] / 255.0f;
  return r * c0 + g * c1 + b * c2;
}

// Table layout: planar, sat[img][q][row + 1][col + 1] (row 0 and column 0 are zero), so that the 64 lanes of a wave - 64
// consecutive pixels of a row - read and write 512 contiguous bytes per quantity.
//
// Row pass: one wave per (image, table row).  The row is walked in 64-pixel chunks; a chunk's five running sums are a
// 6-step wave scan (float64 shuffles) plus the carry of the chunks before it.
__global__ __launch_bounds__(256) void sat_rows_kernel(const uint8_t* __restrict__ sr, const uint8_t* __restrict__ hr,
                                                       double* __restrict__ sat, int n_img, int H, int W, int C) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= n_img * (H + 1)) return;
  const int img = t / (H + 1), r = t - img * (H + 1);
  const size_t plane = (size_t)(H + 1) * (W + 1);
  double* const base = sat + (size_t)img * kQ * plane + (size_t)r * (W + 1);
  if (r == 0) {
    for (int c = lane; c <= W; c += 64)
#pragma unroll
      for (int q = 0; q < kQ; ++q) base[q * plane + c] = 0.0;
    return;
  }
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < kQ; ++q) base[q * plane] = 0.0;
  }
  const uint8_t* ps = sr + ((size_t)img * H + (r - 1)) * W * C;
  const uint8_t* ph = hr + ((size_t)img * H + (r - 1)) * W * C;
  double carry[kQ] = {0, 0, 0, 0, 0};
  for (int c0 = 0; c0 < W; c0 += 64) {
    const int c = c0 + lane;
    double v[kQ] = {0, 0, 0, 0, 0};
    if (c < W) {
      const float x = luma_of(ph + (size_t)c * C, C);     // "ref" = HR
      const float y = luma_of(ps + (size_t)c * C, C);     // "out" = SR
      v[0] = (double)x; v[1] = (double)y;
      v[2] = (double)(x * x); v[3] = (double)(y * y); v[4] = (double)(x * y);    // fp32 products as in metrics.py:60-62
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
#pragma unroll
      for (int q = 0; q < kQ; ++q) {
        const double up = __shfl_up(v[q], o);
        if (lane >= o) v[q] += up;
      }
    }
#pragma unroll
    for (int q = 0; q < kQ; ++q) {
      v[q] += carry[q];
      if (c < W) base[q * plane + c + 1] = v[q];
      carry[q] = __shfl(v[q], 63);
    }
  }
}

// Column pass, in two launches so that a 1024-row table is not one thread's 1024 dependent steps: (1) every 32-row
// segment of a column is summed down in place (its last row = the segment's total, also copied to `segtot`); (2) each
// segment adds the totals of the segments above it.  Threads of a wave are consecutive columns: coalesced rows.
constexpr int kSeg = 32;
__global__ void sat_cols_local_kernel(double* __restrict__ sat, double* __restrict__ segtot, int n_planes, int H, int W, int nseg) {
  const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  const size_t per = (size_t)(W + 1);
  if (t >= (size_t)n_planes * nseg * per) return;
  const int col = (int)(t % per);
  const int seg = (int)((t / per) % nseg);
  const int pl = (int)(t / (per * nseg));
  double* p = sat + (size_t)pl * (H + 1) * per + col;
  const int r0 = seg * kSeg + 1, r1 = min(H, r0 + kSeg - 1);
  double acc = 0.0;
  for (int r = r0; r <= r1; ++r) {
    acc += p[(size_t)r * per];
    p[(size_t)r * per] = acc;
  }
  segtot[((size_t)pl * nseg + seg) * per + col] = acc;
}
__global__ void sat_cols_carry_kernel(double* __restrict__ sat, const double* __restrict__ segtot, int n_planes, int H, int W, int nseg) {
  const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  const size_t per = (size_t)(W + 1);
  if (t >= (size_t)n_planes * (nseg - 1) * per) return;
  const int col = (int)(t % per);
  const int seg = (int)((t / per) % (nseg - 1)) + 1;
  const int pl = (int)(t / (per * (nseg - 1)));
  double carry = 0.0;
  for (int s = 0; s < seg; ++s) carry += segtot[((size_t)pl * nseg + s) * per + col];
  double* p = sat + (size_t)pl * (H + 1) * per + col;
  const int r0 = seg * kSeg + 1, r1 = min(H, r0 + kSeg - 1);
  for (int r = r0; r <= r1; ++r) p[(size_t)r * per] += carry;
}

// The SSIM map value of a pixel from its five window sums and 1 / ws^2, in fp32 in the reference's operation order
// (metrics.py:58-66), for the three sweep kernels and the SSIM maps.
__device__ __forceinline__ float ssim_of_sums(const double (&sum)[kQ], double dinv) {
#pragma clang fp contract(off)     // the reference's rounding: an fma leaves E[x^2] - mu^2 a residue where it is 0
  const float C1 = (float)(0.01 * 0.01), C2 = (float)(0.03 * 0.03);
  const float mu1 = (float)(sum[0] * dinv), mu2 = (float)(sum[1] * dinv);
  const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
  const float s1 = (float)(sum[2] * dinv) - mu1_sq;
  const float s2 = (float)(sum[3] * dinv) - mu2_sq;
  const float s12 = (float)(sum[4] * dinv) - mu12;
  return ((2.0f * mu12 + C1) * (2.0f * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2));
}

// Reflect-padded window along one axis as table differences.  Padded coordinates lo..hi (each side leaves [0, n-1] by less
// than n) cover the real indices [max(lo,0), min(hi,n-1)] once, [1, -lo] once more if lo < 0, and [2(n-1)-hi, n-2] once more if
// hi > n-1 (numpy "reflect": the edge sample is not repeated).  With P the prefix table (P[0] = 0) the covered sum is three
// (+, -) pairs of table entries; a pair that is not needed has both indices equal and cancels.
__device__ __forceinline__ void axis_pairs(int lo, int hi, int n, int (&idx)[6]) {
  idx[0] = min(hi, n - 1) + 1; idx[1] = max(lo, 0);                       // + P[idx0] - P[idx1]: the part inside the image
  idx[2] = lo < 0 ? -lo + 1 : 1; idx[3] = 1;                              // + P[-lo + 1] - P[1]: reflected over the low edge
  idx[4] = n - 1; idx[5] = hi > n - 1 ? 2 * (n - 1) - hi : n - 1;         // + P[n - 1] - P[2 (n - 1) - hi]: over the high edge
}

// The window sums of pixel (i, j) for window size ws, from the Q tables S of its image (planes of (H + 1) x (W + 1)), handed to
// `finish`: the sums are the (row pair, column pair) rectangles of axis_pairs.  The reflection pairs of either axis are skipped by
// wave-uniform branches when no lane of the wave needs them, and all loads of a rectangle are issued before the first add.  (The
// sums stay in this function: handed out through an array parameter they cost the SSIM map kernel 6 VGPRs.)
template <int Q, class Finish>
__device__ __forceinline__ auto corner_window(const double* S, int H, int W, int i, int j, int ws, Finish finish) {
  const int pad = ws / 2, iper = W + 1;
  const size_t plane = (size_t)(H + 1) * iper;
  int ri[6], ci[6];
  axis_pairs(i - pad, i + ws - 1 - pad, H, ri);
  axis_pairs(j - pad, j + ws - 1 - pad, W, ci);
  // does any lane of the wave need the reflection pairs?  (a wave-uniform i: the row answers are scalar anyway)
  const bool row_lo = __builtin_amdgcn_ballot_w64(i - pad < 0) != 0, row_hi = __builtin_amdgcn_ballot_w64(i + ws - 1 - pad > H - 1) != 0;
  const bool col_lo = __builtin_amdgcn_ballot_w64(j - pad < 0) != 0, col_hi = __builtin_amdgcn_ballot_w64(j + ws - 1 - pad > W - 1) != 0;
  double sum[Q] = {};
  auto row_pair = [&](auto RP) __attribute__((always_inline)) {               // + row ri[2 rp], - row ri[2 rp + 1]
    constexpr int rp = decltype(RP)::value;
    const int oa = ri[2 * rp] * iper, ob = ri[2 * rp + 1] * iper;
    auto col_pair = [&](auto CP) __attribute__((always_inline)) {
      constexpr int cp = decltype(CP)::value;
      double va[Q], vb[Q], vc[Q], vd[Q];
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const double* Sq = S + (size_t)q * plane;
        va[q] = Sq[oa + ci[2 * cp]]; vb[q] = Sq[oa + ci[2 * cp + 1]];
        vc[q] = Sq[ob + ci[2 * cp]]; vd[q] = Sq[ob + ci[2 * cp + 1]];
      }
#pragma unroll
      for (int q = 0; q < Q; ++q) sum[q] += (va[q] - vb[q]) - (vc[q] - vd[q]);
    };
    col_pair(std::integral_constant<int, 0>{});
    if (col_lo) col_pair(std::integral_constant<int, 1>{});
    if (col_hi) col_pair(std::integral_constant<int, 2>{});
  };
  row_pair(std::integral_constant<int, 0>{});
  if (row_lo) row_pair(std::integral_constant<int, 1>{});
  if (row_hi) row_pair(std::integral_constant<int, 2>{});
  return finish(sum);
}
// The SSIM map value of pixel (i, j) for window size ws: the five window sums through ssim_of_sums.
__device__ __forceinline__ float corner_ssim(const double* S, int H, int W, int i, int j, int ws, double dinv) {
  return corner_window<kQ>(S, H, W, i, j, ws, [&](const double (&sum)[kQ]) __attribute__((always_inline)) { return ssim_of_sums(sum, dinv); });
}
// The squared-error window sum of pixel (i, j): one table of integers below 2^53, so every difference and the sum are exact.
__device__ __forceinline__ double corner_sqerr(const double* S, int H, int W, int i, int j, int ws) {
  return corner_window<1>(S, H, W, i, j, ws, [](const double (&sum)[1]) __attribute__((always_inline)) { return sum[0]; });
}

// Evaluation: one workgroup = kEvalPix consecutive pixels of one image for ONE window size; up to kWsGroup window sizes share
// a launch (the list travels as a kernel argument; an image's window sizes run back to back).  SSIM map values summed per
// block (float64, fixed order).  A pixel row i with pad p = ws / 2 reads table rows i - p and i + p + 1 (plus the reflected ones
// near the borders): 80 B per pixel and window size, each table row exactly twice per window size.
//
// ROWS = the image width is a multiple of 64 (every MVTec size): a wave's 64 pixels are consecutive pixels of ONE row, so the row
// pairs are wave-uniform (scalar row offsets) and the reflection pairs of both axes are skipped by wave-uniform branches when no
// lane needs them; all loads of a (row pair, column pair) are issued before the first add.  Otherwise every lane works out its
// own pixel (any width).  Same arithmetic either way.
// (Tried: XCD k owns a strip of pixel blocks and window size k works p_k rows further down, so that all window sizes of a
// launch share their top table row in one L2 - 5.0 -> 5.8 ms at 1024 px: the sweep is not bound by the fabric side.)
constexpr int kWsGroup = 16;
struct WsList { int ws[kWsGroup]; double dinv[kWsGroup]; };    // window sizes of a launch and 1 / ws^2 (a float64 division per pixel otherwise)

// Sum of the 64 SSIM map values of a wave's segment, in every lane.  The values are float32 in [-1, 1]; each is first rounded
// to a multiple of 2^-24 (an error of up to 2^-25 per pixel, so this kernel's mean can differ from the corner kernel's in the
// last bits), then the integers are summed exactly, so the order is irrelevant and DPP lane swizzles can do four of the six
// steps (a float64 shuffle chain was 12 ds_bpermute round trips + 30 vector instructions per 64 pixels of a kernel that is
// VALU-bound).
__device__ __forceinline__ double wave_sum_map(float m) {
  int v = __float2int_rn(m * 16777216.0f);
  v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, true);
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return (double)v * (1.0 / 16777216.0);
}
template <bool ROWS>
__global__ __launch_bounds__(256) void ssim_eval_kernel(const double* __restrict__ sat, double* __restrict__ partial,
                                                        int H, int W, const WsList wl, int nblk, int g, int n_img) {
  const int L = blockIdx.x, per_img = nblk * g;
  const int img = L / per_img, r0 = L - img * per_img;
  const int kw = r0 / nblk, pb = r0 - kw * nblk;
  const int ws = wl.ws[kw];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const size_t plane = (size_t)(H + 1) * (W + 1);
  const double* const S = sat + (size_t)img * kQ * plane;
  const double dinv = wl.dinv[kw];
  const int npix = H * W;
  double local = 0.0;
#pragma unroll 1
  for (int it = 0; it < kEvalPix / 256; ++it) {
    const int seg0 = pb * kEvalPix + (wave * (kEvalPix / 256) + it) * 64;    // first pixel of this wave's 64 (wave-uniform)
    if (seg0 >= npix) break;
    int i, j;
    if constexpr (ROWS) { i = seg0 / W; j = seg0 - i * W + lane; }           // i scalar
    else { const int pix = min(seg0 + lane, npix - 1); i = pix / W; j = pix - i * W; }
    const float m = corner_ssim(S, H, W, i, j, ws, dinv);
    if (ROWS || seg0 + lane < npix) local += (double)m;
  }
  __shared__ double red[256];
  const double s = srad_block_sum(local, red);
  if (threadIdx.x == 0) partial[((size_t)img * kWsGroup + kw) * nblk + pb] = s;
}

// ------------------------------------------------------------------------------------------------------------------------
// The sweep for the image widths MVTec runs at (64 / 128 / 256 / 512 / 1024: a power of two that divides 1024): table rows
// through LDS.
//
// Along the rows a reflect-padded window lo..hi is  B(hi) - T(lo)  with
//     T(lo) = P[max(lo, 0)] - (lo < 0 ? P[1 - lo] - P[1] : 0)          B(hi) = P[min(hi, H-1) + 1] + (hi > H-1 ? P[H-1] - P[2(H-1) - hi] : 0)
// (P[r] = table row r, all W + 1 columns of all five quantities).  T depends on the window's first row only, and pixel row i with
// pad p has lo = i - p: for a fixed lo = t EVERY window size of the launch meets the same T(t), at pixel row i = t + p_k.  So a
// 1024-thread workgroup owns 1024 / W consecutive values of t (1024 pixels per window size), keeps its T rows in registers, and
// for each window size of the group streams the B rows once, coalesced, writes D = B - T (the row-summed window: W + 1 prefix
// values per quantity and row) to LDS and evaluates its 1024 pixels from there - column pairs of D instead of 4 - 36 table
// corners per quantity - while the next window size's B rows are in flight in registers (two LDS images, one barrier per
// window size).
//
// The corner kernel above is bound by vector instructions and 8-byte loads (~45 per pixel and window size with the reflection
// pairs of the big windows: 4.5 ms for 2 pairs x 102 window sizes at 1024 px), so this one is built to issue few of either: a
// thread's row elements are (quantity q, row r = tid / W, column tid % W) for q = 0 .. 4 - the same table column for every
// quantity; the quantity's plane and the row (wave-uniform: W >= 64) are the SCALAR offset of a buffer load, ~6 loads and no
// address arithmetic per pixel and window size - plus column W of every (q, r) on the first 5 * 1024 / W threads; 1 / ws^2
// comes from the host; the 64 map values of a wave are summed as integers through DPP.  2.06 ms (1024 px) / 0.38 ms (78 pairs at
// 128 px, with the first, per-element form of this kernel).  What is left is a balance of LDS bytes (40 B per column term), the
// B rows' 8-byte loads and ~120 vector instructions per pixel; the order in which workgroups take the rows (XCD strips, rows
// shared between window sizes kept in one L2) changed nothing: the tables are served by the Infinity Cache fast enough.
typedef __attribute__((ext_vector_type(2))) unsigned int sc_u32x2;
__global__ __launch_bounds__(1024) void ssim_rows_lds_kernel(const double* __restrict__ sat, double* __restrict__ partial,
                                                             int H, int lw, const WsList wl, int g, int t_first, int nt_blocks) {
  const int W = 1 << lw, iper = W + 1, rb = 1024 >> lw, rowq = rb * iper, n_el = kQ * rowq;
  extern __shared__ __attribute__((aligned(16))) double Dl[];              // two images of [kQ][rb][W + 1], then [2][16] wave sums
  double* const wsum = Dl + 2 * n_el;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int img = blockIdx.x / nt_blocks, t0 = t_first + (blockIdx.x - img * nt_blocks) * rb;
  const size_t plane = (size_t)(H + 1) * iper;
  const double* const S = sat + (size_t)img * kQ * plane;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(S), 0, (int)(kQ * plane * 8), 0x00020000);
  auto ld = [&](int voff, size_t soff_el) __attribute__((always_inline)) -> double {     // table entry at voff bytes + soff_el elements
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rs, voff, (int)(soff_el * 8), 0));
  };
  const int r = __builtin_amdgcn_readfirstlane((wave * 64) >> lw);         // this wave's row of the workgroup's rb (scalar)
  const int c = tid & (W - 1);
  const int t = t0 + r;
  const int v_main = c * 8;
  // column W of (quantity q, row rr) on thread q * rb + rr: per-lane rows, so the row offset is part of the vector offset
  const bool tail = tid < kQ * rb;
  const int tq = tail ? tid / rb : 0, trr = tail ? tid - tq * rb : 0;
  const bool tail_wave = wave * 64 < kQ * rb;                              // scalar
  auto tail_off = [&](int row) __attribute__((always_inline)) { return (int)((tq * plane + (size_t)row * iper + W) * 8); };
  // T(t) = P[max(t, 0)] - (t < 0 ? P[1 - t] - P[1] : 0): unconditional loads, the pair cancels for t >= 0 (row 0 = zeros)
  double Tv[kQ], Tt = 0.0;
  {
    const int ta = min(max(t, 0), H), tx = t < 0 ? min(1 - t, H) : 1;
#pragma unroll
    for (int q = 0; q < kQ; ++q) Tv[q] = ld(v_main, q * plane + (size_t)ta * iper) - (ld(v_main, q * plane + (size_t)tx * iper) - ld(v_main, q * plane + iper));
    if (tail_wave) {
      const int tt = t0 + trr, tta = min(max(tt, 0), H), ttx = tt < 0 ? min(1 - tt, H) : 1;
      Tt = ld(tail_off(tta), 0) - (ld(tail_off(ttx), 0) - ld(tail_off(1), 0));
    }
  }
  double b0[kQ], bx[kQ], b0t = 0.0, bxt = 0.0;
  auto load_b = [&](int kw) __attribute__((always_inline)) {
    const int ws = wl.ws[kw], pad = ws / 2;
    const int i = t + pad, hi = i + ws - 1 - pad;                           // scalar
    const int rmain = min(max(hi, 0), H - 1) + 1;
    if (hi > H - 1 && i < H) {                                             // scalar branch around straight-line loads
      const int ry = 2 * (H - 1) - hi;
#pragma unroll
      for (int q = 0; q < kQ; ++q) {
        b0[q] = ld(v_main, q * plane + (size_t)rmain * iper);
        bx[q] = ld(v_main, q * plane + (size_t)(H - 1) * iper) - ld(v_main, q * plane + (size_t)ry * iper);
      }
    } else {
#pragma unroll
      for (int q = 0; q < kQ; ++q) { b0[q] = ld(v_main, q * plane + (size_t)rmain * iper); bx[q] = 0.0; }
    }
    if (tail_wave) {                                                       // per-lane rows: unconditional loads, the pair cancels where not needed
      const int ti = t0 + trr + pad, thi = ti + ws - 1 - pad;
      const bool over = thi > H - 1 && ti < H;
      b0t = ld(tail_off(min(max(thi, 0), H - 1) + 1), 0);
      bxt = ld(tail_off(H - 1), 0) - ld(tail_off(over ? 2 * (H - 1) - thi : H - 1), 0);
    }
  };
  load_b(0);
  for (int kw = 0; kw < g; ++kw) {
    const int ws = wl.ws[kw], pad = ws / 2;
    const int i = t + pad;                                                 // scalar: this wave's pixel row for this window size
    const bool row_ok = i >= 0 && i < H;
    const double dinv = wl.dinv[kw];
    double* const Dk = Dl + (kw & 1) * n_el;
    {
      double* const Dw = Dk + r * iper + c;
#pragma unroll
      for (int q = 0; q < kQ; ++q) Dw[q * rowq] = (b0[q] + bx[q]) - Tv[q];   // (rows that do not exist for this window size are never read)
      if (tail) Dk[tq * rowq + trr * iper + W] = (b0t + bxt) - Tt;
    }
    __syncthreads();
    // the previous window size's 16 wave sums -> one partial per (window size, pixel row): thread 0 of each row's first wave
    if (kw > 0 && (tid & (W - 1)) == 0) {
      const int ip = t + wl.ws[kw - 1] / 2;
      if (ip >= 0 && ip < H) {
        const double* w0 = wsum + ((kw - 1) & 1) * 16 + wave;
        double acc = 0.0;
        for (int k = 0; k < (W >> 6); ++k) acc += w0[k];
        partial[((size_t)img * kWsGroup + kw - 1) * H + ip] = acc;
      }
    }
    if (kw + 1 < g) load_b(kw + 1);
    float m_val = 0.f;
    if (row_ok) {
      const int lo = c - pad, hi = c + ws - 1 - pad;
      const double* const Dr = Dk + r * iper;
      const int c1 = min(hi, W - 1) + 1, c0 = max(lo, 0);
      double sum[kQ];
#pragma unroll
      for (int q = 0; q < kQ; ++q) sum[q] = Dr[q * rowq + c1] - Dr[q * rowq + c0];
      if (__builtin_amdgcn_ballot_w64(lo < 0) != 0) {
        const int ca = lo < 0 ? 1 - lo : 1;
#pragma unroll
        for (int q = 0; q < kQ; ++q) sum[q] += Dr[q * rowq + ca] - Dr[q * rowq + 1];
      }
      if (__builtin_amdgcn_ballot_w64(hi > W - 1) != 0) {
        const int cb = hi > W - 1 ? 2 * (W - 1) - hi : W - 1;
#pragma unroll
        for (int q = 0; q < kQ; ++q) sum[q] += Dr[q * rowq + W - 1] - Dr[q * rowq + cb];
      }
      m_val = ssim_of_sums(sum, dinv);
    }
    const double seg = wave_sum_map(m_val);
    if (lane == 0) wsum[(kw & 1) * 16 + wave] = seg;
  }
  __syncthreads();
  if ((tid & (W - 1)) == 0) {
    const int ip = t + wl.ws[g - 1] / 2;
    if (ip >= 0 && ip < H) {
      const double* w0 = wsum + ((g - 1) & 1) * 16 + wave;
      double acc = 0.0;
      for (int k = 0; k < (W >> 6); ++k) acc += w0[k];
      partial[((size_t)img * kWsGroup + g - 1) * H + ip] = acc;
    }
  }
}

// one workgroup per (image, window size of the group): thread i sums every 256th partial, then a fixed-order block sum
__global__ __launch_bounds__(256) void ssim_finish_kernel(const double* __restrict__ partial, double* __restrict__ out, int n_img, int n_grp,
                                                          int nblk, int out_stride, int out_col0, double inv_count) {
  const int img = blockIdx.x / n_grp, kw = blockIdx.x - img * n_grp;
  const double* p = partial + ((size_t)img * kWsGroup + kw) * nblk;
  double s = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 256) s += p[b];
  __shared__ double red[256];
  const double total = srad_block_sum(s, red);
  if (threadIdx.x == 0) out[(size_t)img * out_stride + out_col0 + kw] = total * inv_count;
}

// ------------------------------------------------------------------------------------------------------------------------
// Per-pixel maps: one fp32 value per pixel and window size from an image's float64 tables, reduced over the `g` window sizes of
// `wl` to ONE value per pixel without a map per size in memory.  What a value is made of is the map's source, a trait struct
// (SsimSrc and SqerrSrc, with their host sides, below): `planes` tables per image, and value(S, H, W, i, j, ws, factor) = the map
// value of pixel (i, j) at window size ws, with `factor` the size's host-computed double (WsList::dinv).  Either source reads its
// window through corner_window: the reflection pairs of either axis are skipped by wave-uniform branches when no lane needs them.

// The pixel of a map kernel's thread (blocks of 256 pixels, `pb` = the block within the image): p = its index, which the caller
// compares with npix before it stores, and (i, j) = the pixel it computes.
// ROWS = the width is a multiple of 64: a wave's 64 pixels lie in one row, the row index is scalar (as in ssim_eval_kernel).
template <bool ROWS>
__device__ __forceinline__ void map_pixel(int pb, int npix, int W, int& p, int& i, int& j) {
  p = pb * 256 + (int)threadIdx.x;
  if constexpr (ROWS) {
    // npix is a multiple of 64 too; a wave past the end (the last block's) computes a copy of the last 64 pixels
    const int seg0 = min(__builtin_amdgcn_readfirstlane(pb * 256 + ((int)threadIdx.x & ~63)), npix - 64);
    i = seg0 / W; j = seg0 - i * W + ((int)threadIdx.x & 63);
  } else {
    const int pix = min(p, npix - 1);                                    // lanes past the end compute a copy of the last pixel
    i = pix / W; j = pix - i * W;
  }
}
// A pixel's thread walks the list in order and keeps one fp32 accumulator:
//   mean: a_1 = v_1, a_k = a_(k-1) + v_k, out = a_K * scale      max: a_k = fmaxf(a_(k-1), v_k)
// - single IEEE fp32 operations in list order, so the result is the bits of the K single maps accumulated the same way.  Lists
// longer than kWsGroup take several launches: `first` = 0 continues from the accumulator the launch before stored in `out`
// (same thread, same pixel, stream order), and only the last launch of a mean gets scale = (float)(1 / K) (1 otherwise; a
// multiply by a host-computed factor, not a division).  The map of ONE size is g = 1, first = 1, scale = 1: v_1 * 1.0f.  The
// loop over the sizes stays a loop: unrolled over the runtime count it would hold several sizes' index sets in registers.
// ONE = the list has one size: v_1 is stored as it is, without the loop and the read-back (the same bits).  The squared-error
// maps take it, their value being so little work that the loop's bookkeeping shows: at 8 x 1024 px and ws 11 a call takes 0.106 ms
// with it and 0.112 ms without; the SSIM maps of one size are as fast through the loop.
template <class Src, bool ROWS, bool ONE = false>
__global__ __launch_bounds__(256) void window_map_kernel(const double* __restrict__ sat, float* __restrict__ out, int H, int W,
                                                         const WsList wl, int g, int reduce_max, int first, float scale, int nblk) {
#pragma clang fp contract(off)
  const int img = blockIdx.x / nblk, pb = blockIdx.x - img * nblk;
  const int npix = H * W;
  int p, i, j;
  map_pixel<ROWS>(pb, npix, W, p, i, j);
  const double* const S = sat + (size_t)img * Src::planes * ((size_t)(H + 1) * (W + 1));
  float* const dst = out + (size_t)img * npix + p;
  if constexpr (ONE) {
    const float v = Src::value(S, H, W, i, j, wl.ws[0], wl.dinv[0]);
    if (p < npix) *dst = v;
    return;
  }
  float acc = 0.0f;
  if (!first && p < npix) acc = *dst;
#pragma unroll 1
  for (int k = 0; k < g; ++k) {
    const float v = Src::value(S, H, W, i, j, wl.ws[k], wl.dinv[k]);
    if (first && k == 0) acc = v;
    else acc = reduce_max ? fmaxf(acc, v) : acc + v;
  }
  if (p < npix) *dst = acc * scale;
}

// ------------------------------------------------------------------------------------------------------------------------
// Squared-error maps (DESIGN.md "Squared-error maps"; the per-pixel form of the MSE score of src/evaluate.py:251-265).  On u8
// images e[i, j] = sum_c (sr - hr)^2 is an integer, so its sum S over the reflect-padded window of corner_ssim is one too, and
// the map is (float)((double)S * inv) with inv = 1 / (C ws^2 65025) from the host: defined bit for bit.
//
// ONE prefix plane of e per image, float64 in the table layout above (every prefix is below (H + 1)(W + 1) * 3 * 65025 < 2^49, so
// float64 is exact), built by the row pass below and the column pass of the SSIM tables; the map kernels read it through
// corner_window<1>.  Per pixel: 8 B of table written by the row pass plus the column pass's 16 to 32 B, 8 B (no reflection) to
// 72 B (both axes reflect on both sides) of corners per window size, and the 4 B store - the SSIM maps cost 200 B of table and
// 80 B per size.
//
// Row pass: one wave per (image, table row), as sat_rows_kernel; a 64-pixel chunk is scanned in u32 (64 * 3 * 65025 < 2^24).
__global__ __launch_bounds__(256) void sqerr_rows_kernel(const uint8_t* __restrict__ sr, const uint8_t* __restrict__ hr,
                                                         double* __restrict__ sat, int n_img, int H, int W, int C) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= n_img * (H + 1)) return;
  const int img = t / (H + 1), r = t - img * (H + 1);
  double* const base = sat + ((size_t)img * (H + 1) + r) * (W + 1);
  if (r == 0) {
    for (int c = lane; c <= W; c += 64) base[c] = 0.0;
    return;
  }
  if (lane == 0) base[0] = 0.0;
  const uint8_t* ps = sr + ((size_t)img * H + (r - 1)) * W * C;
  const uint8_t* ph = hr + ((size_t)img * H + (r - 1)) * W * C;
  double carry = 0.0;
  for (int c0 = 0; c0 < W; c0 += 64) {
    const int c = c0 + lane;
    unsigned v = 0;
    if (c < W)
      for (int ch = 0; ch < C; ++ch) {
        const int d = (int)ps[(size_t)c * C + ch] - (int)ph[(size_t)c * C + ch];
        v += (unsigned)(d * d);
      }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned up = __shfl_up(v, o);
      if (lane >= o) v += up;
    }
    const double s = carry + (double)v;
    if (c < W) base[c + 1] = s;
    carry = __shfl(s, 63);
  }
}

// ws = 1 alone needs no table: out = (float)((double)e * inv) straight from the two stacks, 2 C bytes read and 4 B written per
// pixel.  A thread takes 4 consecutive pixels of the flattened stacks: with `vec` (sr and hr 4-byte aligned, out 16-byte
// aligned) their 4 C bytes are C dwords per stack and the four values one 16-byte store; the pixels of a last, partial group
// and unaligned stacks go byte by byte.
template <int C>
__global__ __launch_bounds__(256) void sqerr_pixel_kernel(const uint8_t* __restrict__ sr, const uint8_t* __restrict__ hr,
                                                          float* __restrict__ out, size_t npix, double inv, int vec) {
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x, p0 = q * 4;
  if (p0 >= npix) return;
  if (vec && p0 + 4 <= npix) {
    uint32_t a[C], b[C];
#pragma unroll
    for (int w = 0; w < C; ++w) {
      a[w] = reinterpret_cast<const uint32_t*>(sr)[q * C + w];
      b[w] = reinterpret_cast<const uint32_t*>(hr)[q * C + w];
    }
    unsigned e[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4 * C; ++k) {                                    // byte k of the group belongs to pixel k / C
      const int d = (int)((a[k / 4] >> (8 * (k % 4))) & 255u) - (int)((b[k / 4] >> (8 * (k % 4))) & 255u);
      e[k / C] += (unsigned)(d * d);
    }
    float4 o;
    o.x = (float)((double)e[0] * inv); o.y = (float)((double)e[1] * inv);
    o.z = (float)((double)e[2] * inv); o.w = (float)((double)e[3] * inv);
    reinterpret_cast<float4*>(out)[q] = o;
    return;
  }
  for (size_t p = p0; p < npix && p < p0 + 4; ++p) {
    unsigned e = 0;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
      const int d = (int)sr[p * C + ch] - (int)hr[p * C + ch];
      e += (unsigned)(d * d);
    }
    out[p] = (float)((double)e * inv);
  }
}

// mean((sr/255 - hr/255)^2) over all H*W*C values of an image: block partial sums (grid = blocks x images) ...
__global__ __launch_bounds__(256) void mse_partial_kernel(const uint8_t* __restrict__ sr, const uint8_t* __restrict__ hr,
                                                          double* __restrict__ partial, size_t n, int nb) {
  const int img = blockIdx.y;
  const uint8_t* a = sr + (size_t)img * n;
  const uint8_t* b = hr + (size_t)img * n;
  double local = 0.0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)nb * 256) {
    const float d = (float)a[i] / 255.0f - (float)b[i] / 255.0f;
    local += (double)(d * d);
  }
  __shared__ double red[256];
  const double s = srad_block_sum(local, red);
  if (threadIdx.x == 0) partial[(size_t)img * nb + blockIdx.x] = s;
}
// ... and one thread per image: the mean as float32 (np.mean of a float32 array), PSNR with data_range 1
__global__ void mse_finish_kernel(const double* __restrict__ partial, double* __restrict__ mse, double* __restrict__ psnr, int n_img,
                                  int nb, double n) {
  const int img = blockIdx.x * blockDim.x + threadIdx.x;
  if (img >= n_img) return;
  double s = 0.0;
  for (int b = 0; b < nb; ++b) s += partial[(size_t)img * nb + b];
  const double m = (double)(float)(s / n);
  mse[img] = m;
  psnr[img] = m == 0.0 ? INFINITY : 10.0 * log10(1.0 / m);
}

__global__ void to_u8_hwc_kernel(const float* __restrict__ x, uint8_t* __restrict__ out, int B, int C, int HW, float mul) {
  const size_t total = (size_t)B * C * HW;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const size_t pix = i / C;
    const int b = (int)(pix / HW);
    const int hw = (int)(pix - (size_t)b * HW);
    float v = x[((size_t)b * C + c) * HW + hw] * mul;
    v = fminf(fmaxf(v, 0.0f), 255.0f);            // clamp(0, 255); NaN -> 0 like torch's clamp+byte on ROCm is undefined
    out[i] = (uint8_t)v;                           // .byte(): truncation toward zero (evaluate.py:214-215)
  }
}

__global__ void quantize_kernel(const float* __restrict__ x, float* __restrict__ y, size_t n, float pr) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float v = fminf(fmaxf(x[i] * pr, 0.0f), 255.0f);
    y[i] = rintf(v) / pr;                          // torch.round = half to even (trainer.py:45-47)
  }
}

// Validation metrics of Trainer.test (metrics.py:70-108): one workgroup per image.
__global__ __launch_bounds__(256) void val_metrics_kernel(const float* __restrict__ sr, const float* __restrict__ hr, int C,
                                                          int H, int W, float rgb_range, double* __restrict__ psnr,
                                                          double* __restrict__ ssim) {
  const int img = blockIdx.x;
  const size_t plane = (size_t)H * W;
  const float* s = sr + (size_t)img * C * plane;
  const float* h = hr + (size_t)img * C * plane;
  const int shave = 4;
  const bool do_shave = W > 2 * shave;                        // "if sr.size(-1) > 2 * shave"
  const int y0 = do_shave ? shave : 0, y1 = do_shave ? H - shave : H;
  const int x0 = do_shave ? shave : 0, x1 = do_shave ? W - shave : W;
  const int h2 = y1 - y0, w2 = x1 - x0;
  __shared__ double red[256];
  // ---- PSNR: diff = (sr - hr) / range over all channels of the shaved region ----
  double local = 0.0;
  for (int c = 0; c < C; ++c)
    for (int p = threadIdx.x; p < h2 * w2; p += 256) {
      const int yy = y0 + p / w2, xx = x0 + p % w2;
      const float d = (s[c * plane + (size_t)yy * W + xx] - h[c * plane + (size_t)yy * W + xx]) / rgb_range;
      local += (double)(d * d);
    }
  const double sq = srad_block_sum(local, red);
  if (threadIdx.x == 0) {
    const double m = (double)(float)(sq / ((double)C * h2 * w2));
    psnr[img] = m == 0.0 ? INFINITY : 10.0 * log10(1.0 / m);
  }
  __syncthreads();                                            // every thread has read red[0] before the second sum writes red
  // ---- SSIM: clamp(x/range, 0, 1), luminance if C > 1, 11x11 box with ZERO padding, C1/C2 * 255^2 ----
  auto lum = [&](const float* t, int yy, int xx) -> float {
    if (yy < y0 || yy >= y1 || xx < x0 || xx >= x1) return 0.0f;           // zero padding of the shaved image
    if (C == 1) return fminf(fmaxf(t[(size_t)yy * W + xx] / rgb_range, 0.0f), 1.0f);
    const float cv[3] = {65.738f / 256.0f, 129.057f / 256.0f, 25.064f / 256.0f};
    float acc = 0.0f;
    for (int c = 0; c < 3; ++c) acc += fminf(fmaxf(t[c * plane + (size_t)yy * W + xx] / rgb_range, 0.0f), 1.0f) * cv[c];
    return acc;
  };
  const float C1 = (float)(0.01 * 0.01 * 255.0 * 255.0), C2 = (float)(0.03 * 0.03 * 255.0 * 255.0);
  const int win = 11, pad = 5;
  local = 0.0;
  for (int p = threadIdx.x; p < h2 * w2; p += 256) {
    const int yy = y0 + p / w2, xx = x0 + p % w2;
    double a1 = 0, a2 = 0, a11 = 0, a22 = 0, a12 = 0;
    for (int dy = -pad; dy <= pad; ++dy)
      for (int dx = -pad; dx <= pad; ++dx) {
        const float u = lum(s, yy + dy, xx + dx), v = lum(h, yy + dy, xx + dx);
        a1 += u; a2 += v; a11 += (double)(u * u); a22 += (double)(v * v); a12 += (double)(u * v);
      }
    const double k = 1.0 / (win * win);
    const float mu1 = (float)(a1 * k), mu2 = (float)(a2 * k);
    const float s1 = (float)(a11 * k) - mu1 * mu1, s2 = (float)(a22 * k) - mu2 * mu2, s12 = (float)(a12 * k) - mu1 * mu2;
    const float m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2));
    local += (double)m;
  }
  const double ss = srad_block_sum(local, red);
  if (threadIdx.x == 0) ssim[img] = ss / ((double)h2 * w2);
}

int chunk_images(int n_img, int H, int W) {
  const size_t per = (size_t)(H + 1) * (W + 1);
  const size_t cap = (size_t)1 << 25;                  // table points per chunk (x 40 bytes)
  size_t c = cap / per;
  if (c < 1) c = 1;
  return (int)std::min<size_t>(c, (size_t)n_img);
}
// widths the LDS-staged sweep takes (ssim_rows_lds_kernel), and the partial sums per (image, window size) either kernel writes
inline bool lds_sweep_ok(int H, int W) {
  return W >= 64 && W <= 1024 && (W & (W - 1)) == 0 && (long long)kQ * (H + 1) * (W + 1) * 8 < (1ll << 31);
}
inline int partial_slots(int H, int W) { return lds_sweep_ok(H, W) ? H : (H * W + kEvalPix - 1) / kEvalPix; }
// the evaluation kernel of the sweep (srad_score_plan's numbering): the LDS sweep, the corner kernel with per-row waves, any width
enum SweepKernel { kSweepLds = 0, kSweepRows = 1, kSweepAny = 2 };
inline SweepKernel sweep_kernel(int H, int W) { return lds_sweep_ok(H, W) ? kSweepLds : W % 64 == 0 ? kSweepRows : kSweepAny; }
inline int grid1d(size_t total) {
  size_t b = (total + 255) / 256;
  return (int)std::min<size_t>(std::max<size_t>(b, 1), 4096);
}

// Workspace of srad_score_pairs (sweep) and srad_anomaly_maps for n_img H x W pairs, each part 256-byte aligned: the tables of
// one chunk of images (`planes` per image: the five of SSIM, or the one of the squared-error maps), the sweep's partial sums
// (sweep only) and the column pass's segment totals.  base == nullptr: sizes only.
struct ScoreWs {
  int chunk, nseg, nblk;          // images per chunk, 32-row segments per table column, partial slots per (image, window size)
  double *sat, *partial, *segtot;
  size_t bytes;
};
ScoreWs plan_score_ws(int n_img, int H, int W, bool sweep, void* base, int planes = kQ) {
  ScoreWs w;
  w.chunk = chunk_images(n_img, H, W);
  w.nseg = (H + kSeg - 1) / kSeg;
  w.nblk = partial_slots(H, W);
  Bump bp(base, 0);
  auto take = [&](size_t doubles) { return reinterpret_cast<double*>(bp.take(2 * doubles)); };    // Bump counts floats
  w.sat = take((size_t)w.chunk * (H + 1) * (W + 1) * planes);
  w.partial = sweep ? take((size_t)w.chunk * kWsGroup * w.nblk) : nullptr;
  w.segtot = take((size_t)w.chunk * planes * w.nseg * (W + 1));
  w.bytes = bp.used;
  return w;
}

// The column pass over `n_planes` row-summed planes, in 32-row segments.
void column_pass(const ScoreWs& w, int n_planes, int H, int W, hipStream_t s) {
  const size_t t = (size_t)n_planes * w.nseg * (W + 1);
  SradProfScope prof(s, SRAD_K_SCORE, 1.0 * n_planes * (H + 1) * (W + 1), 16.0 * n_planes * (H + 1) * (W + 1));
  hipLaunchKernelGGL(sat_cols_local_kernel, dim3((unsigned)((t + 255) / 256)), dim3(256), 0, s, w.sat, w.segtot, n_planes, H, W, w.nseg);
  if (w.nseg > 1) {
    const size_t t2 = (size_t)n_planes * (w.nseg - 1) * (W + 1);
    hipLaunchKernelGGL(sat_cols_carry_kernel, dim3((unsigned)((t2 + 255) / 256)), dim3(256), 0, s, w.sat, w.segtot, n_planes, H, W, w.nseg);
  }
}

// The five tables of n pairs (the chunk that starts at sr / hr): the row pass, then the column pass.
void build_tables(const ScoreWs& w, const uint8_t* sr, const uint8_t* hr, int n, int H, int W, int C, hipStream_t s) {
  const size_t img_bytes = (size_t)H * W * C;
  {
    SradProfScope prof(s, SRAD_K_SCORE, 10.0 * n * H * W, 2.0 * n * img_bytes + 40.0 * n * (H + 1) * (W + 1));
    hipLaunchKernelGGL(sat_rows_kernel, dim3((n * (H + 1) + 3) / 4), dim3(256), 0, s, sr, hr, w.sat, n, H, W, C);
  }
  column_pass(w, n * kQ, H, W, s);
}

// The squared-error table of n pairs: its own row pass, the same column pass.
void build_sqerr_table(const ScoreWs& w, const uint8_t* sr, const uint8_t* hr, int n, int H, int W, int C, hipStream_t s) {
  const size_t img_bytes = (size_t)H * W * C;
  {
    SradProfScope prof(s, SRAD_K_SCORE, 3.0 * n * img_bytes, 2.0 * n * img_bytes + 8.0 * n * (H + 1) * (W + 1));
    hipLaunchKernelGGL(sqerr_rows_kernel, dim3((n * (H + 1) + 3) / 4), dim3(256), 0, s, sr, hr, w.sat, n, H, W, C);
  }
  column_pass(w, n, H, W, s);
}

// argument checks shared by srad_score_pairs and srad_anomaly_maps; `what` (the entry point) starts each message
int check_pairs(const char* what, const uint8_t* sr, const uint8_t* hr, const void* workspace, int n_img, int H, int W, int C) {
  SRAD_REQUIRE(sr && hr && workspace && n_img > 0 && H > 1 && W > 1, "%s: bad argument", what);
  SRAD_REQUIRE(C == 1 || C == 3, "%s: channels must be 1 or 3 (got %d)", what, C);
  SRAD_REQUIRE((long long)(H + 1) * (W + 1) < (1ll << 31), "%s: %dx%d images are too large for the 32-bit table offsets", what, H, W);
  return SRAD_OK;
}
int check_window(const char* what, int ws, int H, int W) {
  SRAD_REQUIRE(ws >= 1 && ws / 2 < H && ws / 2 < W && ws - 1 - ws / 2 < H && ws - 1 - ws / 2 < W,
               "%s: window %d needs more than one reflection of a %dx%d image", what, ws, H, W);
  return SRAD_OK;
}

// The sources of window_map_kernel.  Device side: `planes` and value().  Host side: one_size_instance = a list of one size takes
// the kernel's ONE instance, factor(C, ws) = the double value() is handed
// for a window size, build = the tables of a chunk, and the SradProfScope figures of a map launch per pixel: operations (per
// window size) and algorithmic bytes.
//
// SsimSrc: 1 - the SSIM map of one window size (the `ssim_map` src/metrics.py:66 averages), from the sweep's tables and with its
// per-pixel arithmetic (corner_ssim); factor = 1 / ws^2.  Bytes: the two fp32 luminance planes read once, the fp32 map written once.
struct SsimSrc {
  static constexpr int planes = kQ;
  static constexpr bool one_size_instance = false;
  static constexpr auto build = build_tables;
  static constexpr double ops_px = 40.0;
  static double bytes_px(int) { return 12.0; }
  static double factor(int, int ws) { return 1.0 / ((double)ws * (double)ws); }
  static __device__ __forceinline__ float value(const double* S, int H, int W, int i, int j, int ws, double factor) {
    return 1.0f - corner_ssim(S, H, W, i, j, ws, factor);
  }
};
// SqerrSrc: the squared-error map (above); factor = 1 / (C ws^2 255^2).  Bytes: the two u8 stacks read once, the fp32 map written once.
struct SqerrSrc {
  static constexpr int planes = 1;
  static constexpr bool one_size_instance = true;
  static constexpr auto build = build_sqerr_table;
  static constexpr double ops_px = 10.0;
  static double bytes_px(int C) { return 2.0 * C + 4.0; }
  static double factor(int C, int ws) { return 1.0 / ((double)C * (double)ws * (double)ws * 65025.0); }
  static __device__ __forceinline__ float value(const double* S, int H, int W, int i, int j, int ws, double factor) {
    return (float)(corner_sqerr(S, H, W, i, j, ws) * factor);
  }
};

// The window sizes ws[0 .. g) of one launch (g <= kWsGroup), each with its source's factor.
template <class Src>
WsList fill_ws_list(const int32_t* ws, int g, int C) {
  WsList wl{};
  for (int k = 0; k < g; ++k) { wl.ws[k] = (int)ws[k]; wl.dinv[k] = Src::factor(C, wl.ws[k]); }
  return wl;
}

int map_workspace_bytes(const char* what, int planes, int n_img, int H, int W, size_t* bytes) {
  SRAD_REQUIRE(bytes && n_img > 0 && H > 0 && W > 0, "%s: bad argument", what);
  *bytes = plan_score_ws(n_img, H, W, false, nullptr, planes).bytes;
  return SRAD_OK;
}

// The squared-error maps of window size 1 straight from the stacks (sqerr_pixel_kernel).
int sqerr_pixel_maps(const uint8_t* sr, const uint8_t* hr, int n_img, int H, int W, int C, float* map_out, hipStream_t s) {
  const size_t img_bytes = (size_t)H * W * C, npix = (size_t)n_img * H * W, groups = (npix + 3) / 4;
  SRAD_REQUIRE((groups + 255) / 256 < (1ull << 31), "error_maps: %d %dx%d images are too many pixels for one launch", n_img, H, W);
  const int vec = (reinterpret_cast<uintptr_t>(sr) | reinterpret_cast<uintptr_t>(hr)) % 4 == 0 && reinterpret_cast<uintptr_t>(map_out) % 16 == 0;
  SradProfScope prof(s, SRAD_K_SCORE, 3.0 * n_img * img_bytes, 2.0 * n_img * img_bytes + 4.0 * npix);
  const dim3 grid((unsigned)((groups + 255) / 256));
  const double inv = SqerrSrc::factor(C, 1);
  if (C == 1) hipLaunchKernelGGL(sqerr_pixel_kernel<1>, grid, dim3(256), 0, s, sr, hr, map_out, npix, inv, vec);
  else hipLaunchKernelGGL(sqerr_pixel_kernel<3>, grid, dim3(256), 0, s, sr, hr, map_out, npix, inv, vec);
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

// The four map entry points: the maps of the sizes ws_host[0 .. n_ws) of source Src reduced per pixel (reduce: 0 mean, 1 max)
// into map_out; `what` (the entry point) starts each message.  Every size is checked before anything is launched.
template <class Src>
int run_maps(const char* what, const uint8_t* sr, const uint8_t* hr, int n_img, int H, int W, int C, const int32_t* ws_host, int n_ws,
             int reduce, float* map_out, void* workspace, size_t workspace_bytes, void* stream) {
  SRAD_REQUIRE(map_out, "%s: bad argument", what);
  SRAD_REQUIRE(ws_host && n_ws >= 1, "%s: the window list is empty", what);
  SRAD_REQUIRE(reduce == 0 || reduce == 1, "%s: reduce must be 0 (mean) or 1 (max), got %d", what, reduce);
  SRAD_TRY(check_pairs(what, sr, hr, workspace, n_img, H, W, C));
  for (int k = 0; k < n_ws; ++k) SRAD_TRY(check_window(what, ws_host[k], H, W));
  const ScoreWs w = plan_score_ws(n_img, H, W, false, workspace, Src::planes);
  SRAD_REQUIRE(workspace_bytes >= w.bytes, "%s: workspace %zu bytes, %zu needed", what, workspace_bytes, w.bytes);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const size_t img_bytes = (size_t)H * W * C;
  if constexpr (std::is_same<Src, SqerrSrc>::value)
    if (n_ws == 1 && ws_host[0] == 1) return sqerr_pixel_maps(sr, hr, n_img, H, W, C, map_out, s);      // no window: no table
  const int nblk = (H * W + 255) / 256;
  const float inv_k = (float)(1.0 / (double)n_ws);
  for (int i0 = 0; i0 < n_img; i0 += w.chunk) {
    const int n = std::min(w.chunk, n_img - i0);
    Src::build(w, sr + (size_t)i0 * img_bytes, hr + (size_t)i0 * img_bytes, n, H, W, C, s);
    float* const out = map_out + (size_t)i0 * H * W;
    const dim3 grid((unsigned)((size_t)nblk * n));
    for (int k0 = 0; k0 < n_ws; k0 += kWsGroup) {      // up to kWsGroup window sizes per launch; later launches continue from `out`
      const int g = std::min(kWsGroup, n_ws - k0);
      const WsList wl = fill_ws_list<Src>(ws_host + k0, g, C);
      const int first = k0 == 0;
      const float scale = (reduce == 0 && k0 + g == n_ws) ? inv_k : 1.0f;
      SradProfScope prof(s, SRAD_K_SCORE, Src::ops_px * n * H * W * g, Src::bytes_px(C) * n * H * W);
      const bool rows = W % 64 == 0;
      auto kernel = rows ? window_map_kernel<Src, true> : window_map_kernel<Src, false>;
      if constexpr (Src::one_size_instance)
        if (n_ws == 1) kernel = rows ? window_map_kernel<Src, true, true> : window_map_kernel<Src, false, true>;
      hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, w.sat, out, H, W, wl, g, reduce, first, scale, nblk);
    }
  }
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

}  // namespace

extern "C" {

int srad_to_u8_hwc(const float* x, int B, int C, int H, int W, float rgb_range, uint8_t* out, void* stream) {
  SRAD_REQUIRE(x && out && B > 0 && C > 0 && H > 0 && W > 0, "to_u8_hwc: bad argument");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const size_t total = (size_t)B * C * H * W;
  SradProfScope prof(s, SRAD_K_SCORE, (double)total, 5.0 * total);
  hipLaunchKernelGGL(to_u8_hwc_kernel, dim3(grid1d(total)), dim3(256), 0, s, x, out, B, C, H * W, 255.0f / rgb_range);
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

int srad_quantize(const float* x, float* y, int64_t n, float rgb_range, void* stream) {
  SRAD_REQUIRE(x && y && n > 0, "quantize: bad argument");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(quantize_kernel, dim3(grid1d((size_t)n)), dim3(256), 0, s, x, y, (size_t)n, 255.0f / rgb_range);
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

int srad_score_workspace_bytes(int n_img, int H, int W, size_t* bytes) {
  SRAD_REQUIRE(bytes && n_img > 0 && H > 0 && W > 0, "score_workspace_bytes: bad argument");
  *bytes = plan_score_ws(n_img, H, W, true, nullptr).bytes;
  return SRAD_OK;
}

int srad_score_pairs(const uint8_t* sr, const uint8_t* hr, int n_img, int H, int W, int C, const int32_t* ws_host,
                     int n_ws, double* ssim_out, double* mse_out, double* psnr_out, void* workspace,
                     size_t workspace_bytes, void* stream) {
  SRAD_TRY(check_pairs("score_pairs", sr, hr, workspace, n_img, H, W, C));
  SRAD_REQUIRE(n_ws == 0 || (ws_host && ssim_out), "score_pairs: window list / output missing");
  const ScoreWs w = plan_score_ws(n_img, H, W, true, workspace);
  SRAD_REQUIRE(workspace_bytes >= w.bytes, "score_pairs: workspace %zu bytes, %zu needed", workspace_bytes, w.bytes);
  for (int k = 0; k < n_ws; ++k) SRAD_TRY(check_window("score_pairs", ws_host[k], H, W));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const size_t img_bytes = (size_t)H * W * C;
  const bool want_mse = mse_out && psnr_out;
  for (int i0 = 0; i0 < n_img && (n_ws > 0 || want_mse); i0 += w.chunk) {
    const int n = std::min(w.chunk, n_img - i0);
    const uint8_t* srp = sr + (size_t)i0 * img_bytes;
    const uint8_t* hrp = hr + (size_t)i0 * img_bytes;
    if (want_mse) {                                   // block partials in the (not yet used) SSIM partial area: nb <= kWsGroup * nblk
      const int nb = std::min(64, w.nblk);
      SradProfScope prof(s, SRAD_K_SCORE, 3.0 * n * img_bytes, 2.0 * n * img_bytes);
      hipLaunchKernelGGL(mse_partial_kernel, dim3(nb, n), dim3(256), 0, s, srp, hrp, w.partial, img_bytes, nb);
      hipLaunchKernelGGL(mse_finish_kernel, dim3((n + 63) / 64), dim3(64), 0, s, w.partial, mse_out + i0, psnr_out + i0, n, nb, (double)img_bytes);
    }
    if (n_ws == 0) continue;
    build_tables(w, srp, hrp, n, H, W, C, s);
    for (int k0 = 0; k0 < n_ws; k0 += kWsGroup) {      // up to kWsGroup window sizes per launch
      const int g = std::min(kWsGroup, n_ws - k0);
      const WsList wl = fill_ws_list<SsimSrc>(ws_host + k0, g, C);
      {
        // algorithmic bytes per (pair, window): the two fp32 luminance planes read once
        SradProfScope prof(s, SRAD_K_SCORE, 40.0 * n * H * W * g, 8.0 * n * H * W * g);
        const SweepKernel kern = sweep_kernel(H, W);
        if (kern == kSweepLds) {
          int pmin = wl.ws[0] / 2, pmax = pmin;
          for (int k = 1; k < g; ++k) { pmin = std::min(pmin, wl.ws[k] / 2); pmax = std::max(pmax, wl.ws[k] / 2); }
          const int rb = 1024 / W, t_first = -pmax, nt = H - 1 - pmin - t_first + 1, nt_blocks = (nt + rb - 1) / rb;
          const size_t lds = ((size_t)2 * kQ * rb * (W + 1) + 32) * sizeof(double);
          int lw = 0;
          while ((1 << lw) < W) ++lw;
          SRAD_TRY(srad_launch_dyn<ssim_rows_lds_kernel>(dim3((unsigned)((size_t)nt_blocks * n)), dim3(1024), lds, s, w.sat, w.partial, H, lw,
                                                         wl, g, t_first, nt_blocks));
        } else if (kern == kSweepRows)
          hipLaunchKernelGGL(ssim_eval_kernel<true>, dim3((unsigned)((size_t)w.nblk * g * n)), dim3(256), 0, s, w.sat, w.partial, H, W, wl,
                             w.nblk, g, n);
        else
          hipLaunchKernelGGL(ssim_eval_kernel<false>, dim3((unsigned)((size_t)w.nblk * g * n)), dim3(256), 0, s, w.sat, w.partial, H, W, wl,
                             w.nblk, g, n);
      }
      hipLaunchKernelGGL(ssim_finish_kernel, dim3(n * g), dim3(256), 0, s, w.partial, ssim_out + (size_t)i0 * n_ws, n, g,
                         w.nblk, n_ws, k0, 1.0 / ((double)H * W));
    }
  }
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

int srad_score_plan(int n_img, int H, int W, int* kernel, int* chunk) {
  SRAD_REQUIRE(kernel && chunk && n_img > 0 && H > 1 && W > 1, "score_plan: bad argument");
  *kernel = (int)sweep_kernel(H, W);
  *chunk = chunk_images(n_img, H, W);
  return SRAD_OK;
}

int srad_anomaly_map_workspace_bytes(int n_img, int H, int W, size_t* bytes) {
  return map_workspace_bytes("anomaly_map_workspace_bytes", SsimSrc::planes, n_img, H, W, bytes);
}

int srad_anomaly_maps(const uint8_t* sr, const uint8_t* hr, int n_img, int H, int W, int C, int ws, float* map_out,
                      void* workspace, size_t workspace_bytes, void* stream) {
  const int32_t one = ws;
  return run_maps<SsimSrc>("anomaly_maps", sr, hr, n_img, H, W, C, &one, 1, 0, map_out, workspace, workspace_bytes, stream);
}

int srad_anomaly_maps_multi(const uint8_t* sr, const uint8_t* hr, int n_img, int H, int W, int C, const int32_t* ws_host, int n_ws,
                            int reduce, float* map_out, void* workspace, size_t workspace_bytes, void* stream) {
  return run_maps<SsimSrc>("anomaly_maps_multi", sr, hr, n_img, H, W, C, ws_host, n_ws, reduce, map_out, workspace, workspace_bytes, stream);
}

int srad_error_map_workspace_bytes(int n_img, int H, int W, size_t* bytes) {
  return map_workspace_bytes("error_map_workspace_bytes", SqerrSrc::planes, n_img, H, W, bytes);
}

// the per-pixel form of the MSE score of src/evaluate.py:251-265; ws = 1 takes the table-free sqerr_pixel_kernel
int srad_error_maps(const uint8_t* sr, const uint8_t* hr, int n_img, int H, int W, int C, int ws, float* map_out, void* workspace,
                    size_t workspace_bytes, void* stream) {
  const int32_t one = ws;
  return run_maps<SqerrSrc>("error_maps", sr, hr, n_img, H, W, C, &one, 1, 0, map_out, workspace, workspace_bytes, stream);
}

// the multi-scale form of srad_error_maps; a list of one size is that size's srad_error_maps
int srad_error_maps_multi(const uint8_t* sr, const uint8_t* hr, int n_img, int H, int W, int C, const int32_t* ws_host, int n_ws,
                          int reduce, float* map_out, void* workspace, size_t workspace_bytes, void* stream) {
  return run_maps<SqerrSrc>("error_maps_multi", sr, hr, n_img, H, W, C, ws_host, n_ws, reduce, map_out, workspace, workspace_bytes, stream);
}

int srad_val_metrics(const float* sr, const float* hr, int B, int C, int H, int W, float rgb_range, double* psnr_out,
                     double* ssim_out, void* workspace, size_t workspace_bytes, void* stream) {
  (void)workspace; (void)workspace_bytes;
  SRAD_REQUIRE(sr && hr && psnr_out && ssim_out && B > 0, "val_metrics: bad argument");
  SRAD_REQUIRE(C == 1 || C == 3, "val_metrics: channels must be 1 or 3 (got %d)", C);
  SRAD_REQUIRE(H > 0 && W > 0, "val_metrics: bad argument");
  // the reference shaves 4 rows off each side whenever the WIDTH is above 8: no row is left, its PSNR is NaN and its SSIM raises
  SRAD_REQUIRE(W <= 8 || H > 8, "val_metrics: a %dx%d image has no rows left after the 4-px shave (applied when the width is above 8)",
               H, W);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(val_metrics_kernel, dim3(B), dim3(256), 0, s, sr, hr, C, H, W, rgb_range, psnr_out, ssim_out);
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

// sklearn.metrics.roc_auc_score for binary labels == Mann-Whitney U with ties counted one half
// (reference call sites src/evaluate.py:245,263-265).  Host arithmetic: n is the number of test images.
int srad_roc_auc(const int32_t* labels, const double* scores, int n, double* auc) {
  SRAD_REQUIRE(labels && scores && auc && n > 0, "roc_auc: bad argument");
  std::vector<int> idx(n);
  for (int i = 0; i < n; ++i) idx[i] = i;
  std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return scores[a] < scores[b]; });
  double npos = 0, nneg = 0, rank_sum = 0;
  for (int i = 0; i < n; ++i) (labels[i] ? npos : nneg) += 1;
  if (npos == 0 || nneg == 0)
    return srad_set_error(SRAD_ERR_ARG, "Only one class present in y_true. ROC AUC score is not defined in that case.");
  int i = 0;
  while (i < n) {
    int j = i;
    while (j + 1 < n && scores[idx[j + 1]] == scores[idx[i]]) ++j;
    const double r = 0.5 * (i + j) + 1.0;            // average rank of the tie group
    for (int k = i; k <= j; ++k)
      if (labels[idx[k]]) rank_sum += r;
    i = j + 1;
  }
  *auc = (rank_sum - npos * (npos + 1) / 2.0) / (npos * nneg);
  return SRAD_OK;
}

// sklearn.metrics.average_precision_score, sum over distinct scores from the highest down of (R_k - R_k-1) * P_k, and the best
// F1 = 2 tp / (tp + fp + P) over those thresholds, for the image scores on the host: the definitions of srad_pixel_pr
// (kernels_pixel_pr.hip), with the same exact integer comparison of two F1 values (the earlier, higher threshold keeps a tie).
int srad_average_precision(const int32_t* labels, const double* scores, int n, double* ap, double* f1max) {
  SRAD_REQUIRE(labels && scores && ap && f1max && n > 0, "average_precision: bad argument");
  int64_t npos = 0;
  for (int i = 0; i < n; ++i) {
    if (scores[i] != scores[i]) return srad_set_error(SRAD_ERR_ARG, "average_precision: score %d of %d is NaN", i, n);
    npos += labels[i] != 0;
  }
  if (npos == 0)
    return srad_set_error(SRAD_ERR_ARG, "No positive class found in y_true. Average precision is not defined in that case.");
  std::vector<int> idx(n);
  for (int i = 0; i < n; ++i) idx[i] = i;
  std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return scores[a] > scores[b]; });
  int64_t tp = 0, fp = 0, best_tp = 0, best_den = 1;             // F1 0 until a point beats it
  double sum = 0.0;
  int i = 0;
  while (i < n) {
    const int64_t tp0 = tp;
    int j = i;
    while (j < n && scores[idx[j]] == scores[idx[i]]) {
      (labels[idx[j]] ? tp : fp) += 1;
      ++j;
    }
    sum += (double)(tp - tp0) * (double)tp / (double)(tp + fp);
    const int64_t den = tp + fp + npos;
    if (tp * best_den > best_tp * den) {
      best_tp = tp;
      best_den = den;
    }
    i = j;
  }
  *ap = sum / (double)npos;
  *f1max = 2.0 * (double)best_tp / (double)best_den;
  return SRAD_OK;
}

}  // extern "C"
