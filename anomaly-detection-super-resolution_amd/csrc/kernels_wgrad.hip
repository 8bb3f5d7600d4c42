// kernels_wgrad.hip - everything weight-gradient of the training step on gfx950 (reference src/trainer.py:152-222: the
// parameter gradients of loss.backward() for Linear and conv2d layers), and the launches of the split-K queue that every
// parameter gradient's partial sums go through (wgrad_queue.h holds the queue's structs and all of its decisions).
//
//   wgrad_kernel            dW += dY^T A(X)      64 x 64 tiles, MFMA straight from global memory, no LDS staging (wgrad_body)
//   wgrad_multi_kernel      up to five Linear layers' wgrad_body in one launch (the deferred launch of a Swin block)
//   wgrad_multi_hh_kernel   ... when every layer has both operands stored as bf16
//   wgrad80_kernel          80 -> 80 channels, one 80 x 80 tile per tap
//   wgrad_conv9_kernel      3x3 stride-1 C -> C convolutions (C <= 80), all nine taps per workgroup
//   wgrad_reduce_kernel     sums a batch of queued items' partials into dW / db / column-sum destinations, fixed order
//   decide_tile64, decide_wgrad80, decide_wgrad_conv9, decide_wgrad, decide_multi: which kernel, split geometry, grid (host only)
//   queue_partials, launch_wgrad80, launch_wgrad_conv9, launch_wgrad, defer_wgrad, check_wgrad: reservation and launch of a decision
//   srad_plan_wgrad, srad_plan_wgrad_deferred: a decision reported instead of launched (include/srad.h srad_wgrad_plan)
//   srad_launch_wgrad*, srad_wgrad_*: the entry points (srad_common.h), among them the column-sum reservations the LayerNorm
//   and attention backward kernels use (srad_wgrad_reserve_colsum, srad_wgrad_queue_ln_partials)
#include "srad_common.h"
#include <type_traits>
#include <algorithm>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

namespace {

// ------------------------------------------------------------------------------------------
// Weight gradient.  The contraction runs over the rows m (tokens / pixels), which are the SLOW axis of
// both operands in memory ([m][n] and [m][c], channel contiguous).  An MFMA lane supplies A[i][k] and
// B[k][j] for ONE i / j and a few k, and nothing fixes which n a tile row i stands for - so lane
// (fq, fr) loads the float4 dY[m][n0 + 4 fr .. +3] and uses component e as row fr of n-subtile e
// (n = n0 + 4 fr + e), likewise X for the c-subtiles.  Sixteen lanes then read 256 contiguous bytes of
// one row: fully coalesced fragment loads, 2 loads feed 16 MFMAs, and no LDS transpose is needed.
//   fp32: v_mfma_f32_16x16x4_f32, k = 4 rows per step (row m0 + fq)
//   bf16: v_mfma_f32_16x16x32_bf16, k = 32 rows per step (rows m0 + 8 fq + t, t = 0..7)
// One workgroup = 4 waves on one 64 x 64 (n, c) tile of one tap, each wave on its own rows of the
// workgroup's row range (split-K); waves are summed through LDS.
// Split-K partials go to a workspace with plain stores and are summed (fixed order: bit-reproducible
// gradients) by wgrad_reduce_kernel, ONE launch for a batch of up to 8 layers.  Two things that were tried
// and measured on MI355X before this: float atomicAdd into dW (device-scope atomics on a few hundred
// addresses serialise: 60-170 us per layer) and a last-arriver reduction inside the kernel (the agent-scope
// release/acquire fences it needs write back / invalidate a whole XCD L2 because the eight L2s are not
// coherent with each other: 60-90 us per layer).  A kernel boundary is the cheap cross-XCD barrier.
// ------------------------------------------------------------------------------------------
#ifndef SRAD_WGRAD_PREFETCH
#define SRAD_WGRAD_PREFETCH 1   /* two register sets: measured best together with the two-stream backward */
#endif
constexpr int WG_TS = 64 * 64 + 64;          // floats per partial: the tile and its 64 bias sums

// FULL: Linear layers whose row splits are whole 128-row steps and whose DropPath factor is constant over a 32-row
// wave step - no row / column / padding masks at all (columns past N / Cin read clamped real data into tile rows the
// final store drops), the factor is one value per wave step: fewer registers (two waves per SIMD) and ~200 fewer
// VALU instructions per step.
// XH / YH (FULL only): X / dY are stored as bf16 - half the operand bytes and prefetch registers; the 8 rows x 4 columns a
// lane holds are transposed into the four 8-row MFMA operands with v_perm_b32 instead of being converted.  A bf16 dY is
// already multiplied by its DropPath factor (its producer did that), so no per-step factor either.
// LDS2: the waves' tiles are summed pairwise through TWO tile slots instead of four (waves 2, 3 store, waves 0, 1 add and
// store, then one sum of two): 36 KB instead of 70 KB, two barriers instead of one - for the all-bf16 kernel, whose
// registers allow three workgroups per CU.  PF2: two register sets of operand rows (the next step in flight during this one's
// MFMAs); the all-bf16 kernel at three waves per SIMD runs with one.
template <int PREC, bool CONV, bool FULL = false, bool XH = false, bool YH = false, bool LDS2 = false, bool PF2 = (SRAD_WGRAD_PREFETCH != 0)>
__device__ __forceinline__ void wgrad_body(const WgradParams& p, const int ksplit, const int tn, const int tc,
                                           float* __restrict__ part, const int L) {
  static_assert(!(XH || YH) || (!CONV && PREC == SRAD_PREC_BF16), "bf16 operand storage: Linear layers, bf16 MFMA path");
  extern __shared__ __attribute__((aligned(16))) float wsm[];     // [4 waves][64][68] + [4][64] bias + flag
  constexpr int TST = 68;
  float* const dbs = wsm + (LDS2 ? 2 : 4) * 64 * TST;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  // XCD-aware order: workgroups are dealt round-robin over the 8 XCDs (linear id L runs on XCD L % 8).  With the row
  // split fastest (ks = L % ksplit, ksplit a multiple of 8) every tile of one row range lands on the same XCD, so the
  // range's dY / X rows are fetched into ONE L2 and all the tiles' re-reads of them hit there.
  const int ks = L % ksplit, tile_id = L / ksplit;
  const int bx = tile_id % tn, by = (tile_id / tn) % tc, tap = tile_id / (tn * tc);
  const int n0 = bx * 64, c0 = by * 64;

  constexpr int KR = PREC == SRAD_PREC_BF16 ? 32 : 4;        // rows per wave step
  constexpr int RL = PREC == SRAD_PREC_BF16 ? 8 : 1;         // rows per lane per step
  const int rows_per = srad_wgrad_rows_per<4 * KR>(p.M, ksplit);
  const int mb = ks * rows_per;
  const int me = min(p.M, mb + rows_per);

  const int ncol = n0 + 4 * fr, ccol = c0 + 4 * fr;
  const bool n_ok = ncol < p.N, c_ok = ccol < p.Cin;
  const unsigned noff = (unsigned)(min(ncol, p.N - 4) + p.ycol0);
  const unsigned coff = (unsigned)min(ccol, p.Cin - 4);
  [[maybe_unused]] const int pad = p.ntaps == 9 ? 1 : 0;
  [[maybe_unused]] const int ky = p.ntaps == 9 ? tap / 3 : 0, kx = p.ntaps == 9 ? tap - (tap / 3) * 3 : 0;
  [[maybe_unused]] const int hwo = p.Ho * p.Wo;

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 bsum = f32x4{0.f, 0.f, 0.f, 0.f};
  const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};

  // every load is unconditional on a clamped address; masking happens on the registers afterwards.
  // The next step's loads are issued before this step's MFMAs (two register sets).
  constexpr int NSET = PF2 ? 2 : 1;
  f32x4 av[NSET][YH ? 1 : RL], bv[NSET][XH ? 1 : RL];
  u32x2 avh[NSET][YH ? RL : 1], bvh[NSET][XH ? RL : 1];   // bf16 storage: 4 values = 8 bytes per row
  unsigned okm[2];                    // bit t: a row valid, bit 8 + t: b row valid
  float rs[NSET][FULL ? 1 : RL];
  auto load_step = [&](int m0, auto set_c) {
    constexpr int set = decltype(set_c)::value;
    if constexpr (FULL) {
#pragma unroll
      for (int t = 0; t < RL; ++t) {
        const size_t mr = (size_t)(m0 + RL * fq + t);
        if constexpr (YH) avh[set][t] = *reinterpret_cast<const u32x2*>(reinterpret_cast<const __bf16*>(p.dY) + mr * p.ldy + noff);
        else av[set][t] = *reinterpret_cast<const f32x4*>(p.dY + mr * p.ldy + noff);
        if constexpr (XH) bvh[set][t] = *reinterpret_cast<const u32x2*>(reinterpret_cast<const __bf16*>(p.X) + mr * p.ldx + coff);
        else bv[set][t] = *reinterpret_cast<const f32x4*>(p.X + mr * p.ldx + coff);
      }
      if constexpr (!YH) rs[set][0] = p.row_scale ? p.row_scale[m0 / p.rps] : 1.f;
      return;
    }
    unsigned ok = 0u;
    [[maybe_unused]] int bb = 0, oy = 0, ox = 0;
    if constexpr (CONV) {                 // pixel of the lane's first row; the following rows step from it
      const int mf = min(m0 + RL * fq, p.M - 1);
      bb = mf / hwo;
      const int rem = mf - bb * hwo;
      oy = rem / p.Wo;
      ox = rem - oy * p.Wo;
    }
#pragma unroll
    for (int t = 0; t < RL; ++t) {
      const int m = m0 + RL * fq + t;
      const int mc = min(m, p.M - 1);
      if constexpr (YH) avh[set][t] = *reinterpret_cast<const u32x2*>(reinterpret_cast<const __bf16*>(p.dY) + (size_t)mc * p.ldy + noff);
      else av[set][t] = *reinterpret_cast<const f32x4*>(p.dY + (size_t)mc * p.ldy + noff);
      size_t xr = (size_t)mc;
      bool in = true;
      if constexpr (CONV) {
        if (t > 0 && m < p.M) {           // next pixel in raster order
          ++ox;
          if (ox == p.Wo) { ox = 0; ++oy; if (oy == p.Ho) { oy = 0; ++bb; } }
        }
        const int iy = oy * p.stride - pad + ky, ix = ox * p.stride - pad + kx;
        in = iy >= 0 && iy < p.Hi && ix >= 0 && ix < p.Wi;
        xr = (size_t)((bb * p.Hi + min(max(iy, 0), p.Hi - 1)) * p.Wi + min(max(ix, 0), p.Wi - 1));
      }
      if constexpr (XH) bvh[set][t] = *reinterpret_cast<const u32x2*>(reinterpret_cast<const __bf16*>(p.X) + xr * p.ldx + coff);
      else bv[set][t] = *reinterpret_cast<const f32x4*>(p.X + xr * p.ldx + coff);
      rs[set][t] = (!YH && p.row_scale) ? p.row_scale[mc / p.rps] : 1.f;
      ok |= ((m < me && n_ok) ? 1u : 0u) << t;
      ok |= ((m < me && c_ok && in) ? 1u : 0u) << (8 + t);
    }
    okm[set] = ok;
  };
  auto compute_step = [&](auto set_c) {
    constexpr int set = decltype(set_c)::value;
    f32x4 a[RL], b[RL];
    // 8 rows x (2 dwords = 4 bf16 columns) -> operand e = column e of the 8 rows: dword t/2 of operand 2 w + half takes the
    // low (half 0) or high (half 1) 16 bits of dword w of rows t and t + 1
    auto transpose_h = [&](const u32x2 (&src)[RL], bf16x8 (&dst)[4]) {
#pragma unroll
      for (int w = 0; w < 2; ++w) {
        u32x4 lo, hi;
#pragma unroll
        for (int t2 = 0; t2 < 4; ++t2) {
          lo[t2] = __builtin_amdgcn_perm(src[2 * t2 + 1][w], src[2 * t2][w], 0x05040100u);
          hi[t2] = __builtin_amdgcn_perm(src[2 * t2 + 1][w], src[2 * t2][w], 0x07060302u);
        }
        dst[2 * w] = __builtin_bit_cast(bf16x8, lo);
        dst[2 * w + 1] = __builtin_bit_cast(bf16x8, hi);
      }
    };
#pragma unroll
    for (int t = 0; t < RL; ++t) {
      if constexpr (FULL) {
        if constexpr (YH) {                                 // fp32 view of the row for the bias sums only
#pragma unroll
          for (int w = 0; w < 2; ++w) {
            a[t][2 * w] = __builtin_bit_cast(float, avh[set][t][w] << 16);
            a[t][2 * w + 1] = __builtin_bit_cast(float, avh[set][t][w] & 0xffff0000u);
          }
        } else {
          a[t] = av[set][t] * rs[set][0];
        }
        if constexpr (!XH) b[t] = bv[set][t];
      } else {
        if constexpr (YH) {
          if (!((okm[set] >> t) & 1u)) avh[set][t] = u32x2{0u, 0u};
#pragma unroll
          for (int w = 0; w < 2; ++w) {
            a[t][2 * w] = __builtin_bit_cast(float, avh[set][t][w] << 16);
            a[t][2 * w + 1] = __builtin_bit_cast(float, avh[set][t][w] & 0xffff0000u);
          }
        } else {
          a[t] = ((okm[set] >> t) & 1u) ? av[set][t] * rs[set][t] : zero4;
        }
        if constexpr (XH) { if (!((okm[set] >> (8 + t)) & 1u)) bvh[set][t] = u32x2{0u, 0u}; }
        else b[t] = ((okm[set] >> (8 + t)) & 1u) ? bv[set][t] : zero4;
      }
      bsum += a[t];
    }
    if constexpr (PREC == SRAD_PREC_BF16) {
      bf16x8 ah[4], bh[4];
      if constexpr (YH) {
        transpose_h(avh[set], ah);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int t = 0; t < 8; ++t) ah[e][t] = (__bf16)a[t][e];
      }
      if constexpr (XH) {
        transpose_h(bvh[set], bh);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int t = 0; t < 8; ++t) bh[e][t] = (__bf16)b[t][e];
      }
#pragma unroll
      for (int en = 0; en < 4; ++en)
#pragma unroll
        for (int ec = 0; ec < 4; ++ec)
          acc[en][ec] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[en], bh[ec], acc[en][ec], 0, 0, 0);
    } else {
#pragma unroll
      for (int en = 0; en < 4; ++en)
#pragma unroll
        for (int ec = 0; ec < 4; ++ec)
          acc[en][ec] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0][en], b[0][ec], acc[en][ec], 0, 0, 0);
    }
  };

  {
    using S0 = std::integral_constant<int, 0>;
    using S1 = std::integral_constant<int, 1>;
    constexpr int ST = 4 * KR;
    int m0 = mb + wave * KR;
    if constexpr (PF2) {
      if (m0 < me) load_step(m0, S0{});
      while (m0 < me) {
        if (m0 + ST < me) load_step(m0 + ST, S1{});
        compute_step(S0{});
        m0 += ST;
        if (m0 >= me) break;
        if (m0 + ST < me) load_step(m0 + ST, S0{});
        compute_step(S1{});
        m0 += ST;
      }
    } else {
      (void)sizeof(S1);
      for (; m0 < me; m0 += ST) { load_step(m0, S0{}); compute_step(S0{}); }
    }
  }

  // ---- the four waves' partial tiles through LDS (plain 16-byte stores): lane (fq, fr) element e of
  //      acc[en][ec] is (n = 16 fq + 4 e + en, c = 4 fr + ec) ----
  {
    float* const mine = wsm + (LDS2 ? (wave & 1) : wave) * 64 * TST;
    auto put_tile = [&]() __attribute__((always_inline)) {
#pragma unroll
      for (int en = 0; en < 4; ++en)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          *reinterpret_cast<f32x4*>(mine + (16 * fq + 4 * e + en) * TST + 4 * fr) =
              f32x4{acc[en][0][e], acc[en][1][e], acc[en][2][e], acc[en][3][e]};
    };
    if constexpr (LDS2) {
      if (wave >= 2) put_tile();
      __syncthreads();
      if (wave < 2) {
#pragma unroll
        for (int en = 0; en < 4; ++en)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const f32x4 o = *reinterpret_cast<const f32x4*>(mine + (16 * fq + 4 * e + en) * TST + 4 * fr);
#pragma unroll
            for (int ec = 0; ec < 4; ++ec) acc[en][ec][e] += o[ec];
          }
        put_tile();                       // its own slot again: no other wave touches it before the barrier below
      }
    } else {
      put_tile();
    }
    // bias partial: sum over the four row groups fq, then lanes fq == 0 hold n = 4 fr + e
#pragma unroll
    for (int e = 0; e < 4; ++e) { bsum[e] += __shfl_xor(bsum[e], 16); bsum[e] += __shfl_xor(bsum[e], 32); }
    if (fq == 0) *reinterpret_cast<f32x4*>(dbs + wave * 64 + 4 * fr) = bsum;
  }
  __syncthreads();
  const bool do_bias = p.db != nullptr && by == 0 && tap == 0;
  // thread t owns the float4s e4 = t + 256 j of the tile (n = e4 / 16, c = 4 (e4 % 16))
  f32x4 v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int e4 = tid + 256 * j, nl = e4 >> 4, cl = (e4 & 15) * 4;
    const float* q = wsm + nl * TST + cl;
    if constexpr (LDS2)
      v[j] = *reinterpret_cast<const f32x4*>(q) + *reinterpret_cast<const f32x4*>(q + 64 * TST);
    else
      v[j] = (*reinterpret_cast<const f32x4*>(q) + *reinterpret_cast<const f32x4*>(q + 64 * TST)) +
             (*reinterpret_cast<const f32x4*>(q + 2 * 64 * TST) + *reinterpret_cast<const f32x4*>(q + 3 * 64 * TST));
  }
  float vb = 0.f;
  if (tid < 64) vb = (dbs[tid] + dbs[64 + tid]) + (dbs[128 + tid] + dbs[192 + tid]);

  if (ksplit > 1) {                      // partial tile for wgrad_reduce_kernel
    float* const mypart = part + ((size_t)tile_id * ksplit + ks) * WG_TS;
#pragma unroll
    for (int j = 0; j < 4; ++j) *reinterpret_cast<f32x4*>(mypart + 4 * (tid + 256 * j)) = v[j];
    if (tid < 64) mypart[4096 + tid] = vb;
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int e4 = tid + 256 * j, nl = e4 >> 4, cl = (e4 & 15) * 4;
    const int n = n0 + nl;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = srad_real_channel(c0 + cl + e, p.grp_real, p.grp_pad, p.cin_real);
      if (n < p.n_real && c < p.cin_real) {
        float* dst = p.dW + ((size_t)n * p.cin_real + c) * p.ntaps + tap;
        *dst += v[j][e] * p.alpha;
      }
    }
  }
  if (do_bias && tid < 64 && n0 + tid < p.n_real) p.db[n0 + tid] += vb * p.alpha;
}

// ------------------------------------------------------------------------------------------
// Weight gradient of an 80 -> 80 channel convolution (DRN-L's 160 RCAB convolutions, src/drn.py:143-158) with ONE
// 80 x 80 tile per tap: the 64 x 64 tiles pad 80 channels to 128 on both sides (2.56x the MFMAs and operand loads).
// Same scheme as wgrad_body - fragments straight from global memory, contraction over the token axis, four waves on
// different rows, partial tiles for the reduce kernel - but a lane owns FIVE consecutive channels (a 16-byte and a
// 4-byte load at channel 5 fr): component e of the quintuple is row fr of sub-tile e, so tile row i of sub-tile en
// stands for channel 5 i + en and the tile is 5 x 5 MFMA tiles.  bf16 MFMA, stride 1, 1 or 9 taps.
// ------------------------------------------------------------------------------------------
constexpr int W80_TS = 84;                          // LDS row stride of a wave's 80 x 80 partial tile
constexpr int W80_PART = 80 * 80 + 80;              // floats per partial: the tile (row-major) and 80 bias sums
constexpr size_t W80_LDS = (size_t)(4 * 80 * W80_TS + 4 * 80) * sizeof(float);
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));

template <bool CONV>
__global__ __launch_bounds__(256) void wgrad80_kernel(const WgradParams p, const int ksplit, float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float wsm[];
  float* const dbs = wsm + 4 * 80 * W80_TS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int L = blockIdx.x;
  const int ks = L % ksplit, tap = L / ksplit;      // row split fastest: one XCD per row range (see wgrad_body)
  const int rows_per = srad_wgrad_rows_per<128>(p.M, ksplit);
  const int mb = ks * rows_per;
  const int me = min(p.M, mb + rows_per);
  const unsigned noff = (unsigned)(5 * fr + p.ycol0), coff = (unsigned)(5 * fr);
  [[maybe_unused]] const int pad = p.ntaps == 9 ? 1 : 0;
  [[maybe_unused]] const int ky = p.ntaps == 9 ? tap / 3 : 0, kx = p.ntaps == 9 ? tap - (tap / 3) * 3 : 0;
  [[maybe_unused]] const int hwo = p.Ho * p.Wo;

  f32x4 acc[5][5];
#pragma unroll
  for (int i = 0; i < 5; ++i)
#pragma unroll
    for (int j = 0; j < 5; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bsum[5] = {0.f, 0.f, 0.f, 0.f, 0.f};

  f32x4 av4[2][8], bv4[2][8];
  float av1[2][8], bv1[2][8];
  unsigned okm[2];
  auto load_step = [&](int m0, auto set_c) {
    constexpr int set = decltype(set_c)::value;
    unsigned ok = 0u;
    [[maybe_unused]] int bb = 0, oy = 0, ox = 0;
    if constexpr (CONV) {
      const int mf = min(m0 + 8 * fq, p.M - 1);
      bb = mf / hwo;
      const int rem = mf - bb * hwo;
      oy = rem / p.Wo;
      ox = rem - oy * p.Wo;
    }
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int m = m0 + 8 * fq + t;
      const int mc = min(m, p.M - 1);
      const float* ap = p.dY + (size_t)mc * p.ldy + noff;
      av4[set][t] = *reinterpret_cast<const f32x4u*>(ap);
      av1[set][t] = ap[4];
      size_t xr = (size_t)mc;
      bool in = true;
      if constexpr (CONV) {
        if (t > 0 && m < p.M) {
          ++ox;
          if (ox == p.Wo) { ox = 0; ++oy; if (oy == p.Ho) { oy = 0; ++bb; } }
        }
        const int iy = oy - pad + ky, ix = ox - pad + kx;
        in = iy >= 0 && iy < p.Hi && ix >= 0 && ix < p.Wi;
        xr = (size_t)((bb * p.Hi + min(max(iy, 0), p.Hi - 1)) * p.Wi + min(max(ix, 0), p.Wi - 1));
      }
      const float* bp = p.X + xr * p.ldx + coff;
      bv4[set][t] = *reinterpret_cast<const f32x4u*>(bp);
      bv1[set][t] = bp[4];
      ok |= (m < me ? 1u : 0u) << t;
      ok |= ((m < me && in) ? 1u : 0u) << (8 + t);
    }
    okm[set] = ok;
  };
  auto compute_step = [&](auto set_c) {
    constexpr int set = decltype(set_c)::value;
    bf16x8 ah[5], bh[5];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const bool aok = (okm[set] >> t) & 1u, bok = (okm[set] >> (8 + t)) & 1u;
#pragma unroll
      for (int e = 0; e < 5; ++e) {
        const float a = aok ? (e < 4 ? av4[set][t][e < 4 ? e : 0] : av1[set][t]) : 0.f;
        const float b = bok ? (e < 4 ? bv4[set][t][e < 4 ? e : 0] : bv1[set][t]) : 0.f;
        bsum[e] += a;
        ah[e][t] = (__bf16)a;
        bh[e][t] = (__bf16)b;
      }
    }
#pragma unroll
    for (int en = 0; en < 5; ++en)
#pragma unroll
      for (int ec = 0; ec < 5; ++ec)
        acc[en][ec] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[en], bh[ec], acc[en][ec], 0, 0, 0);
  };
  {
    using S0 = std::integral_constant<int, 0>;
    using S1 = std::integral_constant<int, 1>;
    int m0 = mb + wave * 32;
    if (m0 < me) load_step(m0, S0{});
    while (m0 < me) {
      if (m0 + 128 < me) load_step(m0 + 128, S1{});
      compute_step(S0{});
      m0 += 128;
      if (m0 >= me) break;
      if (m0 + 128 < me) load_step(m0 + 128, S0{});
      compute_step(S1{});
      m0 += 128;
    }
  }
  // ---- the four waves' partial tiles through LDS: lane (fq, fr) element e of acc[en][ec] is
  //      (n = 5 (4 fq + e) + en, c = 5 fr + ec) ----
  {
    float* const mine = wsm + wave * 80 * W80_TS;
#pragma unroll
    for (int en = 0; en < 5; ++en)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float* row = mine + (5 * (4 * fq + e) + en) * W80_TS + 5 * fr;
#pragma unroll
        for (int ec = 0; ec < 5; ++ec) row[ec] = acc[en][ec][e];
      }
#pragma unroll
    for (int e = 0; e < 5; ++e) { bsum[e] += __shfl_xor(bsum[e], 16); bsum[e] += __shfl_xor(bsum[e], 32); }
    if (fq == 0) {
#pragma unroll
      for (int e = 0; e < 5; ++e) dbs[wave * 80 + 5 * fr + e] = bsum[e];
    }
  }
  __syncthreads();
  const bool do_bias = p.db != nullptr && tap == 0;
  float* const mypart = part + ((size_t)tap * ksplit + ks) * W80_PART;
  for (int idx = tid; idx < 1600; idx += 256) {           // float4 idx of the 80 x 80 tile: n = idx / 20, c = 4 (idx % 20)
    const int n = idx / 20, c4 = (idx - n * 20) * 4;
    const float* q = wsm + n * W80_TS + c4;
    const f32x4 v = (*reinterpret_cast<const f32x4*>(q) + *reinterpret_cast<const f32x4*>(q + 80 * W80_TS)) +
                    (*reinterpret_cast<const f32x4*>(q + 2 * 80 * W80_TS) + *reinterpret_cast<const f32x4*>(q + 3 * 80 * W80_TS));
    if (ksplit > 1) {
      *reinterpret_cast<f32x4*>(mypart + 4 * idx) = v;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) p.dW[((size_t)n * 80 + c4 + e) * p.ntaps + tap] += v[e] * p.alpha;
    }
  }
  if (tid < 80) {
    const float vb = (dbs[tid] + dbs[80 + tid]) + (dbs[160 + tid] + dbs[240 + tid]);
    if (ksplit > 1) mypart[6400 + tid] = vb;
    else if (do_bias) p.db[tid] += vb * p.alpha;
  }
}

// ------------------------------------------------------------------------------------------
// Weight gradient of a 3x3, stride-1, C -> C channel convolution (C <= 80: DRN-L's 160 RCAB convolutions,
// src/drn.py:143-158) with ALL NINE taps in one workgroup.  The per-tap kernels above read dY and X nine times (9 x 21 MB per
// layer at 64 px, batch 8) in workgroups of four waves that live for four row steps: 38 us at 64 px, ~130 us at 128 px.
// Here a workgroup stages a 4 x 32 pixel tile of dY and its 6 x 34 halo tile of X ONCE, as bf16, in LDS ([pixel][channel],
// the memory order).  Both MFMA operands are k-contiguous along the PIXEL axis, i.e. transposed with respect to the tiles,
// so they come out of LDS with ds_read_tr16_b64, and a tap is a constant row offset into the halo tile.  MFMA wave t of eight
// owns tap t's C x C accumulator; the ninth tap's tiles are one tile COLUMN for each of the first C / 16 waves.
// A workgroup walks `cpw` consecutive tiles, so the partial tiles (9 C^2 floats per workgroup, the cost of split-K here)
// are amortised.  Bias sums: fp32, by the staging threads.
// Versions measured on the way (80 channels, 64 / 128 px, alone on the chip; DESIGN.md 4b has the table): nine waves staging
// and computing in turns 37 / 68 us; eight waves with the next tile prefetched into registers behind the MFMAs 31.4 / 52.7 us;
// the staging on four loader waves of its own (this kernel) 29.3 / 45.3 us.
// ------------------------------------------------------------------------------------------
constexpr int WC9_TW = 32, WC9_TR = 4, WC9_PT = WC9_TW * WC9_TR, WC9_HW = WC9_TW + 2, WC9_HT = (WC9_TR + 2) * WC9_HW;
template <int NT> struct Wc9 {
  // LDS row stride (bf16): an odd multiple of 32 bytes.  A transposing read's 32 lanes (one phase of the 64 banks) then take
  // EIGHT CONSECUTIVE pixel rows x 32 bytes = every bank once; which pixel stands for which k of the MFMA is free as long as
  // dY and X agree, so lane (fq, tq) reads pixels 4 fq + tq and 16 + 4 fq + tq of a 32-pixel step.  (With pixels 8 fq + tq
  // and + 4 - the operand layout read literally - rows 0-3 and 8-11 share a phase and collide for EVERY stride that is a
  // multiple of 32 bytes: SQ_LDS_BANK_CONFLICT was 50 % of the LDS cycles, and LDS reads are what bounds this kernel.)
  static constexpr int HS = NT == 2 ? 48 : NT == 4 ? 80 : 16 * NT;
  static constexpr size_t LDS = (size_t)2 * (WC9_PT + WC9_HT) * HS * sizeof(__bf16);       // two tile buffers (>= the 4 KB bias exchange)
};

// Twelve waves: eight MFMA waves (accumulators and fragments only) and FOUR LOADER WAVES (waves 8 - 11), three per SIMD = 168
// registers each.  The loader waves hold the next-but-one tile's rows in registers (28 float4 per thread) and convert the next
// tile into the other LDS buffer WHILE the MFMA waves work on this one.  Both roles pass exactly one barrier per tile (and one
// before and one after the loop); each role has a loop of its own so that the loaders' outstanding loads never meet a join.
constexpr int WC9S_THREADS = 768, WC9S_LOADERS = 256;

// YH / XH: dY / X are bf16 arrays (DRN's bf16 training chain: the loaders move half the bytes and convert nothing; the MFMA
// operands are these bf16 values either way, only the bias sums see the rounded gradient)
template <int NT, bool YH = false, bool XH = false>
__global__ __launch_bounds__(WC9S_THREADS) void wgrad_conv9_kernel(const WgradParams p, const int cpw, const int nchunks,
                                                                    const int ksplit, float* __restrict__ part) {
  constexpr int HS = Wc9<NT>::HS, PT = WC9_PT, HT = WC9_HT, HW = WC9_HW;
  constexpr int ROWS_MIN = WC9S_LOADERS / (4 * NT);            // loader thread rows (threads / channel float4s), at least
  constexpr int NQY_MIN = ROWS_MIN / 4, NQX_MIN = ROWS_MIN / 6 < WC9_HW ? ROWS_MIN / 6 : WC9_HW;
  constexpr int NY = (WC9_TW + NQY_MIN - 1) / NQY_MIN, NX = (WC9_HW + NQX_MIN - 1) / NQX_MIN;
  static_assert(NY + NX <= 32, "item masks are one 32-bit word");
  constexpr int BUF = (PT + HT) * HS;
  typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
  extern __shared__ __attribute__((aligned(16))) float wsm[];
  const int C = p.N, c4n = C >> 2, W = p.Wo, H = p.Ho;
  __bf16* const lds0 = reinterpret_cast<__bf16*>(wsm);
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ks = blockIdx.x;
  const int c0 = ks * cpw, c_end = min(nchunks, c0 + cpw);
  const int PART = C * C + C;
  const int rows = WC9S_LOADERS / c4n, nqy = rows >> 2, nqx = min(WC9_HW, rows / 6);

  if (wave >= 8) {
    // =========================== loader waves ===========================
    const int tiles_x = W / WC9_TW;
    const int cpi = ((H + WC9_TR - 1) / WC9_TR) * tiles_x;
    // a loader thread keeps ONE channel float4 (sch) and ONE row of the tile (dY: yy of 4, X: hy of 6) and walks the row's
    // pixels with a constant stride; the roles are derived again from the thread id wherever they are used (see above)
    struct Roles { int sch, t2, yy, qy, hy, qx; };
    auto roles = [&]() __attribute__((always_inline)) -> Roles {
      int t = threadIdx.x - 512;
      asm volatile("" : "+v"(t));
      const int t2 = t / c4n;
      const int h = t2 / 6;
      return Roles{t - t2 * c4n, t2, t2 & 3, t2 >> 2, t2 - h * 6, h};
    };
    unsigned st = 0u;                                          // items that exist: bit i: x < 32, bit NY + i: hx < 34
    {
      const Roles ro = roles();
#pragma unroll
      for (int i = 0; i < NY; ++i) if (ro.qy < nqy && ro.qy + nqy * i < WC9_TW) st |= 1u << i;
#pragma unroll
      for (int i = 0; i < NX; ++i) if (ro.qx < nqx && ro.qx + nqx * i < WC9_HW) st |= 1u << (NY + i);
    }
    typedef typename std::conditional<YH, u32x2, f32x4>::type vy_t;
    typedef typename std::conditional<XH, u32x2, f32x4>::type vx_t;
    const vy_t* const dYb = reinterpret_cast<const vy_t*>(reinterpret_cast<const char*>(p.dY) + (size_t)p.ycol0 * (YH ? 2 : 4));
    const vx_t* const Xb = reinterpret_cast<const vx_t*>(p.X);
    vy_t vy[NY];
    vx_t vx[NX];
    f32x4 bsum = f32x4{0.f, 0.f, 0.f, 0.f};
    unsigned okm = 0u;
    auto issue = [&](const int chunk) __attribute__((always_inline)) {
      const int b = chunk / cpi, r = chunk - b * cpi;
      const int ty = r / tiles_x, tx = r - ty * tiles_x;
      const int y0 = ty * WC9_TR, x0 = tx * WC9_TW;
      const unsigned img = (unsigned)b * H;
      const Roles ro = roles();
      const int sch = ro.sch, qx = ro.qx;
      const int y = y0 + ro.yy, iy = y0 - 1 + ro.hy;
      okm = y < H ? (st & ((1u << NY) - 1u)) : 0u;
      const unsigned oy = ((img + min(y, H - 1)) * W + x0 + min(ro.qy, WC9_TW - 1)) * p.ldy + 4 * sch;
      unsigned sy = (unsigned)nqy * p.ldy;
      int nqx_o = nqx;
      asm volatile("" : "+v"(sy), "+v"(nqx_o));                 // per-item offsets are recomputed, not kept in registers between tiles
#pragma unroll
      for (int i = 0; i < NY; ++i) {
        const unsigned off = ((st >> i) & 1u) ? oy + i * sy : oy;
        vy[i] = dYb[off >> 2];                                   // off: elements, a multiple of 4
      }
      const unsigned rowx = (img + min(max(iy, 0), H - 1)) * W;
      const bool rok = iy >= 0 && iy < H;
#pragma unroll
      for (int i = 0; i < NX; ++i) {
        const int ix = x0 - 1 + qx + nqx_o * i;
        if (rok && (unsigned)ix < (unsigned)W) okm |= st & (1u << (NY + i));
        const unsigned off = (rowx + min(max(ix, 0), W - 1)) * p.ldx + 4 * sch;
        vx[i] = Xb[off >> 2];
      }
    };
    auto to_h4 = [](const f32x4 v) __attribute__((always_inline)) -> bf16x4 {
      bf16x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = (__bf16)v[e];
      return o;
    };
    auto store = [&](__bf16* const buf) __attribute__((always_inline)) {
      const Roles ro = roles();
      __bf16* const yrow = buf + (ro.yy * WC9_TW + ro.qy) * HS + 4 * ro.sch;
      __bf16* const xrow = buf + (PT + ro.hy * HW + ro.qx) * HS + 4 * ro.sch;
      int ysl = nqy * HS, xsl = nqx * HS;
      asm volatile("" : "+v"(ysl), "+v"(xsl));
#pragma unroll
      for (int i = 0; i < NY; ++i) {
        if constexpr (YH) {
          const u32x2 v = ((okm >> i) & 1u) ? vy[i] : u32x2{0u, 0u};
          const bf16x4 h = __builtin_bit_cast(bf16x4, v);
          bsum += f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
          if ((st >> i) & 1u) *reinterpret_cast<u32x2*>(yrow + i * ysl) = v;
        } else {
          const f32x4 v = ((okm >> i) & 1u) ? vy[i] : f32x4{0.f, 0.f, 0.f, 0.f};
          bsum += v;
          if ((st >> i) & 1u) *reinterpret_cast<bf16x4*>(yrow + i * ysl) = to_h4(v);
        }
      }
#pragma unroll
      for (int i = 0; i < NX; ++i) {
        if constexpr (XH) {
          const u32x2 v = ((okm >> (NY + i)) & 1u) ? vx[i] : u32x2{0u, 0u};
          if ((st >> (NY + i)) & 1u) *reinterpret_cast<u32x2*>(xrow + i * xsl) = v;
        } else {
          const f32x4 v = ((okm >> (NY + i)) & 1u) ? vx[i] : f32x4{0.f, 0.f, 0.f, 0.f};
          if ((st >> (NY + i)) & 1u) *reinterpret_cast<bf16x4*>(xrow + i * xsl) = to_h4(v);
        }
      }
    };
    issue(c0);
    store(lds0);
    issue(min(c0 + 1, c_end - 1));
    __syncthreads();                                           // tile c0 is in buffer 0
    for (int c = c0; c < c_end; ++c) {
      if (c + 1 < c_end) store(lds0 + (((c + 1 - c0) & 1) ? BUF : 0));
      issue(min(c + 2, c_end - 1));                            // unconditional: clamped re-reads at the end of the range
      __syncthreads();
    }
    // bias sums: one float4 per loader thread, summed over the thread rows in fixed order by the first MFMA wave
    f32x4* const bs = reinterpret_cast<f32x4*>(wsm);
    {
      const Roles ro = roles();
      if (ro.qy < nqy) bs[ro.t2 * c4n + ro.sch] = bsum;
    }
    __syncthreads();
    return;
  }

  // =========================== MFMA waves ===========================
  const int lane = tid & 63;
  const int fr = lane & 15, fq = lane >> 4, tq = fr >> 2, tp = fr & 3;
  const int ky = wave / 3, kx = wave - ky * 3;
  // the ninth tap: wave w < NT takes COLUMN w of its NT x NT MFMA tiles - the dY fragments it holds anyway and one more X
  // fragment (dealing the tiles w, w + 8, .. over all eight waves cost two fragment reads per MFMA: 16 of a wave's 36
  // transposing reads per step for 4 of its 29 MFMAs, and LDS reads are what bounds a tile)
  f32x4 acc[NT][NT], accx[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < NT; ++i) accx[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto tr8 = [&](const __bf16* r0) __attribute__((always_inline)) -> bf16x8 {
    const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(r0));
    const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(r0 + 16 * HS));
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) { o[e] = lo[e]; o[4 + e] = hi[e]; }
    return o;
  };
  __syncthreads();                                             // tile c0 is in buffer 0
  for (int c = c0; c < c_end; ++c) {
    const __bf16* const cur = lds0 + (((c - c0) & 1) ? BUF : 0);
#pragma unroll 1
    for (int s4 = 0; s4 < WC9_TR; ++s4) {
      const __bf16* const arow = cur + (s4 * 32 + 4 * fq + tq) * HS + 4 * tp;
      const __bf16* const brow = cur + (PT + (s4 + ky) * HW + kx + 4 * fq + tq) * HS + 4 * tp;
      const __bf16* const b8row = cur + (PT + (s4 + 2) * HW + 2 + 4 * fq + tq) * HS + 4 * tp;
      bf16x8 ah[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) ah[t] = tr8(arow + 16 * t);
      bf16x8 bh = tr8(brow);
#pragma unroll
      for (int ec = 0; ec < NT; ++ec) {                         // the next X fragment is in flight during this one's MFMAs
        const bf16x8 bn = tr8(ec + 1 < NT ? brow + 16 * (ec + 1) : b8row + 16 * min(wave, NT - 1));
#pragma unroll
        for (int en = 0; en < NT; ++en) acc[en][ec] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh, ah[en], acc[en][ec], 0, 0, 0);
        bh = bn;
      }
      if (wave < NT) {                                          // bh: column `wave` of the ninth tap's X fragments (a dummy read otherwise)
#pragma unroll
        for (int en = 0; en < NT; ++en) accx[en] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh, ah[en], accx[en], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  // ---- partial tiles.  The MFMAs compute the TRANSPOSED tiles (X fragment as the A operand): lane (fq, fr) holds the four
  //      consecutive input channels c = 16 ec + 4 fq + 0..3 of output channel n = 16 en + fr - one float4 of the row-major
  //      partial per tile (the other way round a lane holds four ROWS: 116 four-byte stores per lane instead of 30 float4; the
  //      launch takes the same time either way, the stores are not what its ~13 us of fixed cost are).
  //      The indices are derived again from the thread id (kept across the loop they spilled) ----
  int tid_e = threadIdx.x;
  asm volatile("" : "+v"(tid_e));
  const int fr_e = tid_e & 15, fq_e = (tid_e >> 4) & 3;
  {
    float* const mypart = part + ((size_t)wave * ksplit + ks) * PART;
#pragma unroll
    for (int en = 0; en < NT; ++en) {
      const int n = 16 * en + fr_e;
#pragma unroll
      for (int ec = 0; ec < NT; ++ec) {
        const int c = 16 * ec + 4 * fq_e;
        if (n < C && c < C) *reinterpret_cast<f32x4*>(mypart + n * C + c) = acc[en][ec];
      }
    }
    if (wave < NT) {
      float* const part8 = part + ((size_t)8 * ksplit + ks) * PART;
#pragma unroll
      for (int en = 0; en < NT; ++en) {
        const int n = 16 * en + fr_e, c = 16 * wave + 4 * fq_e;
        if (n < C && c < C) *reinterpret_cast<f32x4*>(part8 + n * C + c) = accx[en];
      }
    }
  }
  __syncthreads();                                             // the loaders' bias sums are in LDS
  if (tid_e < c4n) {
    const f32x4* const bs = reinterpret_cast<const f32x4*>(wsm);
    f32x4 t = bs[tid_e];
    for (int r = 1; r < 4 * nqy; ++r) t += bs[r * c4n + tid_e];
    *reinterpret_cast<f32x4*>(part + (size_t)ks * PART + C * C + 4 * tid_e) = t;
  }
}

template <int PREC, bool CONV>
__global__ __launch_bounds__(256) void wgrad_kernel(const WgradParams p, const int ksplit, const int tn, const int tc,
                                                    float* __restrict__ part) {
  wgrad_body<PREC, CONV>(p, ksplit, tn, tc, part, blockIdx.x);
}

// Several Linear layers' weight gradients in ONE launch (the five of a Swin block): fewer launch ramps on the side
// stream, and the layers' workgroups fill the chip together.  Each layer's block range starts at a multiple of 8 so
// the XCD mapping of wgrad_body holds.
template <int PREC, bool FULL>
__global__ __launch_bounds__(256, FULL ? 2 : 1) void wgrad_multi_kernel(const WgradMulti mp) {
  int i = 0;
#pragma unroll
  for (int k = 1; k < SRAD_WGRAD_MULTI; ++k)
    if (k < mp.count && (int)blockIdx.x >= mp.blk0[k]) i = k;
  const int L = blockIdx.x - mp.blk0[i];
  if (L >= mp.nblk[i]) return;                       // padding blocks between layers
  if constexpr (PREC == SRAD_PREC_BF16) {
    // operand storage is per layer (the adjust conv's gradient operands stay fp32): workgroup-uniform branch
    if (mp.p[i].x_bf16 && mp.p[i].dy_bf16) { wgrad_body<PREC, false, FULL, true, true>(mp.p[i], mp.ksplit[i], mp.tn[i], mp.tc[i], mp.part[i], L); return; }
    if (mp.p[i].x_bf16) { wgrad_body<PREC, false, FULL, true, false>(mp.p[i], mp.ksplit[i], mp.tn[i], mp.tc[i], mp.part[i], L); return; }
  }
  wgrad_body<PREC, false, FULL>(mp.p[i], mp.ksplit[i], mp.tn[i], mp.tc[i], mp.part[i], L);
}

// The same for a launch whose layers ALL have both operands stored as bf16 (the training step's blocks 1-4 of every RDG):
// only that body, so the kernel's register allocation is that body's, and with the two-slot cross-wave sum (36 KB of LDS)
// four workgroups fit a CU: with ONE register set of operand rows it needs 128 VGPRs (four waves per SIMD cover each other's loads).
__global__ __launch_bounds__(256, 4) void wgrad_multi_hh_kernel(const WgradMulti mp) {
  int i = 0;
#pragma unroll
  for (int k = 1; k < SRAD_WGRAD_MULTI; ++k)
    if (k < mp.count && (int)blockIdx.x >= mp.blk0[k]) i = k;
  const int L = blockIdx.x - mp.blk0[i];
  if (L >= mp.nblk[i]) return;
  wgrad_body<SRAD_PREC_BF16, false, true, true, true, true, false>(mp.p[i], mp.ksplit[i], mp.tn[i], mp.tc[i], mp.part[i], L);
}

// One workgroup per QUARTER of a 64 x 64 output tile of one of the batch's layers (16 rows n, one float4 per
// thread): dW += alpha * sum_k partial[k], k in fixed order.
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const WgradReduceBatch b) {
  const int gt = blockIdx.x >> 2, quarter = blockIdx.x & 3;
  int it = 0;
#pragma unroll
  for (int i = 1; i < SRAD_WGRAD_BATCH; ++i)
    if (i < b.count && gt >= b.it[i].tile0) it = i;
  const WgradReduceItem& d = b.it[it];
  const int tile_id = gt - d.tile0;
  if (d.ntaps == 0) {
    // column sums: dst[c] += sum_k part[k * cin_real + c], c < n_real (LayerNorm dgamma / dbeta, bias-table
    // gradient); 16 columns per workgroup, 16 row phases per column
    __shared__ float red[16][17];
    const int r = threadIdx.x >> 4, cl = threadIdx.x & 15;
    const int col = (tile_id * 4 + quarter) * 16 + cl;
    const int cc = min(col, d.n_real - 1);
    float sum = 0.f;
    int k = r;
    for (; k + 112 < d.ksplit; k += 128) {                      // 8 loads in flight (512 partial rows of a LayerNorm: 32 loads per thread)
      float t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = d.part[(size_t)(k + 16 * u) * d.cin_real + cc];
#pragma unroll
      for (int u = 0; u < 8; ++u) sum += t[u];
    }
    for (; k < d.ksplit; k += 16) sum += d.part[(size_t)k * d.cin_real + cc];
    red[r][cl] = sum;
    __syncthreads();
    if (threadIdx.x < 16 && col < d.n_real) {
      float t = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) t += red[i][cl];
      d.dW[col] += t * d.alpha;
    }
    return;
  }
  if (d.wc) {
    // one wc x wc tile per tap (wgrad80_kernel, wgrad_conv9_kernel): row-major + wc bias sums per partial.  d.tn reduce
    // "tiles" (x 4 workgroups) per tap, d.tc float4 of the tile per workgroup (32 x 50 for 80 channels); the split-K partials
    // are dealt over four thread groups and combined in fixed order.  Lanes d.tc and d.tc + 1 of the tap-0 workgroups take a
    // float4 of the bias sums each.  (Four workgroups per tap - 36 for a whole 3x3 layer - with one thread group and 80 threads
    // walking the bias sums took 36 us for 15 MB: 3.2 ms of a DRN-L training step's side stream.)
    __shared__ f32x4 ph[4][64];
    const int C = d.wc, cc4 = C * C / 4, c4n = C / 4, per = d.tc;
    const int PART = C * C + C;
    const int tap = tile_id / d.tn, sub = (tile_id - tap * d.tn) * 4 + quarter;
    const float* const tb = d.part + (size_t)tap * d.ksplit * PART;
    const int il = threadIdx.x & 63, phase = threadIdx.x >> 6;
    const int bidx = sub * 2 + (il - per);                       // bias float4 of lanes per, per + 1
    const bool is_w = il < per && sub * per + il < cc4;
    const bool is_b = il >= per && il < per + 2 && tap == 0 && bidx < c4n && d.db != nullptr;
    const int idx = is_w ? sub * per + il : (is_b ? cc4 + bidx : 0);
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    int k = phase;
    for (; k + 28 < d.ksplit; k += 32) {                        // 8 loads in flight
      f32x4 t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = *reinterpret_cast<const f32x4*>(tb + (size_t)(k + 4 * u) * PART + 4 * idx);
#pragma unroll
      for (int u = 0; u < 8; ++u) v += t[u];
    }
    for (; k < d.ksplit; k += 4) v += *reinterpret_cast<const f32x4*>(tb + (size_t)k * PART + 4 * idx);
    ph[phase][il] = v;
    __syncthreads();
    if (threadIdx.x < 64 && (is_w || is_b)) {
      const f32x4 t = (ph[0][il] + ph[1][il]) + (ph[2][il] + ph[3][il]);
      if (is_w) {
        const int n = idx / c4n, c0 = (idx - n * c4n) * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) d.dW[((size_t)n * C + c0 + e) * d.ntaps + tap] += t[e] * d.alpha;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) d.db[4 * bidx + e] += t[e] * d.alpha;
      }
    }
    return;
  }
  const int nx = tile_id % d.tn, cy = (tile_id / d.tn) % d.tc, tap = tile_id / (d.tn * d.tc);
  const int tid = threadIdx.x;
  const int e4 = quarter * 256 + tid;
  const float* const base = d.part + (size_t)tile_id * d.ksplit * WG_TS + 4 * e4;
  f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
  int k = 0;
  for (; k + 8 <= d.ksplit; k += 8) {                          // 8 loads in flight
    f32x4 t[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) t[u] = *reinterpret_cast<const f32x4*>(base + (size_t)(k + u) * WG_TS);
#pragma unroll
    for (int u = 0; u < 8; ++u) v += t[u];
  }
  for (; k < d.ksplit; ++k) v += *reinterpret_cast<const f32x4*>(base + (size_t)k * WG_TS);
  const int n0 = nx * 64, c0 = cy * 64;
  const int n = n0 + (e4 >> 4), cl = (e4 & 15) * 4;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int c = srad_real_channel(c0 + cl + e, d.grp_real, d.grp_pad, d.cin_real);
    if (n < d.n_real && c < d.cin_real) {
      float* dst = d.dW + ((size_t)n * d.cin_real + c) * d.ntaps + tap;
      *dst += v[e] * d.alpha;
    }
  }
  if (d.db != nullptr && cy == 0 && tap == 0 && tid < 16 && n0 + quarter * 16 + tid < d.n_real) {
    const float* bb = d.part + (size_t)tile_id * d.ksplit * WG_TS + 4096 + quarter * 16 + tid;
    float vb = 0.f;
    int kk = 0;
    for (; kk + 8 <= d.ksplit; kk += 8) {                      // 8 loads in flight (one after the other they were the launch's tail)
      float t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = bb[(size_t)(kk + u) * WG_TS];
#pragma unroll
      for (int u = 0; u < 8; ++u) vb += t[u];
    }
    for (; kk < d.ksplit; ++kk) vb += bb[(size_t)kk * WG_TS];
    d.db[n0 + quarter * 16 + tid] += vb * d.alpha;
  }
}

// ------------------------------------------------------------------------------------------
// The queue's launch.  wgrad_queue.h decides what is reduced and where a region goes; here are its "reduce this batch now"
// and the texts of its refusals.
// ------------------------------------------------------------------------------------------
int launch_reduce(const WgradQueue& q, const WgradReduceBatch& b, int tiles, hipStream_t stream) {
  SradProfScope prof(stream, SRAD_K_WGRAD_REDUCE, 0.0, 4.0 * q.used);
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(4 * tiles), dim3(256), 0, stream, b);
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

// The one place workspace is handed out (wgrad_queue_reserve): `need` floats (*r) and room for `nitems` more batch entries, after
// a flush if the batch or the workspace is full; fails with an error naming `who` if the region does not fit even then.
int take(WgradQueue& q, const char* who, size_t need, int nitems, hipStream_t stream, WgradRegion* r) {
  const hipStream_t fs = wgrad_queue_pending_layers(q) > 0 && q.own_flush_stream ? q.flush_stream : stream;
  const int rc = wgrad_queue_reserve(q, need, nitems, [&](const WgradReduceBatch& b, int tiles, int) { return launch_reduce(q, b, tiles, fs); }, r);
  switch (rc) {
    case SRAD_WGRAD_TOO_SMALL:
      return srad_set_error(SRAD_ERR_ARG, "%s: split-K workspace too small (%zu floats needed, %zu given)", who, need, q.ws_floats);
    case SRAD_WGRAD_BAD_NITEMS: return srad_set_error(SRAD_ERR_ARG, "%s: %d items in one reservation", who, nitems);
    case SRAD_WGRAD_NO_ROOM:
      return srad_set_error(SRAD_ERR_ARG, "%s: split-K workspace too small next to the deferred layers (%zu floats needed, %zu given, %d layers pending)",
                            who, need, q.ws_floats, wgrad_queue_pending_layers(q));
    default: return rc;
  }
}

constexpr size_t WG_LDS = (size_t)(4 * 64 * 68 + 4 * 64) * sizeof(float);
constexpr size_t WG_LDS2 = (size_t)(2 * 64 * 68 + 4 * 64) * sizeof(float);   // wgrad_body<.., LDS2 = true>

// ------------------------------------------------------------------------------------------
// Decide first, launch second.  Which kernel a layer takes, its tiles, row splits, grid, partial-tile workspace and reduce
// tiles are fixed here from the parameters alone, on the host; the launchers below carry a decision out and srad_plan_wgrad*
// report it (include/srad.h srad_wgrad_plan) - the same functions, so a plan cannot drift from the launch.
// ------------------------------------------------------------------------------------------
struct WgradDecision {
  int family = SRAD_WGRAD_FAM_TILE64;   // SRAD_WGRAD_FAM_TILE64 | W80 | CONV9 (a shared launch's family is decided per launch: decide_multi)
  bool conv = false;                // tile64 / w80: the row-gather variant of the kernel
  int tn = 1, tc = 1;               // tile64: 64-wide tiles along N / Cin
  long tiles = 0;                   // output tiles: tn tc ntaps (tile64), ntaps (w80), 9 (conv9)
  int ksplit = 1, rows_per = 0;     // row splits and rows of one (conv9: workgroups; its ranges are cpw chunks, not rows)
  int grid = 0;                     // workgroups of the layer
  int nt = 0, cpw = 0, nchunks = 0; // conv9: 16-channel sub-tiles, 4 x 32 pixel chunks per workgroup, chunks in all
  size_t need = 0;                  // floats of partial tiles in the queue's workspace; 0: the kernel adds into dW / db itself
  int wc = 0, rtn = 0, rtc = 0;     // the reduce item's geometry (WgradReduceItem wc, tn, tc)
  int reduce_tiles = 0;             // reduce tiles the layer adds to the queue
};

// 64 x 64 tiles: about two workgroups per CU for a launch of its own (wg_target 512; layers that share a launch ask for fewer,
// longer workgroups: less ramp, fewer partial tiles)
template <int PREC>
WgradDecision decide_tile64(const WgradParams& p, const long wg_target) {
  constexpr int KR = PREC == SRAD_PREC_BF16 ? 32 : 4;
  WgradDecision d;
  d.family = SRAD_WGRAD_FAM_TILE64;
  d.conv = p.ntaps == 9 || p.stride != 1;
  d.tn = (p.N + 63) / 64; d.tc = (p.Cin + 63) / 64;
  d.tiles = (long)d.tn * d.tc * p.ntaps;
  d.ksplit = srad_wgrad_split_count<4 * KR>(p.M, d.tiles, wg_target);
  d.rows_per = srad_wgrad_rows_per<4 * KR>(p.M, d.ksplit);
  d.grid = (int)(d.tiles * d.ksplit);
  if (d.ksplit > 1) {
    d.need = (size_t)d.tiles * d.ksplit * WG_TS;
    d.rtn = d.tn; d.rtc = d.tc; d.reduce_tiles = (int)d.tiles;
  }
  return d;
}

// reduce geometry of a layer whose partials are one C x C tile per tap (see wgrad_reduce_kernel)
static void square_reduce_tiles(WgradDecision& d, const int C, const int ntaps) {
  const int cc4 = C * C / 4;
  d.wc = C;
  d.rtn = (cc4 + 199) / 200;                      // x 4 workgroups per tap, <= 50 float4 each
  d.rtc = (cc4 + 4 * d.rtn - 1) / (4 * d.rtn);
  d.reduce_tiles = ntaps * d.rtn;
}

// 80 -> 80 channels, stride 1, bf16: one 80 x 80 tile per tap
static bool wgrad80_supported(const WgradParams& p) {
  return p.N == 80 && p.Cin == 80 && p.n_real == 80 && p.cin_real == 80 && p.stride == 1 && !p.row_scale &&
         (p.ntaps == 1 || (p.Hi == p.Ho && p.Wi == p.Wo));
}

WgradDecision decide_wgrad80(const WgradParams& p) {
  WgradDecision d;
  d.family = SRAD_WGRAD_FAM_W80;
  d.conv = p.ntaps == 9;
  d.tn = d.tc = 1; d.tiles = p.ntaps;
  d.ksplit = srad_wgrad_split_count<128>(p.M, p.ntaps, 512);       // about two workgroups per CU
  d.rows_per = srad_wgrad_rows_per<128>(p.M, d.ksplit);
  d.grid = p.ntaps * d.ksplit;
  if (d.ksplit > 1) {
    d.need = (size_t)p.ntaps * d.ksplit * W80_PART;
    square_reduce_tiles(d, 80, p.ntaps);
  }
  return d;
}

// 3x3 stride-1 C -> C convolution, all nine taps per workgroup (wgrad_conv9_kernel); false: not this layer's kernel
static bool conv9_supported(const WgradParams& p) {
  if (p.ntaps != 9 || p.stride != 1 || p.N != p.Cin || p.n_real != p.N || p.cin_real != p.Cin || p.N > 80 || (p.N & 3) || p.row_scale ||
      ((p.x_bf16 || p.dy_bf16) && !(p.N == 80 && p.dy_bf16)) || p.Hi != p.Ho || p.Wi != p.Wo || (p.Wo % WC9_TW) || (p.ldy & 3) || (p.ldx & 3) || (p.ycol0 & 3) ||
      (size_t)p.M < 8192 || (size_t)p.M * (size_t)std::max(p.ldy, p.ldx) >= ((size_t)1 << 31))
    return false;
  return ((reinterpret_cast<uintptr_t>(p.dY) | reinterpret_cast<uintptr_t>(p.X)) & 15) == 0;
}

WgradDecision decide_wgrad_conv9(const WgradParams& p) {
  WgradDecision d;
  d.family = SRAD_WGRAD_FAM_CONV9;
  d.conv = true;
  const int C = p.N;
  d.nt = p.dy_bf16 ? 5 : std::min(5, (C + 15) / 16);          // bf16 operands: 80 channels only (conv9_supported)
  d.tn = d.tc = 1; d.tiles = 9;
  const int B = p.M / (p.Ho * p.Wo);
  d.nchunks = B * ((p.Ho + WC9_TR - 1) / WC9_TR) * (p.Wo / WC9_TW);
  // workgroups: a 128-pixel tile costs ~2 us, a workgroup ~6 us of ramp plus its partial tiles (9 C^2 floats written and
  // read again): ~4 sqrt(tiles) workgroups balance the two (64 for 256 tiles, 128 for 1024)
  int ksplit = (int)(4.0 * sqrt((double)d.nchunks) + 0.5);
  ksplit = std::max(1, std::min(std::min(ksplit, 256), d.nchunks));
  d.cpw = (d.nchunks + ksplit - 1) / ksplit;
  d.ksplit = (d.nchunks + d.cpw - 1) / d.cpw;
  d.rows_per = d.cpw * WC9_PT;
  d.grid = d.ksplit;
  d.need = 9 * (size_t)d.ksplit * ((size_t)C * C + C);         // always through the reduce kernel
  square_reduce_tiles(d, C, 9);
  return d;
}

// the kernel family of an immediate layer
template <int PREC>
WgradDecision decide_wgrad(const WgradParams& p) {
  if (PREC == SRAD_PREC_BF16 && conv9_supported(p)) return decide_wgrad_conv9(p);
  if (PREC == SRAD_PREC_BF16 && wgrad80_supported(p)) return decide_wgrad80(p);
  return decide_tile64<PREC>(p, 512);
}

// the decision's partial-tile workspace (*part; null: none) and its entry in the reduce batch (pending: a deferred layer's)
int queue_partials(const WgradParams& p, const WgradDecision& d, const char* who, WgradQueue& q, hipStream_t s, const bool pending,
                   float** part) {
  *part = nullptr;
  if (d.need == 0) return SRAD_OK;
  WgradRegion r;
  SRAD_TRY(take(q, who, d.need, 1, s, &r));
  *part = q.ws + r.off;
  WgradReduceItem it{};
  it.dW = p.dW; it.db = p.db; it.part = *part; it.n_real = p.n_real; it.cin_real = p.cin_real; it.ntaps = p.ntaps;
  it.grp_real = d.wc ? 0 : p.grp_real; it.grp_pad = d.wc ? 0 : p.grp_pad;
  it.tn = d.rtn; it.tc = d.rtc; it.ksplit = d.ksplit; it.alpha = p.alpha; it.wc = d.wc;
  wgrad_queue_push(q, it, d.reduce_tiles, r, pending);
  return SRAD_OK;
}

int launch_wgrad80(const WgradParams& p, const WgradDecision& d, WgradQueue& q, hipStream_t s) {
  float* part;
  SRAD_TRY(queue_partials(p, d, "wgrad80", q, s, false, &part));
  SradProfScope prof(s, SRAD_K_WGRAD, 2.0 * p.M * 80.0 * 80.0 * p.ntaps, 4.0 * p.M * 160.0 + 8.0 * 6400.0 * p.ntaps);
  const dim3 grid((unsigned)d.grid);
  SRAD_TRY(d.conv ? srad_launch_dyn<wgrad80_kernel<true>>(grid, dim3(256), W80_LDS, s, p, d.ksplit, part)
                  : srad_launch_dyn<wgrad80_kernel<false>>(grid, dim3(256), W80_LDS, s, p, d.ksplit, part));
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

int launch_wgrad_conv9(const WgradParams& p, const WgradDecision& d, WgradQueue& q, hipStream_t s) {
  const int C = p.N, cpw = d.cpw, nchunks = d.nchunks, ksplit = d.ksplit;
  float* part;
  SRAD_TRY(queue_partials(p, d, "wgrad_conv9", q, s, false, &part));
  SradProfScope prof(s, SRAD_K_WGRAD, 2.0 * p.M * C * C * 9.0,
                     (double)p.M * C * ((p.dy_bf16 ? 2 : 4) + (p.x_bf16 ? 2 : 4)) + 8.0 * 9.0 * ((double)C * C + C) * ksplit);
  const dim3 grid((unsigned)d.grid), block(WC9S_THREADS);
  int rc;
  if (p.dy_bf16)                                                // 80 channels only (conv9_supported): DRN's bf16 training chain
    rc = p.x_bf16 ? srad_launch_dyn<wgrad_conv9_kernel<5, true, true>>(grid, block, Wc9<5>::LDS, s, p, cpw, nchunks, ksplit, part)
                  : srad_launch_dyn<wgrad_conv9_kernel<5, true, false>>(grid, block, Wc9<5>::LDS, s, p, cpw, nchunks, ksplit, part);
  else switch (d.nt) {
    case 1: rc = srad_launch_dyn<wgrad_conv9_kernel<1>>(grid, block, Wc9<1>::LDS, s, p, cpw, nchunks, ksplit, part); break;
    case 2: rc = srad_launch_dyn<wgrad_conv9_kernel<2>>(grid, block, Wc9<2>::LDS, s, p, cpw, nchunks, ksplit, part); break;
    case 3: rc = srad_launch_dyn<wgrad_conv9_kernel<3>>(grid, block, Wc9<3>::LDS, s, p, cpw, nchunks, ksplit, part); break;
    case 4: rc = srad_launch_dyn<wgrad_conv9_kernel<4>>(grid, block, Wc9<4>::LDS, s, p, cpw, nchunks, ksplit, part); break;
    default: rc = srad_launch_dyn<wgrad_conv9_kernel<5>>(grid, block, Wc9<5>::LDS, s, p, cpw, nchunks, ksplit, part); break;
  }
  if (rc) return rc;
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

template <int PREC>
int launch_wgrad(const WgradParams& p, WgradQueue& q, hipStream_t s) {
  const WgradDecision d = decide_wgrad<PREC>(p);
  if (d.family == SRAD_WGRAD_FAM_CONV9) return launch_wgrad_conv9(p, d, q, s);
  if (d.family == SRAD_WGRAD_FAM_W80) return launch_wgrad80(p, d, q, s);
  float* part;
  SRAD_TRY(queue_partials(p, d, "wgrad", q, s, false, &part));
  const dim3 grid((unsigned)d.grid);
  const double K = (double)p.ntaps * p.cin_real;
  SradProfScope prof(s, SRAD_K_WGRAD, 2.0 * p.M * p.n_real * K, 4.0 * p.M * ((double)p.N + p.Cin) + 8.0 * p.n_real * K);
  SRAD_TRY((d.conv ? srad_launch_dyn<wgrad_kernel<PREC, true>>(grid, dim3(256), WG_LDS, s, p, d.ksplit, d.tn, d.tc, part)
                  : srad_launch_dyn<wgrad_kernel<PREC, false>>(grid, dim3(256), WG_LDS, s, p, d.ksplit, d.tn, d.tc, part)));
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

// ---- the shared launch of up to SRAD_WGRAD_MULTI Linear layers ----
// a deferred layer's tiles and splits: the launch is shared, so each layer asks for fewer, longer workgroups
template <int PREC>
WgradDecision decide_deferred(const WgradParams& p) { return decide_tile64<PREC>(p, 144); }

// slot i of the shared launch: the layer's block range starts at a multiple of 8 (the XCD mapping of wgrad_body)
void multi_put(WgradMulti& m, const int i, const WgradParams& p, const WgradDecision& d, float* part) {
  m.p[i] = p; m.ksplit[i] = d.ksplit; m.tn[i] = d.tn; m.tc[i] = d.tc; m.part[i] = part;
  m.blk0[i] = i == 0 ? 0 : (m.blk0[i - 1] + m.nblk[i - 1] + 7) / 8 * 8;
  m.nblk[i] = d.grid;
}

// which kernel sends the layers of m, and with how many workgroups
struct MultiDecision { int family; bool full; int grid; };
int decide_multi(const int prec, const WgradMulti& m, MultiDecision& md) {
  bool full = prec == SRAD_PREC_BF16;            // every layer: whole 128-row steps, DropPath factor constant per wave step
  for (int i = 0; i < m.count && full; ++i) {
    const long rows_per = srad_wgrad_rows_per<128>(m.p[i].M, m.ksplit[i]);
    full = rows_per * m.ksplit[i] == m.p[i].M && (!m.p[i].row_scale || m.p[i].rps % 32 == 0);
  }
  for (int i = 0; i < m.count; ++i)
    SRAD_REQUIRE(!(m.p[i].x_bf16 || m.p[i].dy_bf16) || (prec == SRAD_PREC_BF16 && (!m.p[i].dy_bf16 || m.p[i].x_bf16)),
                 "wgrad: bf16 operand storage needs the bf16 MFMA path, dY only together with X");
  bool all_hh = full;                                // every layer with both operands as bf16: the lean kernel
  for (int i = 0; i < m.count && all_hh; ++i) all_hh = m.p[i].x_bf16 && m.p[i].dy_bf16;
  md.family = all_hh ? SRAD_WGRAD_FAM_MULTI_HH : SRAD_WGRAD_FAM_MULTI;
  md.full = full;
  md.grid = m.blk0[m.count - 1] + m.nblk[m.count - 1];
  return SRAD_OK;
}

template <int PREC>
int defer_wgrad(const WgradParams& p, WgradQueue& q, hipStream_t s) {
  SRAD_REQUIRE(p.ntaps == 1 && p.stride == 1, "wgrad: only Linear layers can be deferred");
  if (q.multi.count == SRAD_WGRAD_MULTI) SRAD_TRY(srad_wgrad_launch_deferred(PREC, q, s));
  const WgradDecision d = decide_deferred<PREC>(p);
  float* part;
  SRAD_TRY(queue_partials(p, d, "wgrad", q, s, true, &part));      // the item is pending until the shared launch goes out
  multi_put(q.multi, wgrad_queue_defer_slot(q), p, d, part);
  q.multi_flops += 2.0 * p.M * p.n_real * (double)p.cin_real;
  q.multi_bytes += 4.0 * p.M * ((double)p.N + p.Cin) + 8.0 * p.n_real * (double)p.cin_real;
  return SRAD_OK;
}

// one layer's entries of a plan
void plan_layer(srad_wgrad_plan& pl, const int i, const int launch, const WgradParams& p, const WgradDecision& d) {
  pl.launch[i] = launch; pl.ksplit[i] = d.ksplit; pl.rows_per[i] = d.rows_per; pl.tn[i] = d.tn; pl.tc[i] = d.tc;
  pl.XH[i] = p.x_bf16 ? 1 : 0; pl.YH[i] = p.dy_bf16 ? 1 : 0;
  pl.nblk[i] = d.grid;
  pl.reduce_tiles += d.reduce_tiles;
}

}  // namespace

int srad_wgrad_flush(WgradQueue& q, hipStream_t stream) {
  return wgrad_queue_flush(q, SRAD_WGRAD_FLUSH_EXPLICIT, [&](const WgradReduceBatch& b, int tiles, int) { return launch_reduce(q, b, tiles, stream); });
}

int srad_wgrad_take(WgradQueue& q, const char* who, size_t need, int nitems, hipStream_t stream, float** part) {
  WgradRegion r;
  SRAD_TRY(take(q, who, need, nitems, stream, &r));
  *part = q.ws + r.off;
  return SRAD_OK;
}

static int check_wgrad(const WgradParams& p);
static int check_wgrad_storage(int prec, const WgradParams& p);

int srad_launch_wgrad_deferred(int prec, const WgradParams& p, WgradQueue& q, hipStream_t stream) {
  SRAD_TRY(check_wgrad(p));
  return prec == SRAD_PREC_BF16 ? defer_wgrad<SRAD_PREC_BF16>(p, q, stream) : defer_wgrad<SRAD_PREC_F32>(p, q, stream);
}

int srad_wgrad_launch_deferred(int prec, WgradQueue& q, hipStream_t stream) {
  WgradMulti& m = q.multi;
  if (m.count == 0) return SRAD_OK;
  MultiDecision md;
  SRAD_TRY(decide_multi(prec, m, md));
  {
    SradProfScope prof(stream, SRAD_K_WGRAD, q.multi_flops, q.multi_bytes);
    const dim3 grid(md.grid), block(256);
    SRAD_TRY((md.family == SRAD_WGRAD_FAM_MULTI_HH ? srad_launch_dyn<wgrad_multi_hh_kernel>(grid, block, WG_LDS2, stream, m)
             : prec != SRAD_PREC_BF16         ? srad_launch_dyn<wgrad_multi_kernel<SRAD_PREC_F32, false>>(grid, block, WG_LDS, stream, m)
             : md.full                        ? srad_launch_dyn<wgrad_multi_kernel<SRAD_PREC_BF16, true>>(grid, block, WG_LDS, stream, m)
                                              : srad_launch_dyn<wgrad_multi_kernel<SRAD_PREC_BF16, false>>(grid, block, WG_LDS, stream, m)));
    SRAD_CHECK_HIP(hipGetLastError());
  }
  wgrad_queue_deferred_launched(q);
  return SRAD_OK;
}

static int check_wgrad(const WgradParams& p) {
  SRAD_REQUIRE(p.M > 0 && p.N > 0 && p.Cin > 0 && p.dW, "wgrad: empty problem M=%d N=%d Cin=%d", p.M, p.N, p.Cin);
  SRAD_REQUIRE((p.N & 3) == 0 && (p.Cin & 3) == 0 && (p.ldy & 3) == 0 && (p.ldx & 3) == 0 && (p.ycol0 & 3) == 0 &&
                   ((uintptr_t)p.dY & 15) == 0 && ((uintptr_t)p.X & 15) == 0,
               "wgrad: operands need channel counts / strides that are multiples of 4 floats (N=%d Cin=%d ldy=%d ldx=%d)", p.N, p.Cin, p.ldy, p.ldx);
  SRAD_REQUIRE(p.n_real > 0 && p.n_real <= p.N && p.cin_real > 0 && p.cin_real <= p.Cin, "wgrad: bad real extents");
  SRAD_REQUIRE(p.grp_pad == 0 || (p.grp_real > 0 && p.grp_real <= p.grp_pad && p.cin_real % p.grp_real == 0 &&
                                  (p.cin_real / p.grp_real) * p.grp_pad <= p.Cin), "wgrad: bad channel groups %d -> %d", p.grp_real, p.grp_pad);
  SRAD_REQUIRE(p.ntaps == 1 || p.ntaps == 9, "wgrad: ntaps must be 1 or 9");
  if (p.ntaps == 9 || p.stride != 1)
    SRAD_REQUIRE(p.Ho > 0 && p.Wo > 0 && p.Hi > 0 && p.Wi > 0 && p.M % (p.Ho * p.Wo) == 0, "wgrad: bad conv geometry");
  SRAD_REQUIRE(!p.row_scale || p.rps > 0, "wgrad: row_scale needs rows-per-sample");
  return SRAD_OK;
}

bool srad_wgrad_conv9_supported(const WgradParams& p) { return conv9_supported(p); }

int srad_launch_wgrad(int prec, const WgradParams& p, WgradQueue& q, hipStream_t stream) {
  SRAD_TRY(check_wgrad(p));
  SRAD_TRY(check_wgrad_storage(prec, p));
  return prec == SRAD_PREC_BF16 ? launch_wgrad<SRAD_PREC_BF16>(p, q, stream) : launch_wgrad<SRAD_PREC_F32>(p, q, stream);
}

static int check_wgrad_storage(int prec, const WgradParams& p) {
  SRAD_REQUIRE((!p.x_bf16 && !p.dy_bf16) || (prec == SRAD_PREC_BF16 && conv9_supported(p)),
               "wgrad: bf16 operand storage is for deferred Linear layers and the nine-tap 80-channel convolution kernel only");
  return SRAD_OK;
}

// What srad_launch_wgrad would launch for p: its own checks and its own decision, nothing launched or reserved.
int srad_plan_wgrad(int prec, const WgradParams& p, srad_wgrad_plan* plan) {
  SRAD_REQUIRE(plan, "wgrad plan: null argument");
  SRAD_TRY(check_wgrad(p));
  SRAD_TRY(check_wgrad_storage(prec, p));
  const WgradDecision d = prec == SRAD_PREC_BF16 ? decide_wgrad<SRAD_PREC_BF16>(p) : decide_wgrad<SRAD_PREC_F32>(p);
  srad_wgrad_plan pl{};
  pl.count = 1; pl.launches = 1;
  pl.precision = prec == SRAD_PREC_BF16 ? SRAD_PREC_BF16 : SRAD_PREC_F32;
  pl.family[0] = d.family; pl.grid[0] = d.grid; pl.CONV = d.conv ? 1 : 0;
  pl.NT = d.nt; pl.cpw = d.cpw; pl.nchunks = d.nchunks;
  plan_layer(pl, 0, 0, p, d);
  *plan = pl;
  return SRAD_OK;
}

// The same for `count` layers given to srad_launch_wgrad_deferred one after the other and then sent (srad_wgrad_launch_deferred):
// a layer that finds SRAD_WGRAD_MULTI waiting sends them first, so up to SRAD_WGRAD_MULTI + 1 layers make two launches.
int srad_plan_wgrad_deferred(int prec, const WgradParams* layers, int count, srad_wgrad_plan* plan) {
  SRAD_REQUIRE(plan && layers, "wgrad plan: null argument");
  SRAD_REQUIRE(count > 0 && count <= SRAD_WGRAD_PLAN_LAYERS, "wgrad plan: 1 to %d deferred layers, not %d", SRAD_WGRAD_PLAN_LAYERS, count);
  srad_wgrad_plan pl{};
  pl.count = count;
  pl.precision = prec == SRAD_PREC_BF16 ? SRAD_PREC_BF16 : SRAD_PREC_F32;
  WgradMulti m{};
  auto send = [&]() -> int {
    MultiDecision md;
    SRAD_TRY(decide_multi(prec, m, md));
    pl.family[pl.launches] = md.family; pl.FULL[pl.launches] = md.full ? 1 : 0; pl.grid[pl.launches] = md.grid;
    ++pl.launches;
    m.count = 0;
    return SRAD_OK;
  };
  for (int i = 0; i < count; ++i) {
    const WgradParams& p = layers[i];
    SRAD_TRY(check_wgrad(p));
    SRAD_REQUIRE(p.ntaps == 1 && p.stride == 1, "wgrad: only Linear layers can be deferred");
    if (m.count == SRAD_WGRAD_MULTI) SRAD_TRY(send());
    const WgradDecision d = prec == SRAD_PREC_BF16 ? decide_deferred<SRAD_PREC_BF16>(p) : decide_deferred<SRAD_PREC_F32>(p);
    const int slot = m.count++;
    multi_put(m, slot, p, d, nullptr);
    plan_layer(pl, i, pl.launches, p, d);
    pl.blk0[i] = m.blk0[slot];
  }
  SRAD_TRY(send());
  *plan = pl;
  return SRAD_OK;
}

// queues alpha times the column sums of `rows` partial rows at `part` (inside r, whose reservation made room for the item)
static int queue_colsum(WgradQueue& q, float* dst, const float* part, const WgradRegion& r, int ncols, int row_stride, int rows, float alpha) {
  SRAD_REQUIRE(q.batch.count < SRAD_WGRAD_BATCH, "wgrad: a column sum was queued without room reserved for it");   // the rows are taken: no flush here
  WgradReduceItem it{};
  it.dW = dst; it.db = nullptr; it.part = part; it.n_real = ncols; it.cin_real = row_stride; it.ntaps = 0; it.grp_real = it.grp_pad = 0;   // ntaps 0: column sums
  it.tn = it.tc = 1; it.ksplit = rows; it.alpha = alpha; it.wc = 0;
  wgrad_queue_push(q, it, (ncols + 63) / 64, r);
  return SRAD_OK;
}

static int reserve_colsum(WgradQueue& q, const char* who, float* dst, int ncols, int row_stride, int nrows, float alpha, int nitems,
                          hipStream_t stream, WgradRegion* r) {
  SRAD_TRY(take(q, who, (size_t)nrows * row_stride, nitems, stream, r));
  if (dst) SRAD_TRY(queue_colsum(q, dst, q.ws + r->off, *r, ncols, row_stride, nrows, alpha));
  return SRAD_OK;
}

int srad_wgrad_reserve_colsum(WgradQueue& q, const char* who, float* dst, int ncols, int row_stride, int nrows, float alpha,
                              int nitems, hipStream_t stream, float** part) {
  WgradRegion r;
  SRAD_TRY(reserve_colsum(q, who, dst, ncols, row_stride, nrows, alpha, nitems, stream, &r));
  *part = q.ws + r.off;
  return SRAD_OK;
}

int srad_wgrad_queue_ln_partials(WgradQueue& q, float* dgamma, float* dbeta, int C, int nrows, hipStream_t stream, float** part) {
  WgradRegion r;
  SRAD_TRY(reserve_colsum(q, "ln_bwd", dgamma, C, 2 * SRAD_LNB_CP, nrows, 1.f, 2, stream, &r));
  *part = q.ws + r.off;
  if (dbeta) SRAD_TRY(queue_colsum(q, dbeta, *part + SRAD_LNB_CP, r, C, 2 * SRAD_LNB_CP, nrows, 1.f));
  return SRAD_OK;
}
