// swin_tiles.h - what the Swin forward kernels share: mlp_block_kernel (kernels_fused.hip), qkv_attn_kernel and ln_qkv_kernel
// (kernels_fused_attn.hip) and swin_block_kernel (kernels_fused_block.hip, the first two without their launch boundary).
// Tile geometry, the MLP chain's stage decode, the fragment-tile load and the chunk-grouped MFMA loop, the window mapping, the
// attention's bias + mask and V-fragment reads, gelu_fast, and the one table of DRCT-L's block shapes every dispatch is built
// from.  DESIGN.md 5g says what stayed written out in which kernel and why.
#pragma once
#include "srad_common.h"

// ---- tile geometry ----
constexpr int SW_LDA = 400;        // LDS row stride of the <=384-wide bf16 activation tile (2 mod 4 sixteen-byte units: conflict-free for the lane groups of ds_read_b128, see kernels_conv80.hip)
constexpr int SW_LDH = 528;        // ... of the <=512-wide hidden tile
constexpr int SW_LDP = 80;         // ... of the probability tile
constexpr int SW_SC = 128;         // output columns per weight stage: 16 per wave
// the MLP chain's vectors as staged in LDS (floats): slots as wide as the widest vector they take (d, no <= 384, m <= 512)
constexpr int SW_V_BP = 0, SW_V_B1 = 384, SW_V_B2 = 896, SW_V_BA = 1280, SW_V_G = 1664, SW_V_B = 2048;   // b_proj | b_fc1 | b_fc2 | b_adj | gamma2 | beta2
constexpr int SW_NV = 2560;        // floats of the six slots (10 per thread)
constexpr int SW_VD = SW_V_B1 - SW_V_BP, SW_VM = SW_V_B2 - SW_V_B1;   // slot widths: a d-wide vector, the hidden bias

// ---- the MLP chain's stages: proj | fc1 | fc2 | adjust, each as 128-column groups x 256-wide k groups ----
// GD / GM / GN = column groups of the block dim / hidden / adjust output, KGD / KGM = k groups of the block dim / hidden,
// KCD / KCM = their 32-wide k chunks (exact: a stage loads and multiplies only its real chunks)
struct MlpStage {
  int ph, g, kg;                   // phase (0 proj, 1 fc1, 2 fc2, 3 adjust), column group, k group
  int kc, nch;                     // k chunks of the phase's weight, chunks of this stage
  bool first, last;                // first stage of its phase; last k group of its column group (the epilogue follows)
};
template <int GD, int KGD, int GM, int KGM, int GN, int KCD, int KCM>
struct MlpChain {
  static_assert(KGD == (KCD + 7) / 8 && KGM == (KCM + 7) / 8, "k groups are 8 chunks wide");
  static constexpr int n_proj = GD * KGD, n_fc1 = GM * KGD, n_fc2 = GD * KGM, n_adj = GN * KGD;
  static constexpr int n_stages = n_proj + n_fc1 + n_fc2 + n_adj;
  static constexpr MlpStage stage(int s) {                        // (stages past the end: the last one, for the look-ahead)
    if (s > n_stages - 1) s = n_stages - 1;
    int ph = 0, kgs = KGD, kc = KCD;
    if (s < n_proj) ph = 0;
    else if ((s -= n_proj) < n_fc1) ph = 1;
    else if ((s -= n_fc1) < n_fc2) { ph = 2; kgs = KGM; kc = KCM; }
    else { s -= n_fc2; ph = 3; }
    const int g = s / kgs, kg = s - g * kgs;
    return MlpStage{ph, g, kg, kc, kc - kg * 8 < 8 ? kc - kg * 8 : 8, s == 0, kg == kgs - 1};
  }
};

// ---- the folded chain (mlp_fold.h): proj | fc1 | adjF, adjF = [bf16(x1) | h] . [A | A W2]^T over KCD + KCM
//      k chunks.  SPLITK (adjust outputs <= 32: two column tiles): ONE stage - wave w owns column tile w & 1 and k part w >> 1
//      of four, each PS = ceil((KCD + KCM) / 4) <= 8 chunks; else 128-column groups x 8-chunk k groups like the other phases ----
template <int GD, int KGD, int GM, int GN, int KCD, int KCM, bool SPLITK>
struct MlpFoldChain {
  static_assert(KGD == (KCD + 7) / 8, "k groups are 8 chunks wide");
  static constexpr int KF = KCD + KCM, KGF = (KF + 7) / 8, PS = (KF + 3) / 4;
  static_assert(!SPLITK || PS <= 8, "a k part fits one register set");
  static constexpr int n_proj = GD * KGD, n_fc1 = GM * KGD, n_adj = SPLITK ? 1 : GN * KGF;
  static constexpr int n_stages = n_proj + n_fc1 + n_adj;
  static constexpr MlpStage stage(int s) {                        // (stages past the end: the last one, for the look-ahead)
    if (s > n_stages - 1) s = n_stages - 1;
    int ph = 0, kgs = KGD, kc = KCD;
    if (s < n_proj) ph = 0;
    else if ((s -= n_proj) < n_fc1) ph = 1;
    else {
      s -= n_fc1; ph = 3; kgs = KGF; kc = KF;
      if (SPLITK) return MlpStage{3, 0, 0, KF, PS, true, true};
    }
    const int g = s / kgs, kg = s - g * kgs;
    return MlpStage{ph, g, kg, kc, kc - kg * 8 < 8 ? kc - kg * 8 : 8, s == 0, kg == kgs - 1};
  }
};
// mlp_block_kernel's folded form: row stride of the folded A tile [rows][32 (KCD + KCM) + 16] (2 mod 4
// sixteen-byte units), and the launch's LDS bytes with that tile in the hidden tile's place; a tile height whose bytes exceed
// the 160 KB of a CU has no folded instance
constexpr int mlp_fold_ldf(int kcd, int kcm) { return 32 * (kcd + kcm) + 16; }
constexpr size_t mlp_fold_lds(int fm, int kcd, int kcm) {
  return (size_t)(fm * SW_LDA + fm * mlp_fold_ldf(kcd, kcm)) * 2 + (size_t)(SW_NV + fm * 16) * sizeof(float);
}
constexpr bool mlp_fold_fits(int fm, int kcd, int kcm) { return mlp_fold_lds(fm, kcd, kcm) <= 160 * 1024; }

// ---- DRCT-L's five Swin block shapes, the one table behind every instance of the four kernels:
//      (d, heads, MLP hidden, adjust outputs, qkv_attn workgroups per CU).  The last column is tuning that cannot be derived.
//      Dispatch matches the geometry key, not d: another shape with the same key (d = 184 ...) runs the same instance. ----
#define SRAD_SWIN_SHAPES(X) X(180, 6, 360, 32, 2) X(212, 4, 424, 32, 2) X(244, 2, 488, 32, 1) X(276, 6, 276, 32, 2) X(308, 4, 308, 180, 1)
struct SwinKey {
  int hdt, kc, heads;              // 16-column tiles of a head, 32-wide k chunks of d, heads
  int gd, kgd, gm, kgm, gn, kcm;   // MlpChain's parameters (KCD == kc)
};
constexpr SwinKey swin_key(int d, int heads = 1, int m = 0, int no = 0) {   // (mlp_block has no heads, the attention no MLP)
  const int kc = (d + 31) / 32, kcm = (m + 31) / 32;
  return SwinKey{(d / heads + 15) / 16, kc, heads, (d + SW_SC - 1) / SW_SC, (kc + 7) / 8, (m + SW_SC - 1) / SW_SC, (kcm + 7) / 8, (no + SW_SC - 1) / SW_SC, kcm};
}
constexpr bool swin_key_mlp_eq(const SwinKey& a, const SwinKey& b) {
  return a.gd == b.gd && a.kgd == b.kgd && a.gm == b.gm && a.kgm == b.kgm && a.gn == b.gn && a.kc == b.kc && a.kcm == b.kcm;
}

#if defined(__HIPCC__)
// the exact-erf GELU on srad_erf_abs (srad_common.h)
__device__ __forceinline__ float gelu_fast(float x) {
  float ex;
  const float erfa = srad_erf_abs(x, ex);
  return 0.5f * x * (1.0f + (x < 0.f ? -erfa : erfa));
}

// XCD affinity: workgroup L runs on XCD L % 8 and each XCD has its own L2, so XCD k takes the k-th contiguous strip of the
// tiles / windows - the same strip of the images in every kernel of the block (see qkv_attn_kernel)
__device__ __forceinline__ int sw_xcd_tile(bool on) {
  return (gridDim.x & 7) == 0 && on ? (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3) : blockIdx.x;
}
// The 8 x 8 window of this workgroup (grid x = windows) and its positions' tokens (cyclic shift + window partition as index
// arithmetic, drct.py:482-504)
struct SwinWindow {
  int H, W, shift, b, wy, wx;
  // token of window position t, and its info word (srad_window_token_info)
  __device__ __forceinline__ int token(int t, int& info) const {
    int tok;
    srad_window_token_info(H, W, 8, shift, b, wy, wx, t >> 3, t & 7, tok, info);
    return tok;
  }
};
__device__ __forceinline__ SwinWindow sw_window(int H, int W, int shift, bool xcd_map) {
  const int win = sw_xcd_tile(xcd_map);
  const int nWx = W / 8, nW = (H / 8) * nWx;
  const int b = win / nW, widx = win - b * nW;
  const int wy = widx / nWx;
  return SwinWindow{H, W, shift, b, wy, widx - wy * nWx};
}
// relative position bias + 0 / -100 shift mask (drct.py:284-292, 449-470) of a (query, key) pair from their info words
// (srad_window_token_info); tbl = [225][stride] with this head at column h, shift = the block's cyclic shift
__device__ __forceinline__ float sw_bias_mask(const float* tbl, int stride, int h, int qi, int ki, int shift) {
  const int ky = (ki >> 8) & 0xff, kx = ki & 0xff, kr = ki >> 16;
  const int qy = (qi >> 8) & 0xff, qx = qi & 0xff, qr = qi >> 16;
  float v = tbl[((qy - ky + 7) * 15 + (qx - kx + 7)) * stride + h];
  if (shift > 0 && qr != kr) v += -100.0f;
  return v;
}
// the MFMA operand of V for P.V: 8 keys x this lane's column, read transposed from row-major V (r0 = the lane's first row
// and column quad, ld = V's row stride)
__device__ __forceinline__ bf16x8 sw_read_v_tr(const __bf16* r0, int ld) {
  typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(r0));
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(r0 + 4 * ld));
  bf16x8 vb;
#pragma unroll
  for (int e = 0; e < 4; ++e) { vb[e] = lo[e]; vb[4 + e] = hi[e]; }
  return vb;
}

// N fragment tiles (1 KB each: 16 weight rows x 32 k; lane: row fr, k 8 fq .. - the 64 lanes cover the tile) from tile
// `tile` of the pack w on, into reg[0 .. N).  The loads are unconditional: a load inside a branch makes hipcc's wait-count
// pass assume the branch was NOT taken at the join and drain every older load there.  A wave without live columns reads one
// 16-byte word per load instead (all lanes the same address: one request).
template <int N, int R>
__device__ __forceinline__ void sw_load_tiles(u32x4 (&reg)[R], const char* w, bool live, size_t tile, int fr, int fq) {
  static_assert(N <= R, "the register set holds the stage");
  const char* base = live ? w + tile * 1024 + fr * 64 + fq * 16 : w;
  const int step = live ? 1024 : 0;
#pragma unroll
  for (int cc = 0; cc < N; ++cc) reg[cc] = *reinterpret_cast<const u32x4*>(base + cc * step);
}
// acc[t] += (A[16 rows of row tile t][nch 32-wide chunks] . W[the wave's 16 columns][..]^T)^T for t < NT; ar = the lane's
// first fragment (row fr, k 8 fq), ld = A's row stride, reg = the chunks' weight fragments.  The activation fragments of CG
// chunks are requested together, THEN multiplied (sched_barrier: left alone the scheduler sinks every LDS read to just above
// its MFMA - the LDS latency exposed once per MFMA).  Operands swapped (W as the MFMA "A"): the result tile is transposed,
// so a lane holds 4 CONSECUTIVE OUTPUT COLUMNS (4 fq + e) of one token row (fr).
template <int CG, int NT, int R, int NA>
__device__ __forceinline__ void sw_mma_chunks(const __bf16* ar, int ld, int nch, int lim, const u32x4 (&reg)[R], f32x4 (&acc)[NA]) {
#pragma unroll
  for (int cc0 = 0; cc0 < lim; cc0 += CG) {
    bf16x8 af[CG][NT];
#pragma unroll
    for (int g = 0; g < CG; ++g)
      if (cc0 + g < nch) {
#pragma unroll
        for (int t = 0; t < NT; ++t) af[g][t] = *reinterpret_cast<const bf16x8*>(ar + t * 16 * ld + (cc0 + g) * 32);
      }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int g = 0; g < CG; ++g)
      if (cc0 + g < nch) {
        const bf16x8 b0 = __builtin_bit_cast(bf16x8, reg[cc0 + g]);
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b0, af[g][t], acc[t], 0, 0, 0);
      }
    __builtin_amdgcn_sched_barrier(0);
  }
}
#endif
