// kernels_attn_bwd.hip - backward of the shifted-window attention on gfx950: dq, dk, dv and the bias-table gradient,
// recomputing P per (window, head) from the saved q | k | v.  Five kernels share the scalar code around their MFMA loops
// as far as hipcc gives them the registers they had with their own copies:
//
//   window_attn_bwd_kernel         8 x 8 windows, fp32 MFMA
//   window_attn_bwd_gen_kernel     window sizes 1 .. 16 other than 8, fp32 MFMA
//   window_attn_bwd_tiled_kernel   32 x 32 and 64 x 64 windows (1024 / 4096 tokens), fp32 MFMA, two passes over 64 x 64 score tiles
//   window_attn_bwd_bf16_kernel    8 x 8, bf16 MFMA, fp32 in and out
//   window_attn_bwd_h_kernel       8 x 8, bf16 in and out: the DRCT training step's kernel
#include "srad_common.h"
#include <math.h>
#include <stdint.h>

namespace {

// ------------------------------------------------------------------------------------------
// What the kernels share (the token / shift-mask geometry is srad_window_token_info of srad_common.h: the fused
// forward takes the same one).
// ------------------------------------------------------------------------------------------
// Workgroup L -> (window, head) of the 8 x 8 kernels.  Workgroups are dealt round-robin over the 8 XCDs; when the window
// count is a multiple of 8, all heads of a window go to ONE XCD (its L2 then holds the window's dO / dqkv lines, which the
// heads share at 4-byte granularity, once): window w on XCD w % 8, or with `strip` XCD k takes the contiguous window strip
// [k nwin / 8, (k + 1) nwin / 8), the strip whose token rows the row-tile kernels before and after give XCD k.
__device__ __forceinline__ void attn_bwd_block_to_window(int L, int nwin, int heads, bool strip, int& win, int& h) {
  if ((nwin & 7) == 0 && strip) { const int slot = L >> 3; win = (L & 7) * (nwin >> 3) + slot / heads; h = slot - (slot / heads) * heads; }
  else if ((nwin & 7) == 0) { const int slot = L >> 3; win = (slot / heads) * 8 + (L & 7); h = slot - (slot / heads) * heads; }
  else { win = L / heads; h = L - win * heads; }
}

// One score of the softmax redo, exactly as the forward forms it: the relative-position bias of (query, key) from the table
// [(2 ws - 1)^2] and the 0 / -100 shift mask (info words as srad_window_token_info packs them; regions differ -> masked).
// The fp32 kernels call it.  The two bf16 kernels keep these three lines written out: with any helper around them, down to one
// that only forms the index, hipcc allocates window_attn_bwd_bf16_kernel 112 VGPRs for 116 and window_attn_bwd_h_kernel<2>
// 104 for 116.  A helper for the whole row (max, exp, sums, dS) moved six of the ten instances, <1> from 124 to 132.
__device__ __forceinline__ float attn_bias_mask(float v, const int qinfo, const int kinfo, const float* tbl, const int ws,
                                                const int tw, const int shift) {
  const int qy = (qinfo >> 8) & 0xff, qx = qinfo & 0xff, qr = qinfo >> 16;
  const int kyy = (kinfo >> 8) & 0xff, kxx = kinfo & 0xff, kr = kinfo >> 16;
  v += tbl[(qy - kyy + ws - 1) * tw + (qx - kxx + ws - 1)];
  if (shift > 0 && qr != kr) v += -100.0f;
  return v;
}

// Bias-table gradient of one (window, head) of 8 x 8, thread t = table entry (dy + 7) * 15 + (dx + 7): it collects dS[q][k] over
// all query positions q whose key k = q - (dy, dx) lies in the window (<= 64 terms), read from the fp32 dS tile [query][key] of
// row stride `stride` - no atomics.  The row goes to the split-K workspace; wgrad_reduce_kernel sums the windows.  The t < 225
// test is in here on purpose: with it at the call sites three kernels take two more SGPRs.
__device__ __forceinline__ void table_grad_row_8x8(const float* tile, const int stride, const int t, float* __restrict__ tpart,
                                                   const int win, const int heads, const int h) {
  const int ws = 8, tw = 2 * ws - 1;
  if (t >= tw * tw) return;
  const int dy = t / tw - (ws - 1), dx = t - (t / tw) * tw - (ws - 1);
  float acc = 0.f;
  for (int qy = max(0, dy); qy < min(ws, ws + dy); ++qy)
    for (int qx = max(0, dx); qx < min(ws, ws + dx); ++qx)
      acc += tile[(qy * ws + qx) * stride + (qy - dy) * ws + (qx - dx)];
  tpart[(size_t)win * (tw * tw * heads) + (size_t)t * heads + h] = acc;
}

// ------------------------------------------------------------------------------------------
// Window attention backward for 8x8 windows (N = 64 tokens), one workgroup per (window, head).
// Pass A walks the head dimension in chunks of 32 columns accumulating S = (q*scale) k^T and
// dP = dO v^T in MFMA accumulators; the softmax is redone in registers exactly as the forward kernel
// does (bias table + 0/-100 shift mask), dS = P (dP - rowsum(P dP)); P and dS go to LDS.
// Pass B walks the chunks again: dq = scale dS k, dk = dS^T (q*scale), dv = P^T dO.
// All MFMAs are v_mfma_f32_16x16x4_f32 (fp32 in, fp32 out) in both precision modes.
// ------------------------------------------------------------------------------------------
constexpr int AB_HC = 32, AB_HS = AB_HC + 4, AB_PS = 64 + 4;
constexpr size_t AB_LDS = (size_t)(4 * 64 * AB_HS + 2 * 64 * AB_PS + 2 * 256) * sizeof(float) + 2 * 64 * sizeof(int);

__global__ __launch_bounds__(256) void window_attn_bwd_kernel(const AttnBwdParams p, float* __restrict__ tpart) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* Qs = reinterpret_cast<float*>(smem);
  float* Ks = Qs + 64 * AB_HS;
  float* Vs = Ks + 64 * AB_HS;
  float* Gs = Vs + 64 * AB_HS;
  float* Pm = Gs + 64 * AB_HS;
  float* Dm = Pm + 64 * AB_PS;
  float* tbl = Dm + 64 * AB_PS;      // [225] (256 reserved)
  float* dtb = tbl + 256;
  int* tok = reinterpret_cast<int*>(dtb + 256);
  int* inf = tok + 64;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int ws = 8, d = p.d, heads = p.heads, hd = d / heads, hdp = p.hdp;
  const int ldq = 3 * heads * hdp;
  const int nWx = p.W / ws, nW = (p.H / ws) * nWx;
  int win, h;
  attn_bwd_block_to_window(blockIdx.x, p.B * nW, heads, false, win, h);
  const int b = win / nW, widx = win - b * nW;
  const int wy = widx / nWx, wx = widx - wy * nWx;
  const float scale = rsqrtf((float)hd);
  const int tw = 2 * ws - 1;

  if (tid < 64) srad_window_token_info(p.H, p.W, ws, p.shift, b, wy, wx, tid / ws, tid % ws, tok[tid], inf[tid]);
  if (tid < tw * tw) tbl[tid] = p.table[(size_t)tid * heads + h];
  __syncthreads();

  // chunk staging: q/k/v as float4 (head-padded rows are 16-byte aligned), dO as scalars
  auto stage = [&](int ch, bool need_v) {
    const int col0 = ch * AB_HC;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = tid + 256 * i;
      const int row = idx >> 3, c = col0 + (idx & 7) * 4;
      const float* base = p.qkv + (size_t)tok[row] * ldq + h * hdp + min(c, hdp - 4);
      f32x4 q4 = *reinterpret_cast<const f32x4*>(base);
      f32x4 k4 = *reinterpret_cast<const f32x4*>(base + heads * hdp);
      f32x4 v4 = need_v ? *reinterpret_cast<const f32x4*>(base + 2 * heads * hdp) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool ok = c + e < hd;
        q4[e] = ok ? q4[e] * scale : 0.f;
        k4[e] = ok ? k4[e] : 0.f;
        v4[e] = ok ? v4[e] : 0.f;
      }
      *reinterpret_cast<f32x4*>(Qs + row * AB_HS + (idx & 7) * 4) = q4;
      *reinterpret_cast<f32x4*>(Ks + row * AB_HS + (idx & 7) * 4) = k4;
      if (need_v) *reinterpret_cast<f32x4*>(Vs + row * AB_HS + (idx & 7) * 4) = v4;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int idx = tid + 256 * i;
      const int row = idx >> 5, cl = idx & 31, c = col0 + cl;
      const float g = p.dout[(size_t)tok[row] * d + h * hd + min(c, hd - 1)];
      Gs[row * AB_HS + cl] = c < hd ? g : 0.f;
    }
  };

  const int nch = (hd + AB_HC - 1) / AB_HC;
  f32x4 s[4], dp[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) { s[j] = f32x4{0.f, 0.f, 0.f, 0.f}; dp[j] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  for (int ch = 0; ch < nch; ++ch) {
    if (ch > 0) __syncthreads();
    stage(ch, true);
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < AB_HC; kk += 16) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(Qs + (wave * 16 + fr) * AB_HS + kk + 4 * fq);
      const f32x4 g = *reinterpret_cast<const f32x4*>(Gs + (wave * 16 + fr) * AB_HS + kk + 4 * fq);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const f32x4 kb = *reinterpret_cast<const f32x4*>(Ks + (j * 16 + fr) * AB_HS + kk + 4 * fq);
        const f32x4 vb = *reinterpret_cast<const f32x4*>(Vs + (j * 16 + fr) * AB_HS + kk + 4 * fq);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          s[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], kb[e], s[j], 0, 0, 0);
          dp[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(g[e], vb[e], dp[j], 0, 0, 0);
        }
      }
    }
  }

  // ---- softmax (row = 16 wave + 4 fq + e, key = 16 j + fr), dS, bias-table gradient ----
  {
    int kinf[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) kinf[j] = inf[j * 16 + fr];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int row = wave * 16 + fq * 4 + e;
      const int qi = inf[row];
      float mx = -1e30f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float v = attn_bias_mask(s[j][e], qi, kinf[j], tbl, ws, tw, p.shift);
        s[j][e] = v;
        mx = fmaxf(mx, v);
      }
      mx = srad_row16_max(mx);
      float sum = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) { s[j][e] = expf(s[j][e] - mx); sum += s[j][e]; }
      sum = srad_row16_sum(sum);
      const float inv = 1.0f / sum;
      float dl = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) { s[j][e] *= inv; dl += s[j][e] * dp[j][e]; }
      dl = srad_row16_sum(dl);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float ds = s[j][e] * (dp[j][e] - dl);
        Pm[row * AB_PS + j * 16 + fr] = s[j][e];
        Dm[row * AB_PS + j * 16 + fr] = ds;
      }
    }
  }
  __syncthreads();
  // bias-table gradient of this (window, head): entry t = (dy + 7) * 15 + (dx + 7) collects dS[q][k] over all query
  // positions q whose key k = q - (dy, dx) lies in the window (<= 64 terms), read from the dS tile - no atomics.
  // The row goes to the split-K workspace; wgrad_reduce_kernel sums the windows.
  table_grad_row_8x8(Dm, AB_PS, tid, tpart, win, heads, h);

  // ---- pass B: dq, dk, dv per 32-column chunk ----
  for (int ch = 0; ch < nch; ++ch) {
    if (ch > 0 || nch > 1) { __syncthreads(); stage(ch, false); __syncthreads(); }
    f32x4 dq[2], dk[2], dv[2];
#pragma unroll
    for (int jt = 0; jt < 2; ++jt) { dq[jt] = f32x4{0.f, 0.f, 0.f, 0.f}; dk[jt] = dq[jt]; dv[jt] = dq[jt]; }
#pragma unroll
    for (int kk = 0; kk < 64; kk += 16) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(Dm + (wave * 16 + fr) * AB_PS + kk + 4 * fq);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int kr = kk + 4 * fq + e;
        const float at = Dm[kr * AB_PS + wave * 16 + fr];     // dS^T
        const float pt = Pm[kr * AB_PS + wave * 16 + fr];     // P^T
#pragma unroll
        for (int jt = 0; jt < 2; ++jt) {
          const float kb = Ks[kr * AB_HS + jt * 16 + fr];
          const float qb = Qs[kr * AB_HS + jt * 16 + fr];
          const float gb = Gs[kr * AB_HS + jt * 16 + fr];
          dq[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], kb, dq[jt], 0, 0, 0);
          dk[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(at, qb, dk[jt], 0, 0, 0);
          dv[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(pt, gb, dv[jt], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float* dst = p.dqkv + (size_t)tok[wave * 16 + fq * 4 + e] * (3 * d) + h * hd;
#pragma unroll
      for (int jt = 0; jt < 2; ++jt) {
        const int c = ch * AB_HC + jt * 16 + fr;
        if (c < hd) {
          dst[c] = dq[jt][e] * scale;
          dst[d + c] = dk[jt][e];
          dst[2 * d + c] = dv[jt][e];
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// The same backward for ANY window size up to 16 (N = ws^2 <= 256 tokens; the reference's CLI presets build windows of
// 2, 4, 8 and 16: window_size = img_size // 4, src/main.py:286 - the 8 x 8 case has its own kernels above).  One workgroup
// per (window, head); the window's tokens are padded to NB blocks of 64 (padding keys get probability 0, padding queries
// are never written).  For each block of 64 queries the whole score row block (64 x 64 NB) and dP stay in MFMA
// accumulators, so the softmax is exact in one pass as above; then key block after key block the P / dS tiles go to LDS
// and feed dq (accumulated in registers over the key blocks), dk and dv (accumulated over the query blocks by
// read-add-write of the workgroup's own rows: one owner, fixed order).  The bias-table gradient is collected in LDS over
// the tiles.  All MFMAs are v_mfma_f32_16x16x4_f32 in every precision mode: these presets are small images, the kernel is
// for coverage, not for the benchmarked configuration.
// ------------------------------------------------------------------------------------------
template <int NB>
__global__ __launch_bounds__(256) void window_attn_bwd_gen_kernel(const AttnBwdParams p, float* __restrict__ tpart) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* Qs = reinterpret_cast<float*>(smem);
  float* Ks = Qs + 64 * AB_HS;
  float* Vs = Ks + 64 * AB_HS;
  float* Gs = Vs + 64 * AB_HS;
  float* Pm = Gs + 64 * AB_HS;
  float* Dm = Pm + 64 * AB_PS;
  float* tbl = Dm + 64 * AB_PS;      // [(2 ws - 1)^2] <= 961 (1024 reserved)
  float* dtb = tbl + 1024;           // its gradient
  int* tok = reinterpret_cast<int*>(dtb + 1024);   // [64 NB]
  int* inf = tok + 64 * NB;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int ws = p.ws, N = ws * ws, d = p.d, heads = p.heads, hd = d / heads, hdp = p.hdp;
  const int ldq = 3 * heads * hdp;
  const int nWx = p.W / ws, nW = (p.H / ws) * nWx;
  const int win = blockIdx.x / heads, h = blockIdx.x - win * heads;
  const int b = win / nW, widx = win - b * nW;
  const int wy = widx / nWx, wx = widx - wy * nWx;
  const float scale = rsqrtf((float)hd);
  const int tw = 2 * ws - 1, ntbl = tw * tw;

  for (int t = tid; t < 64 * NB; t += 256) {
    const int tc = min(t, N - 1);                                 // padding rows point at a real token and are masked
    srad_window_token_info(p.H, p.W, ws, p.shift, b, wy, wx, tc / ws, tc % ws, tok[t], inf[t]);
  }
  for (int t = tid; t < ntbl; t += 256) { tbl[t] = p.table[(size_t)t * heads + h]; dtb[t] = 0.f; }
  __syncthreads();

  // stage a 32-column chunk of 64 rows (block `blk` of the window's tokens) of q*scale / k / v / dO into its LDS tile
  auto stage_rows = [&](float* dst, int blk, int ch, int which /* 0 q, 1 k, 2 v */) {
    const int col0 = ch * AB_HC;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = tid + 256 * i;
      const int row = idx >> 3, c = col0 + (idx & 7) * 4;
      const float* base = p.qkv + (size_t)tok[blk * 64 + row] * ldq + (which * heads + h) * hdp + min(c, hdp - 4);
      f32x4 v4 = *reinterpret_cast<const f32x4*>(base);
#pragma unroll
      for (int e = 0; e < 4; ++e) v4[e] = c + e < hd ? (which == 0 ? v4[e] * scale : v4[e]) : 0.f;
      *reinterpret_cast<f32x4*>(dst + row * AB_HS + (idx & 7) * 4) = v4;
    }
  };
  auto stage_g = [&](int blk, int ch) {
    const int col0 = ch * AB_HC;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int idx = tid + 256 * i;
      const int row = idx >> 5, cl = idx & 31, c = col0 + cl;
      const float g = p.dout[(size_t)tok[blk * 64 + row] * d + h * hd + min(c, hd - 1)];
      Gs[row * AB_HS + cl] = c < hd ? g : 0.f;
    }
  };

  const int nch = (hd + AB_HC - 1) / AB_HC;                        // <= 4 (head dims up to 128)
  for (int qb = 0; qb < NB; ++qb) {
    if (qb * 64 >= N) break;
    // ---- S = (q scale) k^T and dP = dO v^T for this query block against every key block ----
    f32x4 s[NB][4], dp[NB][4];
#pragma unroll
    for (int kb = 0; kb < NB; ++kb)
#pragma unroll
      for (int j = 0; j < 4; ++j) { s[kb][j] = f32x4{0.f, 0.f, 0.f, 0.f}; dp[kb][j] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    for (int ch = 0; ch < nch; ++ch) {
      __syncthreads();
      stage_rows(Qs, qb, ch, 0);
      stage_g(qb, ch);
#pragma unroll
      for (int kb = 0; kb < NB; ++kb) {
        if (kb > 0) __syncthreads();
        stage_rows(Ks, kb, ch, 1);
        stage_rows(Vs, kb, ch, 2);
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < AB_HC; kk += 16) {
          const f32x4 a = *reinterpret_cast<const f32x4*>(Qs + (wave * 16 + fr) * AB_HS + kk + 4 * fq);
          const f32x4 g = *reinterpret_cast<const f32x4*>(Gs + (wave * 16 + fr) * AB_HS + kk + 4 * fq);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const f32x4 kbv = *reinterpret_cast<const f32x4*>(Ks + (j * 16 + fr) * AB_HS + kk + 4 * fq);
            const f32x4 vb = *reinterpret_cast<const f32x4*>(Vs + (j * 16 + fr) * AB_HS + kk + 4 * fq);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              s[kb][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], kbv[e], s[kb][j], 0, 0, 0);
              dp[kb][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(g[e], vb[e], dp[kb][j], 0, 0, 0);
            }
          }
        }
      }
    }
    // ---- softmax over the window's N keys (row = 64 qb + 16 wave + 4 fq + e, key = 64 kb + 16 j + fr), dS in place of dp ----
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int qi = inf[qb * 64 + wave * 16 + fq * 4 + e];
      float mx = -1e30f;
#pragma unroll
      for (int kb = 0; kb < NB; ++kb)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int key = kb * 64 + j * 16 + fr;
          float v = attn_bias_mask(s[kb][j][e], qi, inf[key], tbl, ws, tw, p.shift);
          if (key >= N) v = -1e30f;
          s[kb][j][e] = v;
          mx = fmaxf(mx, v);
        }
      mx = srad_row16_max(mx);
      float sum = 0.f;
#pragma unroll
      for (int kb = 0; kb < NB; ++kb)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float pv = kb * 64 + j * 16 + fr < N ? expf(s[kb][j][e] - mx) : 0.f;
          s[kb][j][e] = pv;
          sum += pv;
        }
      sum = srad_row16_sum(sum);
      const float inv = 1.0f / sum;
      float dl = 0.f;
#pragma unroll
      for (int kb = 0; kb < NB; ++kb)
#pragma unroll
        for (int j = 0; j < 4; ++j) { s[kb][j][e] *= inv; dl += s[kb][j][e] * dp[kb][j][e]; }
      dl = srad_row16_sum(dl);
      const bool qreal = qb * 64 + wave * 16 + fq * 4 + e < N;      // a padding query contributes nothing to dk / dv / the table
#pragma unroll
      for (int kb = 0; kb < NB; ++kb)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          dp[kb][j][e] = qreal ? s[kb][j][e] * (dp[kb][j][e] - dl) : 0.f;
          if (!qreal) s[kb][j][e] = 0.f;
        }
    }
    // ---- key block after key block: P / dS tiles -> LDS, table gradient, dq (registers), dk / dv (read-add-write) ----
    f32x4 dq[4][2];
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) { dq[ch][0] = f32x4{0.f, 0.f, 0.f, 0.f}; dq[ch][1] = dq[ch][0]; }
#pragma unroll
    for (int kb = 0; kb < NB; ++kb) {
      if (kb * 64 >= N) continue;
      __syncthreads();
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          Pm[(wave * 16 + fq * 4 + e) * AB_PS + j * 16 + fr] = s[kb][j][e];
          Dm[(wave * 16 + fq * 4 + e) * AB_PS + j * 16 + fr] = dp[kb][j][e];
        }
      __syncthreads();
      // table entry t = (dy + ws - 1) (2 ws - 1) + (dx + ws - 1): the dS of every (query, key = query - (dy, dx)) pair of this tile
      for (int t = tid; t < ntbl; t += 256) {
        const int dy = t / tw - (ws - 1), dx = t - (t / tw) * tw - (ws - 1);
        float acc = 0.f;
        for (int qy = max(0, dy); qy < min(ws, ws + dy); ++qy)
          for (int qx = max(0, dx); qx < min(ws, ws + dx); ++qx) {
            const int qn = qy * ws + qx - qb * 64, kn = (qy - dy) * ws + (qx - dx) - kb * 64;
            if (qn >= 0 && qn < 64 && kn >= 0 && kn < 64) acc += Dm[qn * AB_PS + kn];
          }
        dtb[t] += acc;                                              // (one thread per entry: no race)
      }
#pragma unroll
      for (int ch = 0; ch < 4; ++ch) {
        if (ch >= nch) continue;
        __syncthreads();
        stage_rows(Ks, kb, ch, 1);
        stage_rows(Qs, qb, ch, 0);
        stage_g(qb, ch);
        __syncthreads();
        f32x4 dk[2], dv[2];
#pragma unroll
        for (int jt = 0; jt < 2; ++jt) { dk[jt] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[jt] = dk[jt]; }
#pragma unroll
        for (int kk = 0; kk < 64; kk += 16) {
          const f32x4 a = *reinterpret_cast<const f32x4*>(Dm + (wave * 16 + fr) * AB_PS + kk + 4 * fq);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int kr = kk + 4 * fq + e;
            const float at = Dm[kr * AB_PS + wave * 16 + fr];     // dS^T
            const float pt = Pm[kr * AB_PS + wave * 16 + fr];     // P^T
#pragma unroll
            for (int jt = 0; jt < 2; ++jt) {
              const float kbv = Ks[kr * AB_HS + jt * 16 + fr];
              const float qbv = Qs[kr * AB_HS + jt * 16 + fr];
              const float gb = Gs[kr * AB_HS + jt * 16 + fr];
              dq[ch][jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], kbv, dq[ch][jt], 0, 0, 0);
              dk[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(at, qbv, dk[jt], 0, 0, 0);
              dv[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(pt, gb, dv[jt], 0, 0, 0);
            }
          }
        }
        // dk / dv rows of key block kb (row = 64 kb + 16 wave + 4 fq + e): first query block writes, later ones add
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int key = kb * 64 + wave * 16 + fq * 4 + e;
          if (key >= N) continue;
          float* dst = p.dqkv + (size_t)tok[key] * (3 * d) + h * hd;
#pragma unroll
          for (int jt = 0; jt < 2; ++jt) {
            const int c = ch * AB_HC + jt * 16 + fr;
            if (c < hd) {
              if (qb == 0) { dst[d + c] = dk[jt][e]; dst[2 * d + c] = dv[jt][e]; }
              else { dst[d + c] += dk[jt][e]; dst[2 * d + c] += dv[jt][e]; }
            }
          }
        }
      }
    }
    // dq rows of this query block
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
      if (ch >= nch) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int qrow = qb * 64 + wave * 16 + fq * 4 + e;
        if (qrow >= N) continue;
        float* dst = p.dqkv + (size_t)tok[qrow] * (3 * d) + h * hd;
#pragma unroll
        for (int jt = 0; jt < 2; ++jt) {
          const int c = ch * AB_HC + jt * 16 + fr;
          if (c < hd) dst[c] = dq[ch][jt][e] * scale;
        }
      }
    }
    __threadfence_block();
  }
  __syncthreads();
  for (int t = tid; t < ntbl; t += 256) tpart[(size_t)win * (ntbl * heads) + (size_t)t * heads + h] = dtb[t];
}
constexpr size_t ABG_LDS(int nb) { return (size_t)(4 * 64 * AB_HS + 2 * 64 * AB_PS + 2 * 1024) * sizeof(float) + 2 * 64 * nb * sizeof(int); }

// ------------------------------------------------------------------------------------------
// The same backward for 32 x 32 and 64 x 64 windows (N = 1024 / 4096 tokens: the 512 and 1024 px presets), where a 64 x N
// score row block no longer fits in accumulators.  One workgroup per (window, head) owns every output of that pair, and
// nothing N x N ever exists: the scores are walked as 64 x 64 tiles (query block qb, key block kb), twice per query block.
//   pass 1, kb = 0 .. N/64 - 1:  S = (q scale) k^T + bias + mask and dP = dO v^T of the tile; the row maximum m, the row sum
//           l of exp(S - m) and a = sum exp(S - m) dP are carried online (rescaled when m grows).  D = rowsum(P dP) = a / l.
//   pass 2, kb = 0 .. N/64 - 1:  the tile's S and dP again, P = exp(S - m) / l, dS = P (dP - D); the P / dS tiles go through
//           LDS as in the general kernel: dq += dS k in registers over kb (written once per query block), dk = dS^T (q scale)
//           and dv = P^T dO added to the workgroup's own rows in HBM (the thread that wrote an element is the one that adds
//           to it, query blocks in ascending order), and dS folded into the head's table gradient, which stays in LDS
//           ((2 ws - 1)^2 floats: 64.5 KB at ws 64) until the end.
// A block of 64 tokens is 64 / ws window rows (two at ws 32, one at 64), so a tile only meets (4 ws / 64 - 1)(2 ws - 1) <= 189
// entries of the table: that slice is fetched per tile (the whole table and its gradient do not both fit in LDS), and the
// fold has one thread per entry of the slice - no atomics, fixed order, bit-identical from run to run.
// ------------------------------------------------------------------------------------------
constexpr int ABT_SLICE = 192;      // >= 3 * 63 (ws 32) and >= 127 (ws 64)
constexpr size_t ABT_LDS(int ws) {
  return (size_t)(4 * 64 * AB_HS + 2 * 64 * AB_PS + ABT_SLICE + (2 * ws - 1) * (2 * ws - 1) + 3) * sizeof(float) + 4 * 64 * sizeof(int);
}
static_assert(ABT_LDS(64) <= 160 * 1024, "window_attn_bwd (tiled): LDS budget");

// attn_bias_mask against a slice of the table that starts at row dy0 + ws - 1 (dy0 = smallest qy - ky of the tile)
__device__ __forceinline__ float attn_bias_mask_slice(float v, const int qinfo, const int kinfo, const float* tsl, const int dy0,
                                                      const int ws, const int tw, const int shift) {
  const int qy = (qinfo >> 8) & 0xff, qx = qinfo & 0xff, qr = qinfo >> 16;
  const int kyy = (kinfo >> 8) & 0xff, kxx = kinfo & 0xff, kr = kinfo >> 16;
  v += tsl[(qy - kyy - dy0) * tw + (qx - kxx + ws - 1)];
  if (shift > 0 && qr != kr) v += -100.0f;
  return v;
}

__global__ __launch_bounds__(256) void window_attn_bwd_tiled_kernel(const AttnBwdParams p, float* __restrict__ tpart) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* Qs = reinterpret_cast<float*>(smem);
  float* Ks = Qs + 64 * AB_HS;
  float* Vs = Ks + 64 * AB_HS;
  float* Gs = Vs + 64 * AB_HS;
  float* Pm = Gs + 64 * AB_HS;
  float* Dm = Pm + 64 * AB_PS;
  float* tsl = Dm + 64 * AB_PS;      // the tile's slice of the bias table [2 rpb - 1][2 ws - 1]
  int* tokq = reinterpret_cast<int*>(tsl + ABT_SLICE);   // [64] each: tokens / info words of the query and the key block
  int* infq = tokq + 64;
  int* tokk = infq + 64;
  int* infk = tokk + 64;
  float* dtb = reinterpret_cast<float*>(infk + 64);      // [(2 ws - 1)^2] the head's table gradient

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int ws = p.ws, N = ws * ws, d = p.d, heads = p.heads, hd = d / heads, hdp = p.hdp;
  const int nblk = N / 64, rpb = 64 / ws;                            // window rows per block of 64 tokens
  const int ldq = 3 * heads * hdp;
  const int nWx = p.W / ws, nW = (p.H / ws) * nWx;
  const int win = blockIdx.x / heads, h = blockIdx.x - win * heads;
  const int b = win / nW, widx = win - b * nW;
  const int wy = widx / nWx, wx = widx - wy * nWx;
  const float scale = rsqrtf((float)hd);
  const int tw = 2 * ws - 1, ntbl = tw * tw, nsl = (2 * rpb - 1) * tw;
  const int nch = (hd + AB_HC - 1) / AB_HC;                          // <= 4 (head dims up to 128)

  for (int t = tid; t < ntbl; t += 256) dtb[t] = 0.f;

  auto set_block = [&](int* tok, int* inf, int blk) {
    if (tid < 64) { const int n = blk * 64 + tid; srad_window_token_info(p.H, p.W, ws, p.shift, b, wy, wx, n / ws, n % ws, tok[tid], inf[tid]); }
  };
  // table rows (qb - kb) rpb - (rpb - 1) + ws - 1 ... of the tile (qb, kb): every (qy - ky, qx - kx) its 64 x 64 pairs meet
  auto load_slice = [&](int dy0) {
    if (tid < nsl) {
      const int r = dy0 + ws - 1 + tid / tw;
      tsl[tid] = r >= 0 && r < tw ? p.table[((size_t)r * tw + (tid - (tid / tw) * tw)) * heads + h] : 0.f;
    }
  };
  // stage a 32-column chunk of the 64 rows `tok` of q*scale / k / v / dO into its LDS tile
  auto stage_rows = [&](float* dst, const int* tok, int ch, int which /* 0 q, 1 k, 2 v */) {
    const int col0 = ch * AB_HC;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = tid + 256 * i;
      const int row = idx >> 3, c = col0 + (idx & 7) * 4;
      const float* base = p.qkv + (size_t)tok[row] * ldq + (which * heads + h) * hdp + min(c, hdp - 4);
      f32x4 v4 = *reinterpret_cast<const f32x4*>(base);
#pragma unroll
      for (int e = 0; e < 4; ++e) v4[e] = c + e < hd ? (which == 0 ? v4[e] * scale : v4[e]) : 0.f;
      *reinterpret_cast<f32x4*>(dst + row * AB_HS + (idx & 7) * 4) = v4;
    }
  };
  auto stage_g = [&](int ch) {
    const int col0 = ch * AB_HC;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int idx = tid + 256 * i;
      const int row = idx >> 5, cl = idx & 31, c = col0 + cl;
      const float g = p.dout[(size_t)tokq[row] * d + h * hd + min(c, hd - 1)];
      Gs[row * AB_HS + cl] = c < hd ? g : 0.f;
    }
  };
  // S = (q scale) k^T and dP = dO v^T of the current tile (row = 16 wave + 4 fq + e, key = 16 j + fr).  Called after a barrier
  // behind set_block; with one chunk the query block's q and dO stay in LDS from its first tile on (stage_q false).
  f32x4 s[4], dp[4];
  auto tile_scores = [&](bool stage_q) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < 4; ++j) { s[j] = f32x4{0.f, 0.f, 0.f, 0.f}; dp[j] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    for (int ch = 0; ch < nch; ++ch) {
      if (ch > 0) __syncthreads();
      if (stage_q || nch > 1) { stage_rows(Qs, tokq, ch, 0); stage_g(ch); }
      stage_rows(Ks, tokk, ch, 1);
      stage_rows(Vs, tokk, ch, 2);
      __syncthreads();
#pragma unroll
      for (int kk = 0; kk < AB_HC; kk += 16) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(Qs + (wave * 16 + fr) * AB_HS + kk + 4 * fq);
        const f32x4 g = *reinterpret_cast<const f32x4*>(Gs + (wave * 16 + fr) * AB_HS + kk + 4 * fq);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const f32x4 kbv = *reinterpret_cast<const f32x4*>(Ks + (j * 16 + fr) * AB_HS + kk + 4 * fq);
          const f32x4 vb = *reinterpret_cast<const f32x4*>(Vs + (j * 16 + fr) * AB_HS + kk + 4 * fq);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            s[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], kbv[e], s[j], 0, 0, 0);
            dp[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(g[e], vb[e], dp[j], 0, 0, 0);
          }
        }
      }
    }
  };

  for (int qb = 0; qb < nblk; ++qb) {
    __syncthreads();
    set_block(tokq, infq, qb);
    // ---- pass 1: row maximum, row sum and D = rowsum(P dP), online over the key blocks ----
    float rm[4], rl[4], ra[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) { rm[e] = -1e30f; rl[e] = 0.f; ra[e] = 0.f; }
    for (int kb = 0; kb < nblk; ++kb) {
      const int dy0 = (qb - kb) * rpb - (rpb - 1);
      if (kb > 0) __syncthreads();
      set_block(tokk, infk, kb);
      load_slice(dy0);
      __syncthreads();
      tile_scores(kb == 0);
      int kinf[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) kinf[j] = infk[j * 16 + fr];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int qi = infq[wave * 16 + fq * 4 + e];
        float mx = -1e30f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float v = attn_bias_mask_slice(s[j][e], qi, kinf[j], tsl, dy0, ws, tw, p.shift);
          s[j][e] = v;
          mx = fmaxf(mx, v);
        }
        mx = fmaxf(rm[e], srad_row16_max(mx));
        float sum = 0.f, da = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) { const float pv = expf(s[j][e] - mx); sum += pv; da += pv * dp[j][e]; }
        const float corr = expf(rm[e] - mx);
        rl[e] = rl[e] * corr + srad_row16_sum(sum);
        ra[e] = ra[e] * corr + srad_row16_sum(da);
        rm[e] = mx;
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) { rl[e] = 1.0f / rl[e]; ra[e] *= rl[e]; }       // 1 / l and D
    // ---- pass 2: P and dS tile after tile -> table gradient, dq (registers), dk / dv (read-add-write of own rows) ----
    f32x4 dq[4][2];
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) { dq[ch][0] = f32x4{0.f, 0.f, 0.f, 0.f}; dq[ch][1] = dq[ch][0]; }
    for (int kb = 0; kb < nblk; ++kb) {
      const int dy0 = (qb - kb) * rpb - (rpb - 1);
      __syncthreads();
      set_block(tokk, infk, kb);
      load_slice(dy0);
      __syncthreads();
      tile_scores(false);
      {
        int kinf[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) kinf[j] = infk[j * 16 + fr];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = wave * 16 + fq * 4 + e;
          const int qi = infq[row];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float v = attn_bias_mask_slice(s[j][e], qi, kinf[j], tsl, dy0, ws, tw, p.shift);
            const float pv = expf(v - rm[e]) * rl[e];
            Pm[row * AB_PS + j * 16 + fr] = pv;
            Dm[row * AB_PS + j * 16 + fr] = pv * (dp[j][e] - ra[e]);
          }
        }
      }
      __syncthreads();
      // slice entry t = (dyl + rpb - 1) (2 ws - 1) + (dx + ws - 1): the dS of every (query, key = query - (dy, dx)) pair of this tile
      if (tid < nsl) {
        const int dyl = tid / tw - (rpb - 1), dxi = tid - (tid / tw) * tw, dx = dxi - (ws - 1);
        float acc = 0.f;
        for (int qyl = max(0, dyl); qyl < min(rpb, rpb + dyl); ++qyl)
          for (int qx = max(0, dx); qx < min(ws, ws + dx); ++qx)
            acc += Dm[(qyl * ws + qx) * AB_PS + (qyl - dyl) * ws + qx - dx];
        dtb[((qb - kb) * rpb + dyl + ws - 1) * tw + dxi] += acc;     // (one thread per entry of a tile, tiles behind barriers: no race)
      }
#pragma unroll
      for (int ch = 0; ch < 4; ++ch) {
        if (ch >= nch) continue;
        if (nch > 1) {
          __syncthreads();
          stage_rows(Ks, tokk, ch, 1);
          stage_rows(Qs, tokq, ch, 0);
          stage_g(ch);
          __syncthreads();
        }
        f32x4 dk[2], dv[2];
#pragma unroll
        for (int jt = 0; jt < 2; ++jt) { dk[jt] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[jt] = dk[jt]; }
#pragma unroll
        for (int kk = 0; kk < 64; kk += 16) {
          const f32x4 a = *reinterpret_cast<const f32x4*>(Dm + (wave * 16 + fr) * AB_PS + kk + 4 * fq);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int kr = kk + 4 * fq + e;
            const float at = Dm[kr * AB_PS + wave * 16 + fr];     // dS^T
            const float pt = Pm[kr * AB_PS + wave * 16 + fr];     // P^T
#pragma unroll
            for (int jt = 0; jt < 2; ++jt) {
              const float kbv = Ks[kr * AB_HS + jt * 16 + fr];
              const float qbv = Qs[kr * AB_HS + jt * 16 + fr];
              const float gb = Gs[kr * AB_HS + jt * 16 + fr];
              dq[ch][jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], kbv, dq[ch][jt], 0, 0, 0);
              dk[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(at, qbv, dk[jt], 0, 0, 0);
              dv[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(pt, gb, dv[jt], 0, 0, 0);
            }
          }
        }
        // dk / dv rows of key block kb (row = 16 wave + 4 fq + e): the first query block writes, later ones add (same thread)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float* dst = p.dqkv + (size_t)tokk[wave * 16 + fq * 4 + e] * (3 * d) + h * hd;
#pragma unroll
          for (int jt = 0; jt < 2; ++jt) {
            const int c = ch * AB_HC + jt * 16 + fr;
            if (c < hd) {
              if (qb == 0) { dst[d + c] = dk[jt][e]; dst[2 * d + c] = dv[jt][e]; }
              else { dst[d + c] += dk[jt][e]; dst[2 * d + c] += dv[jt][e]; }
            }
          }
        }
      }
    }
    // dq rows of this query block
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
      if (ch >= nch) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float* dst = p.dqkv + (size_t)tokq[wave * 16 + fq * 4 + e] * (3 * d) + h * hd;
#pragma unroll
        for (int jt = 0; jt < 2; ++jt) {
          const int c = ch * AB_HC + jt * 16 + fr;
          if (c < hd) dst[c] = dq[ch][jt][e] * scale;
        }
      }
    }
  }
  __syncthreads();
  for (int t = tid; t < ntbl; t += 256) tpart[(size_t)win * ((size_t)ntbl * heads) + (size_t)t * heads + h] = dtb[t];
}

// ------------------------------------------------------------------------------------------
// The same backward with bf16 MFMA operands (v_mfma_f32_16x16x32_bf16, fp32 accumulation) for the bf16 precision
// mode: q, k, v, dO chunks are staged as bf16; P and dS leave the softmax as bf16 tiles - dS in both orientations
// (row-major for dq = dS k, transposed for dk = dS^T q), P transposed (dv = P^T dO) - and the second operand of
// those three products (k, q, dO: contraction over tokens, their slow axis in LDS) comes through the transposing
// LDS read ds_read_b64_tr_b16.  Softmax statistics, dS and the bias-table gradient stay fp32.
// ------------------------------------------------------------------------------------------
constexpr int AH_HS = 32 + 8, AH_PS = 64 + 8;
constexpr size_t AH_LDS = (size_t)(4 * 64 * AH_HS + 3 * 64 * AH_PS) * sizeof(__bf16) + (size_t)(256 + 64 * 68) * sizeof(float) + 2 * 64 * sizeof(int);

__global__ __launch_bounds__(256) void window_attn_bwd_bf16_kernel(const AttnBwdParams p, float* __restrict__ tpart) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __bf16* Qs = reinterpret_cast<__bf16*>(smem);          // [64][AH_HS] q * scale chunk
  __bf16* Ks = Qs + 64 * AH_HS;
  __bf16* Vs = Ks + 64 * AH_HS;
  __bf16* Gs = Vs + 64 * AH_HS;                          // dO chunk
  __bf16* Dm = Gs + 64 * AH_HS;                          // [query][key] dS
  __bf16* DmT = Dm + 64 * AH_PS;                         // [key][query] dS
  __bf16* PmT = DmT + 64 * AH_PS;                        // [key][query] P
  float* tbl = reinterpret_cast<float*>(PmT + 64 * AH_PS);   // [225] (256 reserved)
  float* Df = tbl + 256;                                 // [64][68] fp32 dS for the bias-table gradient
  int* tok = reinterpret_cast<int*>(Df + 64 * 68);
  int* inf = tok + 64;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int ws = 8, d = p.d, heads = p.heads, hd = d / heads, hdp = p.hdp;
  const int ldq = 3 * heads * hdp;
  const int nWx = p.W / ws, nW = (p.H / ws) * nWx;
  int win, h;
  attn_bwd_block_to_window(blockIdx.x, p.B * nW, heads, false, win, h);
  const int b = win / nW, widx = win - b * nW;
  const int wy = widx / nWx, wx = widx - wy * nWx;
  const float scale = rsqrtf((float)hd);
  const int tw = 2 * ws - 1;

  if (tid < 64) srad_window_token_info(p.H, p.W, ws, p.shift, b, wy, wx, tid / ws, tid % ws, tok[tid], inf[tid]);
  if (tid < tw * tw) tbl[tid] = p.table[(size_t)tid * heads + h];
  __syncthreads();

  auto stage = [&](int ch, bool need_v) {
    const int col0 = ch * 32;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = tid + 256 * i;
      const int row = idx >> 3, cl = (idx & 7) * 4, c = col0 + cl;
      const float* base = p.qkv + (size_t)tok[row] * ldq + h * hdp + min(c, hdp - 4);
      const f32x4 q4 = *reinterpret_cast<const f32x4*>(base);
      const f32x4 k4 = *reinterpret_cast<const f32x4*>(base + heads * hdp);
      const f32x4 v4 = need_v ? *reinterpret_cast<const f32x4*>(base + 2 * heads * hdp) : f32x4{0.f, 0.f, 0.f, 0.f};
      bf16x4 qh, kh, vh;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool ok = c + e < hd;
        qh[e] = (__bf16)(ok ? q4[e] * scale : 0.f);
        kh[e] = (__bf16)(ok ? k4[e] : 0.f);
        vh[e] = (__bf16)(ok ? v4[e] : 0.f);
      }
      *reinterpret_cast<bf16x4*>(Qs + row * AH_HS + cl) = qh;
      *reinterpret_cast<bf16x4*>(Ks + row * AH_HS + cl) = kh;
      if (need_v) *reinterpret_cast<bf16x4*>(Vs + row * AH_HS + cl) = vh;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int idx = tid + 256 * i;
      const int row = idx >> 5, cl = idx & 31, c = col0 + cl;
      const float g = p.dout[(size_t)tok[row] * d + h * hd + min(c, hd - 1)];
      Gs[row * AH_HS + cl] = (__bf16)(c < hd ? g : 0.f);
    }
  };

  const int nch = (hd + 31) / 32;
  f32x4 s[4], dp[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) { s[j] = f32x4{0.f, 0.f, 0.f, 0.f}; dp[j] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  for (int ch = 0; ch < nch; ++ch) {
    if (ch > 0) __syncthreads();
    stage(ch, true);
    __syncthreads();
    const bf16x8 a = *reinterpret_cast<const bf16x8*>(Qs + (wave * 16 + fr) * AH_HS + 8 * fq);
    const bf16x8 g = *reinterpret_cast<const bf16x8*>(Gs + (wave * 16 + fr) * AH_HS + 8 * fq);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bf16x8 kb = *reinterpret_cast<const bf16x8*>(Ks + (j * 16 + fr) * AH_HS + 8 * fq);
      const bf16x8 vb = *reinterpret_cast<const bf16x8*>(Vs + (j * 16 + fr) * AH_HS + 8 * fq);
      s[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, kb, s[j], 0, 0, 0);
      dp[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(g, vb, dp[j], 0, 0, 0);
    }
  }

  // ---- softmax (row = 16 wave + 4 fq + e, key = 16 j + fr), dS ----
  {
    int kinf[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) kinf[j] = inf[j * 16 + fr];
    f32x4 pr[4], dsr[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int row = wave * 16 + fq * 4 + e;
      const int qi = inf[row];
      const int qy = (qi >> 8) & 0xff, qx = qi & 0xff, qr = qi >> 16;
      float mx = -1e30f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int kyy = (kinf[j] >> 8) & 0xff, kxx = kinf[j] & 0xff, kr = kinf[j] >> 16;   // attn_bias_mask, written out (see there)
        float v = s[j][e] + tbl[(qy - kyy + ws - 1) * tw + (qx - kxx + ws - 1)];
        if (p.shift > 0 && qr != kr) v += -100.0f;
        s[j][e] = v;
        mx = fmaxf(mx, v);
      }
      mx = srad_row16_max(mx);
      float sum = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) { s[j][e] = __expf(s[j][e] - mx); sum += s[j][e]; }
      sum = srad_row16_sum(sum);
      const float inv = 1.0f / sum;
      float dl = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) { s[j][e] *= inv; dl += s[j][e] * dp[j][e]; }
      dl = srad_row16_sum(dl);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float ds = s[j][e] * (dp[j][e] - dl);
        pr[j][e] = s[j][e]; dsr[j][e] = ds;
        Dm[row * AH_PS + j * 16 + fr] = (__bf16)ds;
        Df[row * 68 + j * 16 + fr] = ds;
      }
    }
    // transposed tiles: this lane's four rows 4 fq .. 4 fq + 3 of query slab `wave` are consecutive along k
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bf16x4 ph, dh;
#pragma unroll
      for (int e = 0; e < 4; ++e) { ph[e] = (__bf16)pr[j][e]; dh[e] = (__bf16)dsr[j][e]; }
      *reinterpret_cast<bf16x4*>(PmT + (j * 16 + fr) * AH_PS + wave * 16 + 4 * fq) = ph;
      *reinterpret_cast<bf16x4*>(DmT + (j * 16 + fr) * AH_PS + wave * 16 + 4 * fq) = dh;
    }
  }
  __syncthreads();
  table_grad_row_8x8(Df, 68, tid, tpart, win, heads, h);

  // ---- pass B: dq, dk, dv per 32-column chunk ----
  typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
  const int tq = fr >> 2, tp = fr & 3;
  for (int ch = 0; ch < nch; ++ch) {
    if (ch > 0 || nch > 1) { __syncthreads(); stage(ch, false); __syncthreads(); }
    f32x4 dq[2], dk[2], dv[2];
#pragma unroll
    for (int jt = 0; jt < 2; ++jt) { dq[jt] = f32x4{0.f, 0.f, 0.f, 0.f}; dk[jt] = dq[jt]; dv[jt] = dq[jt]; }
#pragma unroll
    for (int kk = 0; kk < 64; kk += 32) {
      const bf16x8 a_ds = *reinterpret_cast<const bf16x8*>(Dm + (wave * 16 + fr) * AH_PS + kk + 8 * fq);
      const bf16x8 a_dst = *reinterpret_cast<const bf16x8*>(DmT + (wave * 16 + fr) * AH_PS + kk + 8 * fq);
      const bf16x8 a_pt = *reinterpret_cast<const bf16x8*>(PmT + (wave * 16 + fr) * AH_PS + kk + 8 * fq);
#pragma unroll
      for (int jt = 0; jt < 2; ++jt) {
        // B[k = token kk + 8 fq + t][j = column 16 jt + fr] of the row-major chunk tiles: two transposing reads each
        auto tr8 = [&](const __bf16* tile) -> bf16x8 {
          const __bf16* r0 = tile + (kk + 8 * fq + tq) * AH_HS + jt * 16 + 4 * tp;
          const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(r0));
          const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(r0 + 4 * AH_HS));
          bf16x8 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) { o[e] = lo[e]; o[4 + e] = hi[e]; }
          return o;
        };
        dq[jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_ds, tr8(Ks), dq[jt], 0, 0, 0);
        dk[jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_dst, tr8(Qs), dk[jt], 0, 0, 0);
        dv[jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_pt, tr8(Gs), dv[jt], 0, 0, 0);
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float* dst = p.dqkv + (size_t)tok[wave * 16 + fq * 4 + e] * (3 * d) + h * hd;
#pragma unroll
      for (int jt = 0; jt < 2; ++jt) {
        const int c = ch * 32 + jt * 16 + fr;
        if (c < hd) {
          if (p.dqkv_h) {
            __bf16* dh_ = p.dqkv_h + (size_t)tok[wave * 16 + fq * 4 + e] * (3 * d) + h * hd;
            dh_[c] = (__bf16)(dq[jt][e] * scale);
            dh_[d + c] = (__bf16)dk[jt][e];
            dh_[2 * d + c] = (__bf16)dv[jt][e];
          } else {
            dst[c] = dq[jt][e] * scale;
            dst[d + c] = dk[jt][e];
            dst[2 * d + c] = dv[jt][e];
          }
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// All-bf16 form of the same backward, the training step's case: q (already scaled and rounded, exactly the operand the
// forward's MFMA took) | k | v and dO arrive as bf16 in per-head slots of hp columns, so a thread stages its share of a
// 32-column chunk with four 16-byte loads issued before anything else (it derives its row's token itself), and dq | dk | dv
// leave as bf16.  NCH = 32-column chunks of the head dim (1 .. 4).  With ONE chunk (head dim <= 32, DRCT-L's 30) the second
// operands of the three pass-B products are fetched (transposing LDS reads) right after pass A and the staging tiles are
// dead from then on: the fp32 dS copy the bias-table gradient sums is laid over them.  That brings the workgroup to 48.5 KB
// of LDS - three per CU, which for the 768 (window, head) pairs of the 8-image training batch is ONE resident round on
// 256 CUs instead of one and a half.  With more chunks pass B stages them again and the dS copy has its own 17 KB.
// ------------------------------------------------------------------------------------------
template <int NCH> constexpr size_t ag_lds_bytes() {
  return (size_t)(4 * 64 * AH_HS + 3 * 64 * AH_PS) * sizeof(__bf16) + 256 * sizeof(float) + 2 * 64 * sizeof(int) +
         (NCH > 1 ? (size_t)64 * 68 * sizeof(float) : 0);
}
static_assert((size_t)64 * 68 * sizeof(float) <= (size_t)4 * 64 * AH_HS * sizeof(__bf16), "the fp32 dS copy must fit in the staging tiles");

template <int NCH>
__global__ __launch_bounds__(256) void window_attn_bwd_h_kernel(const AttnBwdParams p, float* __restrict__ tpart) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __bf16* Qs = reinterpret_cast<__bf16*>(smem);          // [64][AH_HS] q * scale (32-column chunk)
  __bf16* Ks = Qs + 64 * AH_HS;
  __bf16* Vs = Ks + 64 * AH_HS;
  __bf16* Gs = Vs + 64 * AH_HS;                          // dO
  __bf16* Dm = Gs + 64 * AH_HS;                          // [query][key] dS
  __bf16* DmT = Dm + 64 * AH_PS;                         // [key][query] dS
  __bf16* PmT = DmT + 64 * AH_PS;                        // [key][query] P
  float* tbl = reinterpret_cast<float*>(PmT + 64 * AH_PS);   // [225] (256 reserved)
  int* tok = reinterpret_cast<int*>(tbl + 256);
  int* inf = tok + 64;
  // [64][68] fp32 dS: over Qs .. Gs once pass A is done with them (one chunk), else behind everything
  float* Df = NCH == 1 ? reinterpret_cast<float*>(smem) : reinterpret_cast<float*>(inf + 64);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int ws = 8, d = p.d, heads = p.heads, hd = d / heads, hp = p.hp_h;
  const int nWx = p.W / ws, nW = (p.H / ws) * nWx;
  int win, h;                                            // XCD k: window strip k (affinity with the row-tile kernels)
  attn_bwd_block_to_window(blockIdx.x, p.B * nW, heads, !p.no_xcd_map, win, h);
  const int b = win / nW, widx = win - b * nW;
  const int wy = widx / nWx, wx = widx - wy * nWx;
  const float scale = rsqrtf((float)hd);
  const int tw = 2 * ws - 1;

  // ---- staging: thread = (row tid / 4, 8 columns of the chunk), everything in flight before the first LDS store ----
  const int srow = tid >> 2, scl = (tid & 3) * 8;
  int stok, sinf;
  srad_window_token_info(p.H, p.W, ws, p.shift, b, wy, wx, srow / ws, srow % ws, stok, sinf);
  const __bf16* const qrow = p.qkv_h + (size_t)stok * (3 * heads * hp) + h * hp;
  const __bf16* const grow = p.dout_h + (size_t)stok * (heads * hp) + h * hp;
  u32x4 sq, sk, sv, sg;
  auto load_chunk = [&](int ch, bool need_v) __attribute__((always_inline)) {
    const int off = min(ch * 32 + scl, hp - 8);
    sq = *reinterpret_cast<const u32x4*>(qrow + off);
    sk = *reinterpret_cast<const u32x4*>(qrow + heads * hp + off);
    if (need_v) sv = *reinterpret_cast<const u32x4*>(qrow + 2 * heads * hp + off);
    sg = *reinterpret_cast<const u32x4*>(grow + off);
  };
  auto store_chunk = [&](int ch, bool need_v) __attribute__((always_inline)) {
    auto put = [&](__bf16* tile, const u32x4& raw) {        // columns at or beyond the head dim are zero in LDS
      bf16x8 v = __builtin_bit_cast(bf16x8, raw);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = ch * 32 + scl + e < hd ? v[e] : (__bf16)0.f;
      *reinterpret_cast<bf16x8*>(tile + srow * AH_HS + scl) = v;
    };
    put(Qs, sq); put(Ks, sk); if (need_v) put(Vs, sv); put(Gs, sg);
  };
  load_chunk(0, true);
  {
    const float tv = p.table[(size_t)min(tid, tw * tw - 1) * heads + h];
    if ((tid & 3) == 0) { tok[srow] = stok; inf[srow] = sinf; }
    tbl[tid] = tv;
  }
  store_chunk(0, true);
  __syncthreads();

  // ---- pass A: S = q k^T, dP = dO v^T (row = 16 wave + 4 fq + e, key = 16 j + fr) ----
  f32x4 s[4], dp[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) { s[j] = f32x4{0.f, 0.f, 0.f, 0.f}; dp[j] = f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    if (ch + 1 < NCH) load_chunk(ch + 1, true);             // the next chunk's rows are in flight over this chunk's MFMAs
    const bf16x8 a = *reinterpret_cast<const bf16x8*>(Qs + (wave * 16 + fr) * AH_HS + 8 * fq);
    const bf16x8 g = *reinterpret_cast<const bf16x8*>(Gs + (wave * 16 + fr) * AH_HS + 8 * fq);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bf16x8 kb = *reinterpret_cast<const bf16x8*>(Ks + (j * 16 + fr) * AH_HS + 8 * fq);
      const bf16x8 vb = *reinterpret_cast<const bf16x8*>(Vs + (j * 16 + fr) * AH_HS + 8 * fq);
      s[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, kb, s[j], 0, 0, 0);
      dp[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(g, vb, dp[j], 0, 0, 0);
    }
    if (ch + 1 < NCH) { __syncthreads(); store_chunk(ch + 1, true); __syncthreads(); }
  }
  // second operands of pass B: B[k = token kk + 8 fq + t][j = column 16 jt + fr] of the row-major tiles
  typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
  const int tq = fr >> 2, tp = fr & 3;
  auto tr8 = [&](const __bf16* tile, int kk, int jt) __attribute__((always_inline)) -> bf16x8 {
    const __bf16* r0 = tile + (kk + 8 * fq + tq) * AH_HS + jt * 16 + 4 * tp;
    const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(r0));
    const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(r0 + 4 * AH_HS));
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) { o[e] = lo[e]; o[4 + e] = hi[e]; }
    return o;
  };
  bf16x8 bK[2][2], bQ[2][2], bG[2][2];
  if constexpr (NCH == 1) {
#pragma unroll
    for (int k2 = 0; k2 < 2; ++k2)
#pragma unroll
      for (int jt = 0; jt < 2; ++jt) { bK[k2][jt] = tr8(Ks, 32 * k2, jt); bQ[k2][jt] = tr8(Qs, 32 * k2, jt); bG[k2][jt] = tr8(Gs, 32 * k2, jt); }
  } else {
    load_chunk(0, false);                                   // pass B walks the chunks again (k, q, dO): chunk 0 in flight over the softmax
  }

  // ---- softmax and dS in registers (their LDS reads are tbl / inf only) ----
  f32x4 pr[4], dsr[4];
  {
    int kinf[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) kinf[j] = inf[j * 16 + fr];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int row = wave * 16 + fq * 4 + e;
      const int qi = inf[row];
      const int qy = (qi >> 8) & 0xff, qx = qi & 0xff, qr = qi >> 16;
      float mx = -1e30f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int kyy = (kinf[j] >> 8) & 0xff, kxx = kinf[j] & 0xff, kr = kinf[j] >> 16;   // attn_bias_mask, written out (see there)
        float v = s[j][e] + tbl[(qy - kyy + ws - 1) * tw + (qx - kxx + ws - 1)];
        if (p.shift > 0 && qr != kr) v += -100.0f;
        s[j][e] = v;
        mx = fmaxf(mx, v);
      }
      mx = srad_row16_max(mx);
      float sum = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) { s[j][e] = __expf(s[j][e] - mx); sum += s[j][e]; }
      sum = srad_row16_sum(sum);
      const float inv = 1.0f / sum;
      float dl = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) { s[j][e] *= inv; dl += s[j][e] * dp[j][e]; }
      dl = srad_row16_sum(dl);
#pragma unroll
      for (int j = 0; j < 4; ++j) { pr[j][e] = s[j][e]; dsr[j][e] = s[j][e] * (dp[j][e] - dl); }
    }
  }
  __syncthreads();                                       // every wave has read the staging tiles: Df (one chunk) / chunk 0 may overwrite them
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int row = wave * 16 + fq * 4 + e;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      Dm[row * AH_PS + j * 16 + fr] = (__bf16)dsr[j][e];
      Df[row * 68 + j * 16 + fr] = dsr[j][e];
    }
  }
  // transposed tiles: this lane's four rows 4 fq .. 4 fq + 3 of query slab `wave` are consecutive along k
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    bf16x4 ph, dh;
#pragma unroll
    for (int e = 0; e < 4; ++e) { ph[e] = (__bf16)pr[j][e]; dh[e] = (__bf16)dsr[j][e]; }
    *reinterpret_cast<bf16x4*>(PmT + (j * 16 + fr) * AH_PS + wave * 16 + 4 * fq) = ph;
    *reinterpret_cast<bf16x4*>(DmT + (j * 16 + fr) * AH_PS + wave * 16 + 4 * fq) = dh;
  }
  if constexpr (NCH > 1) store_chunk(0, false);
  __syncthreads();

  // ---- pass B: dq = dS k, dk = dS^T q, dv = P^T dO, 32 columns at a time ----
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    if constexpr (NCH > 1) {
      if (ch + 1 < NCH) load_chunk(ch + 1, false);
#pragma unroll
      for (int k2 = 0; k2 < 2; ++k2)
#pragma unroll
        for (int jt = 0; jt < 2; ++jt) { bK[k2][jt] = tr8(Ks, 32 * k2, jt); bQ[k2][jt] = tr8(Qs, 32 * k2, jt); bG[k2][jt] = tr8(Gs, 32 * k2, jt); }
    }
    f32x4 dq[2], dk[2], dv[2];
#pragma unroll
    for (int jt = 0; jt < 2; ++jt) { dq[jt] = f32x4{0.f, 0.f, 0.f, 0.f}; dk[jt] = dq[jt]; dv[jt] = dq[jt]; }
#pragma unroll
    for (int k2 = 0; k2 < 2; ++k2) {
      const bf16x8 a_ds = *reinterpret_cast<const bf16x8*>(Dm + (wave * 16 + fr) * AH_PS + 32 * k2 + 8 * fq);
      const bf16x8 a_dst = *reinterpret_cast<const bf16x8*>(DmT + (wave * 16 + fr) * AH_PS + 32 * k2 + 8 * fq);
      const bf16x8 a_pt = *reinterpret_cast<const bf16x8*>(PmT + (wave * 16 + fr) * AH_PS + 32 * k2 + 8 * fq);
#pragma unroll
      for (int jt = 0; jt < 2; ++jt) {
        dq[jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_ds, bK[k2][jt], dq[jt], 0, 0, 0);
        dk[jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_dst, bQ[k2][jt], dk[jt], 0, 0, 0);
        dv[jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_pt, bG[k2][jt], dv[jt], 0, 0, 0);
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      __bf16* dst = p.dqkv_h + (size_t)tok[wave * 16 + fq * 4 + e] * (3 * d) + h * hd;
#pragma unroll
      for (int jt = 0; jt < 2; ++jt) {
        const int c = ch * 32 + jt * 16 + fr;
        if (c < hd) {
          dst[c] = (__bf16)(dq[jt][e] * scale);
          dst[d + c] = (__bf16)dk[jt][e];
          dst[2 * d + c] = (__bf16)dv[jt][e];
        }
      }
    }
    if constexpr (NCH > 1) {
      if (ch + 1 < NCH) { __syncthreads(); store_chunk(ch + 1, false); __syncthreads(); }
    }
  }
  table_grad_row_8x8(Df, 68, tid, tpart, win, heads, h);
}

}  // namespace

// windows other than 8 x 8: window_attn_bwd_gen_kernel (N = ws^2 <= 256) or window_attn_bwd_tiled_kernel (ws 32 and 64), fp32
// operands and results in every precision mode
static int launch_attn_bwd_gen(const AttnBwdParams& p, WgradQueue& q, hipStream_t stream) {
  const bool tiled = p.ws == 32 || p.ws == 64;
  SRAD_REQUIRE((p.ws >= 1 && p.ws <= 16) || tiled, "window_attn_bwd: window sizes 1 .. 16, 32 and 64 train (got %d)", p.ws);
  SRAD_REQUIRE(p.qkv && p.dout && p.dqkv && !p.qkv_h && !p.dqkv_h, "window_attn_bwd: window sizes other than 8 take fp32 q | k | v, dO and dqkv");
  SRAD_REQUIRE(p.d / p.heads <= 128, "window_attn_bwd: head dims up to 128 (got %d)", p.d / p.heads);
  // tokens are ints in the kernels (every product with a row length is formed in 64 bits), (window, head) pairs the grid
  SRAD_REQUIRE((double)p.B * p.H * p.W < 2147483648.0 && (double)p.B * p.H * p.W / (p.ws * p.ws) * p.heads < 2147483648.0,
               "window_attn_bwd: batch %d of %dx%d tokens is too large for 32-bit token numbers", p.B, p.H, p.W);
  const int nW = (p.H / p.ws) * (p.W / p.ws), tw = 2 * p.ws - 1;
  SRAD_REQUIRE((double)tw * tw * p.heads < 2147483648.0, "window_attn_bwd: %d heads of a %d x %d table overflow a row of partials", p.heads, tw, tw);
  const int ncols = tw * tw * p.heads, nwin = p.B * nW;
  float* tpart = nullptr;
  SRAD_TRY(srad_wgrad_reserve_colsum(q, "window_attn_bwd", p.dtable, ncols, ncols, nwin, 1.f, 1, stream, &tpart));
  const double T = (double)p.B * p.H * p.W;
  SradProfScope prof(stream, SRAD_K_ATTN_BWD, 10.0 * T * p.ws * p.ws * p.d, 4.0 * T * 8 * p.d);
  const int nb = (p.ws * p.ws + 63) / 64;
  const dim3 grid(nwin * p.heads), block(256);
  if (tiled) SRAD_TRY(srad_launch_dyn<window_attn_bwd_tiled_kernel>(grid, block, ABT_LDS(p.ws), stream, p, tpart));
  else if (nb == 1) SRAD_TRY(srad_launch_dyn<window_attn_bwd_gen_kernel<1>>(grid, block, ABG_LDS(1), stream, p, tpart));
  else if (nb == 2) SRAD_TRY(srad_launch_dyn<window_attn_bwd_gen_kernel<2>>(grid, block, ABG_LDS(2), stream, p, tpart));
  else if (nb == 3) SRAD_TRY(srad_launch_dyn<window_attn_bwd_gen_kernel<3>>(grid, block, ABG_LDS(3), stream, p, tpart));
  else SRAD_TRY(srad_launch_dyn<window_attn_bwd_gen_kernel<4>>(grid, block, ABG_LDS(4), stream, p, tpart));
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

int srad_launch_window_attn_bwd(int prec, const AttnBwdParams& p, WgradQueue& q, hipStream_t stream) {
  SRAD_REQUIRE(p.H % p.ws == 0 && p.W % p.ws == 0, "window_attn_bwd: %dx%d not a multiple of the window", p.H, p.W);
  SRAD_REQUIRE(p.d % p.heads == 0 && p.hdp % 4 == 0 && p.hdp >= p.d / p.heads, "window_attn_bwd: bad head geometry");
  SRAD_REQUIRE(p.shift >= 0 && p.shift < (p.ws > 0 ? p.ws : 1), "window_attn_bwd: bad shift %d", p.shift);
  if (p.ws != 8) return launch_attn_bwd_gen(p, q, stream);
  const int nW = (p.H / p.ws) * (p.W / p.ws);
  const double T = (double)p.B * p.H * p.W;
  const int ncols = 225 * p.heads, nwin = p.B * nW;
  float* tpart = nullptr;
  SRAD_TRY(srad_wgrad_reserve_colsum(q, "window_attn_bwd", p.dtable, ncols, ncols, nwin, 1.f, 1, stream, &tpart));
  SradProfScope prof(stream, SRAD_K_ATTN_BWD, 10.0 * T * 64 * p.d, 4.0 * T * 8 * p.d);
  const dim3 grid(p.B * nW * p.heads), block(256);
  if (prec == SRAD_PREC_BF16 && p.qkv_h) {
    const int hd = p.d / p.heads;
    SRAD_REQUIRE(p.dout_h && p.dqkv_h && hd <= 128 && p.hp_h % 8 == 0 && p.hp_h >= hd && p.hp_h <= 128 &&
                     (((uintptr_t)p.qkv_h | (uintptr_t)p.dout_h) & 15) == 0,
                 "window_attn_bwd: the all-bf16 form takes head dims <= 128 in 16-byte aligned slots of hp columns, and writes bf16");
    const int nch = (hd + 31) / 32;
    if (nch == 1) SRAD_TRY(srad_launch_dyn<window_attn_bwd_h_kernel<1>>(grid, block, ag_lds_bytes<1>(), stream, p, tpart));
    else if (nch == 2) SRAD_TRY(srad_launch_dyn<window_attn_bwd_h_kernel<2>>(grid, block, ag_lds_bytes<2>(), stream, p, tpart));
    else if (nch == 3) SRAD_TRY(srad_launch_dyn<window_attn_bwd_h_kernel<3>>(grid, block, ag_lds_bytes<3>(), stream, p, tpart));
    else SRAD_TRY(srad_launch_dyn<window_attn_bwd_h_kernel<4>>(grid, block, ag_lds_bytes<4>(), stream, p, tpart));
  } else if (prec == SRAD_PREC_BF16) {
    SRAD_TRY(srad_launch_dyn<window_attn_bwd_bf16_kernel>(grid, block, AH_LDS, stream, p, tpart));
  } else {
    SRAD_TRY(srad_launch_dyn<window_attn_bwd_kernel>(grid, block, AB_LDS, stream, p, tpart));
  }
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}
