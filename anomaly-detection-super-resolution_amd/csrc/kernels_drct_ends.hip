// kernels_drct_ends.hip - the end of the DRCT bf16 inference forward's body as one launch: final LayerNorm ->
// conv_after_body + feat0 -> conv_before_upsample -> LeakyReLU(0.01) into c2 (reference src/drct.py:881, 893-894).  One workgroup
// per 16 pixels of an LR row; it normalises the tile's 5 x 20 halo into LDS, computes conv_after_body on the tile's own 3 x 18
// halo (recomputed per tile, as swin_block recomputes k | v), keeps that c1 tile in LDS as bf16 and runs conv_before_upsample
// from it.  The rounding points are the chain's: LayerNorm output and c1 rounded to bf16 as MFMA operands, fp32 accumulation,
// biases and feat0 added in fp32.  (The stem was built as one launch too and taken out again: its gain was inside the
// run-to-run spread)
// Halo and c1 pixels are kept in ONE linear order, q = row * 20 + column: a tap (dy, dx) is the constant offset dy * 20 + dx in
// it, so the 16-row MFMA tiles of sw_mma_chunks walk it as they walk a token tile.  Columns 18, 19 of a c1 row and the rows
// past 60 are computed and never read.
#include "srad_common.h"
#include "swin_tiles.h"

namespace {

constexpr int DE_HALO_W = 20, DE_HALO_PIX = 100;   // the 5 x 20 LayerNorm halo of a 16-pixel tile
constexpr int DE_HALO_ROWS = 106;                  // ... and the rows the last c1 tile's taps reach (63 + 2 * 20 + 2), zeros
constexpr int DE_C1_ROWS = 64;                     // 3 x 20 c1 positions in four 16-row MFMA tiles
constexpr int DE_F = 64, DE_NT2 = DE_F / 16;       // conv_before_upsample's outputs
constexpr int DE_WAVES = 12, DE_THREADS = DE_WAVES * 64;
constexpr int DE_RED_BYTES = 9 * DE_NT2 * 64 * 16; // phase 2's partial sums, one slot per (tap, column tile, lane)
constexpr int DE_EP = 192;                         // E <= 192: twelve 16-column tiles

constexpr int de_ld(int KC) { return 32 * KC + 8; }                       // LDS row stride in elements (swin_tiles.h's bank rule)
constexpr int de_halo_bytes(int KC) {                                     // the halo region also holds the reduction buffer
  return DE_HALO_ROWS * de_ld(KC) * 2 > DE_RED_BYTES ? DE_HALO_ROWS * de_ld(KC) * 2 : DE_RED_BYTES;
}
constexpr int de_lds_bytes(int KC) { return de_halo_bytes(KC) + DE_C1_ROWS * de_ld(KC) * 2; }

// ---- packs ----
// conv weight [N][Cin][3][3] -> bf16 MFMA fragments [ceil(N / 16)][9 taps][KC = ceil(Cin / 32)] tiles of 1 KB (16 rows x 32 k,
// row-major inside: pack_weight_frag_kernel's tile), rows >= N and channels >= Cin zero
__global__ void pack_conv_frag_kernel(const float* __restrict__ src, __bf16* __restrict__ dst, int N, int Cin, int KC, size_t total) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int kin = (int)(i & 31), rin = (int)((i >> 5) & 15);
    const size_t tile = i >> 9;
    const int kc = (int)(tile % KC), tap = (int)(tile / KC % 9), nt = (int)(tile / ((size_t)KC * 9));
    const int n = nt * 16 + rin, c = kc * 32 + kin;
    dst[i] = (__bf16)((n < N && c < Cin) ? src[((size_t)n * Cin + c) * 9 + tap] : 0.f);
  }
}
__device__ __forceinline__ u32x2 de_bf16x4(const f32x4 v, bool keep) {
  bf16x4 h;
#pragma unroll
  for (int e = 0; e < 4; ++e) h[e] = (__bf16)v[e];
  const u32x2 u = __builtin_bit_cast(u32x2, h);
  return keep ? u : u32x2{0u, 0u};
}

// ---- body end ----
template <int KC>
__global__ __launch_bounds__(DE_THREADS) void drct_body_end_kernel(const DrctBodyEndParams p) {
  constexpr int LD = de_ld(KC), KW = 32 * KC, NI = (KW + 63) / 64;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __bf16* const halo = reinterpret_cast<__bf16*>(smem);                             // [DE_HALO_ROWS][LD]
  __bf16* const c1 = reinterpret_cast<__bf16*>(smem + de_halo_bytes(KC));           // [DE_C1_ROWS][LD]
  f32x4* const red = reinterpret_cast<f32x4*>(smem);                                // [9][DE_NT2][64], over the halo once it is dead
  const int lane = threadIdx.x & 63, fr = lane & 15, fq = lane >> 4, wave = threadIdx.x >> 6;
  const int H = p.H, W = p.W, E = p.E;
  const int row = blockIdx.x / p.tpr, x0 = (blockIdx.x - row * p.tpr) << 4;
  const int b = row / H, y = row - b * H;
  const f32x4 z4 = f32x4{0.f, 0.f, 0.f, 0.f};

  // ---- prologue: the halo's LayerNorm, 16 lanes per pixel (lane fr: channels 4 fr + 64 i), three passes of 48 pixels ----
  {
    f32x4 xv[3][NI], gv[NI], bv[NI];
    bool in[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int hp = j * 48 + wave * 4 + fq, hy = hp / DE_HALO_W, hx = hp - hy * DE_HALO_W;
      const int iy = y - 2 + hy, ix = x0 - 2 + hx;
      in[j] = hp < DE_HALO_PIX && iy >= 0 && iy < H && ix >= 0 && ix < W;
      const float* const src = p.X + ((size_t)(b * H + min(max(iy, 0), H - 1)) * W + min(max(ix, 0), W - 1)) * p.ldx;
#pragma unroll
      for (int i = 0; i < NI; ++i) xv[j][i] = *reinterpret_cast<const f32x4*>(src + min(4 * fr + 64 * i, E - 4));
    }
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      gv[i] = *reinterpret_cast<const f32x4*>(p.ln_g + min(4 * fr + 64 * i, E - 4));
      bv[i] = *reinterpret_cast<const f32x4*>(p.ln_b + min(4 * fr + 64 * i, E - 4));
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int hp = j * 48 + wave * 4 + fq;
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        xv[j][i] = 4 * fr + 64 * i < E ? xv[j][i] : z4;
        s += (xv[j][i][0] + xv[j][i][1]) + (xv[j][i][2] + xv[j][i][3]);
      }
      s = srad_row16_sum(s);
      const float mean = s / (float)E;
      float v = 0.f;
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        xv[j][i] = 4 * fr + 64 * i < E ? xv[j][i] - mean : z4;
        v += (xv[j][i][0] * xv[j][i][0] + xv[j][i][1] * xv[j][i][1]) + (xv[j][i][2] * xv[j][i][2] + xv[j][i][3] * xv[j][i][3]);
      }
      v = srad_row16_sum(v);
      const float rstd = rsqrtf(v / (float)E + 1e-5f);
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int c = 4 * fr + 64 * i;
        // pixels outside the image are conv_after_body's zero padding; the channels up to the chunk boundary are zeros too
        if (hp < DE_HALO_ROWS && c < KW)
          *reinterpret_cast<u32x2*>(halo + hp * LD + c) = de_bf16x4(xv[j][i] * rstd * gv[i] + bv[i], in[j] && c < E);
      }
    }
  }
  __syncthreads();

  // ---- phase 1: c1 = conv_after_body(halo) + bias + feat0 on the 3 x 20 positions; wave = 16-column tile of the E outputs ----
  const bool live = 16 * wave < E;
  const char* const w1 = reinterpret_cast<const char*>(p.w1);
  const size_t tile0 = (size_t)wave * 9 * KC;
  f32x4 acc[4] = {z4, z4, z4, z4};
  {
    u32x4 wr[3][KC];
    sw_load_tiles<KC>(wr[0], w1, live, tile0, fr, fq);
    sw_load_tiles<KC>(wr[1], w1, live, tile0 + KC, fr, fq);
    static_for<0, 9>([&](auto T) {
      constexpr int tap = decltype(T)::value;
      if constexpr (tap + 2 < 9) sw_load_tiles<KC>(wr[(tap + 2) % 3], w1, live, tile0 + (size_t)(tap + 2) * KC, fr, fq);
      sw_mma_chunks<2, 4>(halo + (fr + (tap / 3) * DE_HALO_W + tap % 3) * LD + 8 * fq, LD, KC, KC, wr[tap % 3], acc);
    });
  }
  // the epilogue's operands (activations first), then phase 2's weights: wave = tap, four column tiles x KC chunks
  const int ch = 16 * wave + 4 * fq;
  const bool chok = ch < E;
  f32x4 f0[4];
  bool ok[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int q = 16 * t + fr, r = q / DE_HALO_W, c = q - r * DE_HALO_W;
    const int iy = y - 1 + r, ix = x0 - 1 + c;
    ok[t] = r < 3 && c < 18 && iy >= 0 && iy < H && ix >= 0 && ix < W;
    f0[t] = *reinterpret_cast<const f32x4*>(p.feat0 + ((size_t)(b * H + min(max(iy, 0), H - 1)) * W + min(max(ix, 0), W - 1)) * E + min(ch, E - 4));
  }
  const f32x4 bias1 = *reinterpret_cast<const f32x4*>(p.b1 + min(ch, E - 4));
  const f32x4 bias2 = *reinterpret_cast<const f32x4*>(p.b2 + 16 * min(wave, DE_NT2 - 1) + 4 * fq);
  const int tap2 = min(wave, 8);
  u32x4 w2r[DE_NT2][KC];
#pragma unroll
  for (int nt = 0; nt < DE_NT2; ++nt)
    sw_load_tiles<KC>(w2r[nt], reinterpret_cast<const char*>(p.w2), wave < 9, (size_t)(nt * 9 + tap2) * KC, fr, fq);
  // c1 rounded to bf16, ZERO outside the image: conv_before_upsample pads c1, not the LayerNorm
  if (ch < KW) {
#pragma unroll
    for (int t = 0; t < 4; ++t) *reinterpret_cast<u32x2*>(c1 + (16 * t + fr) * LD + ch) = de_bf16x4(acc[t] + bias1 + f0[t], ok[t] && chok);
  }
  __syncthreads();

  // ---- phase 2: conv_before_upsample on the tile's 16 pixels, K split over the waves by tap ----
  {
    f32x4 a2[DE_NT2] = {z4, z4, z4, z4};
    const __bf16* const ar = c1 + (fr + (tap2 / 3) * DE_HALO_W + tap2 % 3) * LD + 8 * fq;
    bf16x8 af[KC];
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) af[kc] = *reinterpret_cast<const bf16x8*>(ar + kc * 32);
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) {
#pragma unroll
      for (int nt = 0; nt < DE_NT2; ++nt)
        a2[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, w2r[nt][kc]), af[kc], a2[nt], 0, 0, 0);
    }
    if (wave < 9) {
#pragma unroll
      for (int nt = 0; nt < DE_NT2; ++nt) red[(wave * DE_NT2 + nt) * 64 + lane] = a2[nt];
    }
  }
  __syncthreads();
  if (wave >= DE_NT2) return;
  f32x4 v = red[wave * 64 + lane];                                 // wave nt finishes column tile nt, taps in a fixed order
#pragma unroll
  for (int k = 1; k < 9; ++k) v += red[(k * DE_NT2 + wave) * 64 + lane];
  v += bias2;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : v[e] * 0.01f;
  const int x = x0 + fr;
  if (x < W) *reinterpret_cast<f32x4*>(p.Y + ((size_t)(b * H + y) * W + x) * DE_F + 16 * wave + 4 * fq) = v;
}

template <int KC>
int launch_body_end(const DrctBodyEndParams& p, dim3 grid, hipStream_t s) {
  return srad_launch_dyn<drct_body_end_kernel<KC>>(grid, dim3(DE_THREADS), (size_t)de_lds_bytes(KC), s, p);
}

}  // namespace

// The host-only rule (include/srad.h): shapes the kernel takes, and one round of 16-pixel tiles on the chip.  Measured at
// batch 8, 32 x 32 (two rounds on 256 CUs; tools/drct_ends_bench.py): 46.9 us against 63.7 us for the three
// launches, so a second round would still win at op level; the threshold stays at the default of one round until the
// anomaly-eval leg, the caller with such batches, has been measured with it.
extern "C" int srad_drct_ends_supported_cus(int prec, int E, int F, int C, int B, int H, int W, int cus) {
  if (prec != SRAD_PREC_BF16 || E < 4 || E % 4 || E > DE_EP || F != DE_F || (C != 1 && C != 3) || B < 1 || H < 1 || W < 1) return 0;
  return (long long)B * H * ((W + 15) / 16) <= cus;
}
extern "C" int srad_drct_ends_supported(int prec, int E, int F, int C, int B, int H, int W) {
  return srad_drct_ends_supported_cus(prec, E, F, C, B, H, W, srad_cu_count());
}

size_t srad_drct_conv_frag_bytes(int n, int cin) { return (size_t)((n + 15) / 16) * 9 * ((cin + 31) / 32) * 1024; }

int srad_launch_pack_conv_frag(const float* src, void* dst, int n, int cin, hipStream_t s) {
  const size_t total = srad_drct_conv_frag_bytes(n, cin) / 2;
  const int blocks = (int)((total + 255) / 256 > 2048 ? 2048 : (total + 255) / 256);
  SradProfScope prof(s, SRAD_K_PACK, 0.0, 36.0 * n * cin + 2.0 * total);
  hipLaunchKernelGGL(pack_conv_frag_kernel, dim3(blocks), dim3(256), 0, s, src, reinterpret_cast<__bf16*>(dst), n, cin, (cin + 31) / 32, total);
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

static bool de_al16(const void* q) { return ((uintptr_t)q & 15) == 0; }

int srad_launch_drct_body_end(const DrctBodyEndParams& q, hipStream_t s) {
  SRAD_REQUIRE(q.X && q.ln_g && q.ln_b && q.w1 && q.b1 && q.feat0 && q.w2 && q.b2 && q.Y, "drct_body_end: null argument");
  SRAD_REQUIRE(q.E >= 4 && q.E % 4 == 0 && q.E <= DE_EP, "drct_body_end: E = %d must be a multiple of 4, at most %d", q.E, DE_EP);
  SRAD_REQUIRE(q.B >= 1 && q.H >= 1 && q.W >= 1, "drct_body_end: empty map %d x %d x %d", q.B, q.H, q.W);
  SRAD_REQUIRE(q.ldx >= q.E && q.ldx % 4 == 0 && de_al16(q.X) && de_al16(q.ln_g) && de_al16(q.ln_b) && de_al16(q.b1) && de_al16(q.b2) &&
                   de_al16(q.feat0) && de_al16(q.w1) && de_al16(q.w2) && de_al16(q.Y),
               "drct_body_end: rows and vectors must be 16-byte aligned (ldx = %d)", q.ldx);
  DrctBodyEndParams p = q;
  p.tpr = (p.W + 15) / 16;
  SRAD_REQUIRE((int64_t)p.B * p.H * p.tpr < (1LL << 31) && (int64_t)p.B * p.H * p.W < (1LL << 31) / 64, "drct_body_end: too many tiles");
  const dim3 grid((unsigned)(p.B * p.H * p.tpr));
  const double T = (double)p.B * p.H * p.W;
  SradProfScope prof(s, SRAD_K_BODY_END, 2.0 * T * 9 * p.E * (p.E + DE_F), 4.0 * T * (2 * p.E + DE_F) + 18.0 * p.E * (p.E + DE_F));
  switch ((p.E + 31) / 32) {
    case 1: SRAD_TRY(launch_body_end<1>(p, grid, s)); break;
    case 2: SRAD_TRY(launch_body_end<2>(p, grid, s)); break;
    case 3: SRAD_TRY(launch_body_end<3>(p, grid, s)); break;
    case 4: SRAD_TRY(launch_body_end<4>(p, grid, s)); break;
    case 5: SRAD_TRY(launch_body_end<5>(p, grid, s)); break;
    default: SRAD_TRY(launch_body_end<6>(p, grid, s)); break;
  }
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

// ---- the launch on raw fp32 weights, packed into caller scratch (include/srad.h) ----
extern "C" {

size_t srad_op_drct_ends_scratch_bytes(int E, int F) {
  if (E < 1 || F < 1) return 0;
  return srad_align_up(srad_drct_conv_frag_bytes(E, E), 256) + srad_align_up(srad_drct_conv_frag_bytes(F, E), 256);
}

int srad_op_drct_body_end(const float* x, int ldx, int B, int H, int W, int E, int F, const float* ln_g, const float* ln_b, const float* w1,
                          const float* b1, const float* feat0, const float* w2, const float* b2, float* c2, void* scratch,
                          size_t scratch_bytes, void* stream) {
  SRAD_REQUIRE(x && ln_g && ln_b && w1 && b1 && feat0 && w2 && b2 && c2 && scratch, "op_drct_body_end: null argument");
  SRAD_REQUIRE(E >= 4 && E % 4 == 0 && E <= DE_EP, "op_drct_body_end: E = %d must be a multiple of 4, at most %d", E, DE_EP);
  SRAD_REQUIRE(F == DE_F, "op_drct_body_end: F = %d must be %d", F, DE_F);
  SRAD_REQUIRE(B >= 1 && H >= 1 && W >= 1, "op_drct_body_end: empty map %d x %d x %d", B, H, W);
  SRAD_REQUIRE(ldx >= E && ldx % 4 == 0 && de_al16(x) && de_al16(feat0) && de_al16(c2) && de_al16(ln_g) && de_al16(ln_b) && de_al16(b1) && de_al16(b2),
               "op_drct_body_end: rows and vectors must be 16-byte aligned (ldx = %d)", ldx);
  const size_t n1 = srad_align_up(srad_drct_conv_frag_bytes(E, E), 256), n2 = srad_align_up(srad_drct_conv_frag_bytes(F, E), 256);
  SRAD_REQUIRE(scratch_bytes >= n1 + n2 && ((uintptr_t)scratch & 255) == 0, "op_drct_body_end: scratch %zu bytes, %zu needed (256-byte aligned)",
               scratch_bytes, n1 + n2);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  char* const sc = reinterpret_cast<char*>(scratch);
  SRAD_TRY(srad_launch_pack_conv_frag(w1, sc, E, E, s));
  SRAD_TRY(srad_launch_pack_conv_frag(w2, sc + n1, F, E, s));
  DrctBodyEndParams p{};
  p.X = x; p.ldx = ldx; p.ln_g = ln_g; p.ln_b = ln_b; p.w1 = sc; p.w2 = sc + n1; p.b1 = b1; p.b2 = b2; p.feat0 = feat0; p.Y = c2;
  p.B = B; p.H = H; p.W = W; p.E = E;
  return srad_launch_drct_body_end(p, s);
}

}  // extern "C"
