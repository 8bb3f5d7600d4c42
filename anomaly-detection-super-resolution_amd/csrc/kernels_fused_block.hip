// kernels_fused_block.hip - a whole DRCT Swin block + the RDG's adjust conv as ONE bf16 launch (window 8, inference):
//
//   xn   = LayerNorm1(x[window tokens]);  q|k|v = xn . Wqkv^T + b              (src/drct.py:477, 278)
//   a    = softmax(q*scale k^T + rel-pos bias + shift mask) v                   (src/drct.py:281-299)
//   x1   = x + proj(a) + b_proj;  x2 = x1 + fc2(GELU(fc1(LayerNorm2(x1))))      (src/drct.py:300, 509-510, 184-190)
//   out  = act(adjust(x2) + b_adj) * alpha (+ R)                                (src/drct.py:389-396)
//
// i.e. qkv_attn_kernel followed by mlp_block_kernel<16> without the launch boundary and without the attention output's trip
// through HBM.  A workgroup owns a QUARTER of a window: its 16 query tokens (window rows 2q, 2q + 1) are the 16-row tile of
// the MLP half, so 64 windows x 4 quarters fill 256 CUs.  Each workgroup gathers and normalises all 64 rows of its window and
// projects k and v of every head for them (redundantly with its three siblings - on a matrix pipe the two-kernel form leaves
// 80-95 % idle); q is projected for its own row tile only.  A wave then owns one head: scores, bias + mask, softmax and P.V of
// 16 queries x 64 keys stay inside the wave (no barrier between them), and the result lands as the bf16 A tile of the proj
// GEMM in LDS.  The weights of all five matrices stream through ONE sequence of register-set stages (three ahead, as in the
// two kernels), so the first MLP stages are in flight under the attention.  Head rows are stored at the smallest stride that
// keeps the bank rule (48 / 80 elements for the 46- / 77-wide heads of d = 276 / 308), so k | v of all heads fit next to the
// window tile at every d.
//
// FOLD form (inference; mlp_fold.h): x2 is read by the adjust conv alone and nothing non-linear sits between, so
//   out  = act([A | A W2] . [x1 | h] + (A b2 + b_a)) * alpha (+ R),   h = GELU(fc1(LayerNorm2(x1)))
// replaces the last two lines: no fc2 phase, no x2, one barrier less, and x1 leaves the registers after the proj epilogue.
//
// Write hazard: adjust_k (k < 4) writes columns [d, d + no) of its 16 rows into the same dense buffer whose columns [0, d)
// other workgroups of this launch still read.  d % 4 == 0, every access is a float4 on a 4-column boundary, so no access
// straddles the two ranges.  adjust5 writes the other dense buffer.
//
// The tile geometry, the MLP stage decode, the transposed V read and the chunk-grouped MFMA loop are swin_tiles.h's, shared
// with the two kernels.  What else the kernels have in common is written out here, each with a note why (through
// the shared form this kernel or mlp_block_kernel ran slower).  Same rules as there: unconditional loads on clamped addresses,
// activations ahead of weights, padding zeroed by selects, stage geometry in template parameters (no runtime-indexed register
// arrays: no scratch), LDS row strides of 2 mod 4 sixteen-byte units.
#include "swin_tiles.h"

namespace {

// Stage counts and the LDS layout of one instance.  HDT = ceil(head_dim / 16), KC = ceil(d / 32).
template <int HDT, int KC, int HEADS>
struct BlkGeo {
  static constexpr int HDP = 16 * HDT, LDX = KC * 32 + 16;
  // head row stride: the smallest multiple of 8 elements >= HDP whose count of 16-byte units is 2 mod 4 (32 -> 48, 48 -> 48,
  // 64 -> 80, 80 -> 80, 128 -> 144)
  static constexpr int HS = (HDP / 8 + (6 - HDP / 8 % 4) % 4) * 8;
  static_assert(HS >= HDP && HS % 8 == 0 && HS / 8 % 4 == 2, "head rows keep the bank rule");
  static constexpr int NKVT = HEADS * 2 * HDT, NQT = HEADS * HDT;  // 16-column tiles of k | v (x 4 row tiles) and of q (x 1)
  static constexpr int NKVS = (NKVT + 7) / 8, NQS = (NQT + 7) / 8; // column stages: one tile per wave
  static constexpr int QS = NKVS + NQS;                            // weight stages of the attention half: a stage spans all KC k chunks
  // bytes
  static constexpr int XN_B = 64 * LDX * 2, KV_B = 2 * HEADS * 64 * HS * 2, Q_B = HEADS * 16 * HS * 2, PS_B = HEADS * 16 * SW_LDP * 2;
  static constexpr int A1_B = 16 * SW_LDA * 2, HS_B = 16 * SW_LDH * 2;
  // the normalised window is dead once q | k | v exist, so the probabilities (and the attention tile, if both fit) overlay it
  static constexpr bool A1_OVER = PS_B + A1_B <= XN_B;
  static constexpr int OFF_KV = XN_B, OFF_Q = OFF_KV + KV_B;
  static constexpr int OFF_A1 = A1_OVER ? PS_B : OFF_Q + Q_B;
  static constexpr int OFF_PS = 0;
  static constexpr int OFF_VEC = A1_OVER ? OFF_Q + Q_B : OFF_A1 + A1_B;
  static constexpr int NBIAS = HEADS * 3 * HDP, NTBL = 225 * HEADS, NTBLP = (NTBL + 3) & ~3;
  // floats: MLP vectors | gamma1 320 | beta1 320 | qkv bias | table | LayerNorm2 partial sums [16][8][2] | softmax sums [HEADS][16]
  static constexpr int NFLT = SW_NV + 640 + NBIAS + NTBLP + 256 + 128;
  static constexpr int LDS = OFF_VEC + NFLT * 4 + 64 * 4;          // + window geometry words [64]
  static_assert(KV_B >= HS_B, "the hidden tile overlays k | v");
  static_assert(LDS <= 160 * 1024, "swin_block: LDS budget");
};

// GD .. KCM: the stage geometry of the MLP half, as mlp_block_kernel's (KCD == KC)
// FOLD: the folded second half (mlp_fold.h) - p.w_adj is the pack of [A | A W2], p.b_adj is A b2 + b_a, and
// p.w_fc2 is not read: proj | fc1 | adjF, no fc2 phase and no x2
template <int HDT, int KC, int HEADS, int GD, int KGD, int GM, int KGM, int GN, int KCM, bool FOLD>
__global__ __launch_bounds__(512) void swin_block_kernel(const SwinBlockParams p) {
  using G = BlkGeo<HDT, KC, HEADS>;
  constexpr int KCD = KC;
  constexpr int HDP = G::HDP, HS = G::HS, LDX = G::LDX;
  constexpr int RC = KC > 8 ? KC : 8;                                    // fragment registers per weight set: a W_qkv stage holds all
                                                                         // KC (<= 10) chunks of its tile, an MLP stage up to 8
  constexpr int NKVS = G::NKVS, QS = G::QS;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __bf16* XN = reinterpret_cast<__bf16*>(smem);                          // [64][LDX] LayerNorm1(window)
  __bf16* KV = reinterpret_cast<__bf16*>(smem + G::OFF_KV);              // [k | v][HEADS][64][HS]
  __bf16* Qb = reinterpret_cast<__bf16*>(smem + G::OFF_Q);               // [HEADS][16][HS] (scaled)
  __bf16* A1 = reinterpret_cast<__bf16*>(smem + G::OFF_A1);              // [16][SW_LDA] attention output -> LN2(x1) -> x2
  __bf16* Ps = reinterpret_cast<__bf16*>(smem + G::OFF_PS);              // [HEADS][16][SW_LDP] probabilities
  __bf16* Hs = KV;                                                       // [16][SW_LDH] GELU(fc1): k | v are dead by then
  // FOLD: adjF's A tile instead, [16][LDF] = bf16(x1) in k chunks [0, KC) | GELU(fc1) in chunks [KC, KC + KCM), one k range
  constexpr int KF = KC + KCM, LDF = KF * 32 + 16;                       // (row stride: 2 mod 4 sixteen-byte units)
  constexpr bool SPLITK = FOLD && GN == 1;                               // adjust outputs <= 32: k split over the eight waves
  static_assert(!FOLD || 16 * LDF * 2 <= G::KV_B, "the folded A tile overlays k | v");
  static_assert(!SPLITK || 4 * 2 * 16 * 16 * 4 <= G::A1_B, "the k parts' partial sums overlay the LayerNorm2 tile");
  [[maybe_unused]] __bf16* Ft = KV;
  float* vec = reinterpret_cast<float*>(smem + G::OFF_VEC);
  float* v_g1 = vec + SW_NV;                                              // [320] gamma1
  float* v_b1n = v_g1 + 320;                                             // [320] beta1
  float* v_bias = v_b1n + 320;                                           // [HEADS][3][HDP] q|k|v bias (0 in padding)
  float* tbl = v_bias + G::NBIAS;                                        // [225][HEADS] relative position bias
  float* red = tbl + G::NTBLP;                                           // [16][8][2] LayerNorm2 partial sums
  float* lsum = red + 256;                                               // [HEADS][16] softmax denominators
  int* inf = reinterpret_cast<int*>(lsum + 128);                         // [64] (region << 16) | (py << 8) | px

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int wave_s = __builtin_amdgcn_readfirstlane(wave);
  const int d = p.d, m = p.m, no = p.no, hd = d / HEADS;
  const float scale = rsqrtf((float)hd);
  // grid = (windows, 4 quarters): a window's four workgroups have linear ids that differ by the window count, a multiple of 8
  // where the XCD-affine mapping applies, so they share an XCD (and its L2 copy of the window's rows and of the weights)
  const int quarter = blockIdx.y;
  // (qkv_attn_kernel's sw_window, written out: through the helper d = 180 / 212 ran 0.02 - 0.08 us slower)
  int win = blockIdx.x;
  if ((gridDim.x & 7) == 0 && !p.no_xcd_map) win = (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
  const int ws = 8, nWx = p.W / ws, nW = (p.H / ws) * nWx;
  const int b = win / nW, widx = win - b * nW;
  const int wy = widx / nWx, wx = widx - wy * nWx;
  auto token_of = [&](int t, int& info) {
    int token;
    srad_window_token_info(p.H, p.W, ws, p.shift, b, wy, wx, t >> 3, t & 7, token, info);
    return token;
  };
  const int xrow = tid >> 3, col4 = tid & 7;
  int info;
  const int my_tok = token_of(xrow, info);                        // the window row this thread gathers
  const int row_tok = token_of(16 * quarter + fr, info);          // the tile row this lane owns in the MLP half
  if (tid < 64) {
    token_of(tid, info);
    inf[tid] = info;
  }

  using Chain = std::conditional_t<FOLD, MlpFoldChain<GD, KGD, GM, GN, KCD, KCM, SPLITK>, MlpChain<GD, KGD, GM, KGM, GN, KCD, KCM>>;
  constexpr int n_mlp = Chain::n_stages;
  constexpr int n_all = QS + n_mlp;
  float* const v_bp = vec; float* const v_bf1 = vec + SW_V_B1; float* const v_bf2 = vec + SW_V_B2; float* const v_ba = vec + SW_V_BA;
  float* const v_g2 = vec + SW_V_G; float* const v_b2n = vec + SW_V_B;

  // the 16-column tile of q | k | v this wave owns in column stage cs: head, slice (0 q, 1 k, 2 v), column tile of the
  // slice, liveness
  struct QTile { int hl, which, ct; bool live; };
  auto qtile = [&](int cs) -> QTile {
    if (cs < NKVS) {
      const int j = cs * 8 + wave_s, hl = j / (2 * HDT), r = j - hl * 2 * HDT;
      return QTile{hl, 1 + r / HDT, r % HDT, j < G::NKVT};
    }
    const int j = (cs - NKVS) * 8 + wave_s, hl = j / HDT;
    return QTile{hl, 0, j - hl * HDT, j < G::NQT};
  };
  // ---- ONE weight stream for the whole block: stages [0, QS) are the per-head fragment tiles of W_qkv (a wave owns 16 virtual
  //      columns of a stage and nobody else reads their weights), stages [QS, n_all) those of proj | fc1 | fc2 | adjust exactly
  //      as in mlp_block_kernel.  Straight from global memory into MFMA operand registers, three stages ahead. ----
  constexpr int NSETS = 3;
  u32x4 w_reg[NSETS][RC];
  auto load_w = [&](auto S, u32x4 (&reg)[RC]) __attribute__((always_inline)) {
    constexpr int u = decltype(S)::value < n_all - 1 ? decltype(S)::value : n_all - 1;
    if constexpr (u < QS) {
      const QTile t = qtile(u);
      const char* const Wq = reinterpret_cast<const char*>(p.w_qkv);
      const int gt = (t.hl * 3 + t.which) * HDT + t.ct;                       // tile row of the pack: [head][q | k | v][HDT]
      // (sw_load_tiles written out: through the helper all five instances compile differently)
      const char* base = t.live ? Wq + (size_t)gt * KC * 1024 + fr * 64 + fq * 16 : Wq;
      const int step = t.live ? 1024 : 0;
#pragma unroll
      for (int cc = 0; cc < KC; ++cc) reg[cc] = *reinterpret_cast<const u32x4*>(base + cc * step);
    } else if constexpr (SPLITK && Chain::stage(u - QS).ph == 3) {
      // adjF's one stage: column tile wave & 1 (the pack's rows are padded to 128: both tiles exist), k part wave >> 1; a
      // part that ends past the last chunk reloads that chunk (the MFMA loop zeroes its operand)
      constexpr MlpStage sg = Chain::stage(u - QS);
      const char* base = (const char*)p.w_adj + (size_t)(wave_s & 1) * sg.kc * 1024 + fr * 64 + fq * 16;
      const int p0 = (wave_s >> 1) * sg.nch;
#pragma unroll
      for (int cc = 0; cc < sg.nch; ++cc) reg[cc] = *reinterpret_cast<const u32x4*>(base + (size_t)min(p0 + cc, sg.kc - 1) * 1024);
    } else {
      constexpr MlpStage sg = Chain::stage(u - QS);
      const char* w = (const char*)(sg.ph == 0 ? p.w_proj : (sg.ph == 1 ? p.w_fc1 : (sg.ph == 2 ? p.w_fc2 : p.w_adj)));
      const int nreal = sg.ph == 0 ? d : (sg.ph == 1 ? m : (sg.ph == 2 ? d : no));
      const bool live = (sg.g * 8 + wave_s) * 16 < nreal;
      const char* base = live ? w + ((size_t)(sg.g * 8 + wave) * sg.kc + sg.kg * 8) * 1024 + fr * 64 + fq * 16 : w;
      const int step = live ? 1024 : 0;
#pragma unroll
      for (int cc = 0; cc < sg.nch; ++cc) reg[cc] = *reinterpret_cast<const u32x4*>(base + cc * step);
    }
  };

  // ---- loads in the order their data is needed: the window's rows, the tile's shortcut quads, the vectors, the first stage ----
  f32x4 a_reg[KC];
  {
    const char* src = reinterpret_cast<const char*>(p.x) + (size_t)my_tok * p.ldx * 4;
#pragma unroll
    for (int j = 0; j < KC; ++j) a_reg[j] = *reinterpret_cast<const f32x4*>(src + (unsigned)min(j * 32 + col4 * 4, d - 4) * 4u);
  }
  // accumulator layout of this lane in the MLP half: token row fr of the tile, columns 128 g + 16 wave + 4 fq + (0..3)
  f32x4 x1[GD];
#pragma unroll
  for (int g = 0; g < GD; ++g)
    x1[g] = *reinterpret_cast<const f32x4*>(p.x + (size_t)row_tok * p.ldx + min(SW_SC * g + 16 * wave + 4 * fq, d - 4));
  typedef const float __attribute__((address_space(1)))* gfloat_p;
  float g1q, b1q, biasq[2], tblq[3];
  {
    const int e = min(tid, d - 1);
    g1q = ((gfloat_p)p.ln1_g)[e]; b1q = ((gfloat_p)p.ln1_b)[e];
    // (the qkv-bias staging is ln_qkv_kernel's, written out in both: as a helper it changes all ten ln_qkv instances)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int idx = min(tid + 512 * q, G::NBIAS - 1);
      const int slice = idx / HDP, c = idx - slice * HDP, hh = slice / 3, which = slice - 3 * hh;
      biasq[q] = ((gfloat_p)p.b_qkv)[which * d + hh * hd + min(c, hd - 1)];
      if (c >= hd) biasq[q] = 0.f;
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) tblq[q] = ((gfloat_p)p.table)[min(tid + 512 * q, G::NTBL - 1)];
  }
  // the MLP vectors into their slots (SW_V_*)
  f32x4 vq[2];
  int v_off = 0, v_len = 0;
  {
    const float* src = p.b_proj; int n = d;
    if (wave_s == 1) { src = p.b_fc1; n = m; v_off = SW_V_B1; }
    else if (wave_s == 2) { src = p.b_fc2; n = d; v_off = SW_V_B2; }
    else if (wave_s == 3) { src = p.b_adj; n = no; v_off = SW_V_BA; }
    else if (wave_s == 4) { src = p.ln2_g; n = d; v_off = SW_V_G; }
    else if (wave_s == 5) { src = p.ln2_b; n = d; v_off = SW_V_B; }
    v_len = wave_s == 1 ? SW_VM : SW_VD;
    vq[0] = *reinterpret_cast<const f32x4*>(src + min(4 * lane, n - 4));
    vq[1] = *reinterpret_cast<const f32x4*>(src + min(256 + 4 * lane, n - 4));
  }
  load_w(std::integral_constant<int, 0>{}, w_reg[0]);
  if (tid < 320) { v_g1[tid] = tid < d ? g1q : 0.f; v_b1n[tid] = tid < d ? b1q : 0.f; }
#pragma unroll
  for (int q = 0; q < 2; ++q)
    if (tid + 512 * q < G::NBIAS) v_bias[tid + 512 * q] = biasq[q];
#pragma unroll
  for (int q = 0; q < 3; ++q)
    if (tid + 512 * q < G::NTBL) tbl[tid + 512 * q] = tblq[q];
  if (wave_s < 6) {
    *reinterpret_cast<f32x4*>(vec + v_off + 4 * lane) = vq[0];
    if (256 + 4 * lane < v_len) *reinterpret_cast<f32x4*>(vec + v_off + 256 + 4 * lane) = vq[1];
  }
  // ---- LayerNorm1 from the registers (the 8 lanes of a row hold all its columns) -> bf16 -> XN ----
  // (written out in each of its three kernels: with the statistics in a swin_tiles.h helper the d = 276 / 308 instances go from
  // 178 / 190 to 188 / 204 VGPRs)
  {
    float s = 0.f, ss = 0.f;
#pragma unroll
    for (int j = 0; j < KC; ++j) {
      const bool in = j * 32 + col4 * 4 < d;
      const f32x4 v = in ? a_reg[j] : f32x4{0.f, 0.f, 0.f, 0.f};
      s += (v[0] + v[1]) + (v[2] + v[3]);
      ss += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
    }
    { s = srad_row8_sum(s); ss = srad_row8_sum(ss); }
    const float mu = s / (float)d;
    const float rstd = rsqrtf(fmaxf(ss / (float)d - mu * mu, 0.f) + 1e-5f);
    __syncthreads();                                              // vectors / table / window geometry staged
#pragma unroll
    for (int j = 0; j < KC; ++j) {
      const int c = j * 32 + col4 * 4;
      const f32x4 g4 = *reinterpret_cast<const f32x4*>(v_g1 + c);
      const f32x4 b4 = *reinterpret_cast<const f32x4*>(v_b1n + c);
      const f32x4 v = c < d ? (a_reg[j] - mu) * rstd * g4 + b4 : f32x4{0.f, 0.f, 0.f, 0.f};
      bf16x4 hh;
      hh[0] = (__bf16)v[0]; hh[1] = (__bf16)v[1]; hh[2] = (__bf16)v[2]; hh[3] = (__bf16)v[3];
      *reinterpret_cast<bf16x4*>(XN + xrow * LDX + c) = hh;
    }
  }
  static_for<1, NSETS>([&](auto Q) { load_w(Q, w_reg[decltype(Q)::value]); });   // the rest of the weight look-ahead
  __syncthreads();                                                // the normalised window is in LDS

  // ================================================== attention half ==================================================
  // ---- q|k|v = xn . W^T : one 16-column tile per wave and stage, transposed result (lane: token fr of row tile t, 4 columns);
  //      k | v tiles for all four row tiles, q tiles for this workgroup's row tile only ----
  // (a lambda of its own, as the head-group loop was: with its temporaries scoped like this the d = 180 / 212 / 244 instances
  // compile to the instruction streams they had)
  [&]() __attribute__((always_inline)) {
    f32x4 ac[4];
    static_for<0, QS>([&](auto LS) {
      constexpr int cs = decltype(LS)::value, S = cs;
      constexpr bool isq = cs >= NKVS;
      constexpr int NT = isq ? 1 : 4;
      constexpr int nch = KC;
      u32x4 (&reg)[RC] = w_reg[S % NSETS];
      const QTile t = qtile(cs);
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) ac[tt] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (t.live) {
        const __bf16* ar = XN + ((isq ? 16 * quarter : 0) + fr) * LDX + 8 * fq;
        // the window fragments of two chunks (q: of all chunks) are requested together, THEN multiplied (see qkv_attn_kernel)
        sw_mma_chunks<isq ? KC : 2, NT>(ar, LDX, nch, nch, reg, ac);
      }
      load_w(std::integral_constant<int, S + NSETS>{}, reg);
      // bias, the attention's scale on q, zero padding -> the bf16 tiles the attention reads
      if (t.live) {
        const int c = t.ct * 16 + 4 * fq;
        const f32x4 bias = *reinterpret_cast<const f32x4*>(v_bias + (t.hl * 3 + t.which) * HDP + c);
        __bf16* dst = isq ? Qb + (t.hl * 16 + fr) * HS + c : KV + (((t.which - 1) * HEADS + t.hl) * 64 + fr) * HS + c;
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) {
          f32x4 v = ac[tt] + bias;
          if constexpr (isq) v = v * scale;
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = c + e < hd ? v[e] : 0.f;
          bf16x4 hh;
#pragma unroll
          for (int e = 0; e < 4; ++e) hh[e] = (__bf16)v[e];
          *reinterpret_cast<bf16x4*>(dst + tt * 16 * HS) = hh;
        }
      }
    });
    __syncthreads();                                              // q, k, v complete: the window tile is dead
    {
      // columns [d, 32 KC) of the attention tile: the proj GEMM's k padding
      const int row = tid >> 5, c = d + (tid & 31);
      if (c < KC * 32) A1[row * SW_LDA + c] = (__bf16)0.f;
    }
    // ---- one head per wave: S = q k^T + bias + mask, softmax, O = P V for this tile's 16 queries against the window's 64 keys ----
    if (wave_s < HEADS) {
      const int h = wave_s;
      const __bf16* Qs = Qb + h * 16 * HS;
      const __bf16* Ks = KV + h * 64 * HS;
      const __bf16* Vs = KV + (HEADS + h) * 64 * HS;
      __bf16* Pw = Ps + h * 16 * SW_LDP;
      f32x4 sc[4];
      // relative position bias + 0 / -100 shift mask (drct.py:284-292, 449-470) of the lane's 16 (key, query) pairs
      // (qkv_attn_kernel's sw_bias_mask, written out: with it and sw_window the step ran 0.1 - 0.2 % slower)
      {
        int qi[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) qi[e] = inf[16 * quarter + 4 * fq + e];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int ki = inf[j * 16 + fr], ky = (ki >> 8) & 0xff, kx = ki & 0xff, kr = ki >> 16;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int qy = (qi[e] >> 8) & 0xff, qx = qi[e] & 0xff, qr = qi[e] >> 16;
            float v = tbl[((qy - ky + 7) * 15 + (qx - kx + 7)) * HEADS + h];
            if (p.shift > 0 && qr != kr) v += -100.0f;
            sc[j][e] = v;
          }
        }
      }
      f32x4 s4[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) s4[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < HDP; kk += 32) {
        // head dims padded to 48 / 80: the last 32-wide step has 16 real columns and the row ends there.  The lanes of the upper
        // half (fq >= 2) load a clamped column of the same row and get zeros in both operands.
        const bool half = kk + 32 > HDP, cut = half && fq >= 2;
        const int col = kk + 8 * (half ? fq & 1 : fq);
        const bf16x8 zero = {(__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f};
        bf16x8 a = *reinterpret_cast<const bf16x8*>(Qs + fr * HS + col);
        a = cut ? zero : a;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          bf16x8 bb = *reinterpret_cast<const bf16x8*>(Ks + (j * 16 + fr) * HS + col);
          bb = cut ? zero : bb;
          s4[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bb, s4[j], 0, 0, 0);
        }
      }
      // lane: queries 4 fq + e (e = 0..3) of the tile, keys 16 j + fr
#pragma unroll
      for (int j = 0; j < 4; ++j) s4[j] += sc[j];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float mx = srad_row16_max(fmaxf(fmaxf(s4[0][e], s4[1][e]), fmaxf(s4[2][e], s4[3][e])));
        float pr[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) pr[j] = __expf(s4[j][e] - mx);
        const float rs = srad_row16_sum(pr[0] + pr[1]) + srad_row16_sum(pr[2] + pr[3]);   // the two key halves, as qkv_attn_kernel sums them
        if (fr == 0) lsum[h * 16 + 4 * fq + e] = rs;
#pragma unroll
        for (int j = 0; j < 4; ++j) Pw[(4 * fq + e) * SW_LDP + j * 16 + fr] = (__bf16)pr[j];
      }
      __builtin_amdgcn_wave_barrier();                            // P and the sums are this wave's own: LDS keeps a wave's accesses in order
      const float inv = 1.0f / lsum[h * 16 + fr];
      const int tq = fr >> 2, tp = fr & 3;
#pragma unroll
      for (int j = 0; j < HDT; ++j) {
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 64; kk += 32) {
          const bf16x8 pa = *reinterpret_cast<const bf16x8*>(Pw + fr * SW_LDP + kk + 8 * fq);
          const bf16x8 vb = sw_read_v_tr(Vs + (kk + 8 * fq + tq) * HS + j * 16 + 4 * tp, HS);
          o = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vb, pa, o, 0, 0, 0);
        }
        // transposed result: token fr of the tile, columns 16 j + 4 fq + e of the head -> the proj GEMM's A tile
        __bf16* dst = A1 + fr * SW_LDA + h * hd;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = j * 16 + 4 * fq + e;
          if (c < hd) dst[c] = (__bf16)(o[e] * inv);
        }
      }
    }
  }();

  // ============================ MLP half: mlp_block_kernel<16> on the tile's 16 token rows ============================
  auto col4_of = [&](int g) { return SW_SC * g + 16 * wave + 4 * fq; };
  auto store_bf4 = [&](__bf16* base, int ld, int c4, f32x4 v) __attribute__((always_inline)) {
    bf16x4 h;
    h[0] = (__bf16)v[0]; h[1] = (__bf16)v[1]; h[2] = (__bf16)v[2]; h[3] = (__bf16)v[3];
    *reinterpret_cast<bf16x4*>(base + fr * ld + c4) = h;
  };
  // c += (A[16 rows][k0 .. k0 + nch*32) . W[16 columns of this wave][..]^T)^T
  auto mma_stage = [&](const __bf16* A, int lda, int k0, int nch, const u32x4 (&reg)[RC], f32x4 (&c)[1]) __attribute__((always_inline)) {
    sw_mma_chunks<8, 1>(A + fr * lda + k0 + 8 * fq, lda, nch, 8, reg, c);
  };
  auto epi_proj = [&](auto GI, const f32x4& c) __attribute__((always_inline)) {
    constexpr int g = decltype(GI)::value;
    x1[g] += c + *reinterpret_cast<const f32x4*>(v_bp + min(col4_of(g), SW_VD - 4));
    if constexpr (g != GD - 1) return;
    // LayerNorm2 over the d real columns of x1 -> bf16 -> A1 (all proj reads of A1 are behind a barrier)
    float sm = 0.f, sq = 0.f;
#pragma unroll
    for (int gg = 0; gg < GD; ++gg) {
      const f32x4 v = col4_of(gg) < d ? x1[gg] : f32x4{0.f, 0.f, 0.f, 0.f};
      sm += (v[0] + v[1]) + (v[2] + v[3]);
      sq += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
    }
    sm += __shfl_xor(sm, 16); sq += __shfl_xor(sq, 16);
    sm += __shfl_xor(sm, 32); sq += __shfl_xor(sq, 32);
    if (fq == 0) { red[(fr * 8 + wave) * 2 + 0] = sm; red[(fr * 8 + wave) * 2 + 1] = sq; }
    __syncthreads();
    float su = 0.f, s2 = 0.f;
#pragma unroll
    for (int w = 0; w < 8; ++w) { su += red[fr * 16 + 2 * w]; s2 += red[fr * 16 + 2 * w + 1]; }
    const float mu = su / (float)d;
    const float rstd = rsqrtf(fmaxf(s2 / (float)d - mu * mu, 0.f) + 1e-5f);
#pragma unroll
    for (int gg = 0; gg < GD; ++gg) {
      const int c4 = col4_of(gg);
      const f32x4 gam = *reinterpret_cast<const f32x4*>(v_g2 + min(c4, SW_VD - 4));
      const f32x4 bet = *reinterpret_cast<const f32x4*>(v_b2n + min(c4, SW_VD - 4));
      store_bf4(A1, SW_LDA, c4, c4 < d ? (x1[gg] - mu) * rstd * gam + bet : f32x4{0.f, 0.f, 0.f, 0.f});
      // FOLD: x1 itself is adjF's first k range (k | v are dead: every wave is past the attention); x1[] dies here
      if constexpr (FOLD) {
        if (c4 < 32 * KC) store_bf4(Ft, LDF, c4, c4 < d ? x1[gg] : f32x4{0.f, 0.f, 0.f, 0.f});
      }
    }
  };
  auto epi_fc1 = [&](int g, const f32x4& c) __attribute__((always_inline)) {
    const int c4 = col4_of(g);
    f32x4 v = c + *reinterpret_cast<const f32x4*>(v_bf1 + min(c4, SW_VM - 4));
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = gelu_fast(v[e]);
    if constexpr (FOLD) {
      if (c4 < 32 * KCM) store_bf4(Ft + 32 * KC, LDF, c4, c4 < m ? v : f32x4{0.f, 0.f, 0.f, 0.f});
    } else
    store_bf4(Hs, SW_LDH, c4, c4 < m ? v : f32x4{0.f, 0.f, 0.f, 0.f});      // m % 4 == 0
  };
  auto epi_fc2 = [&](auto GI, const f32x4& c) __attribute__((always_inline)) {
    constexpr int g = decltype(GI)::value;
    x1[g] += c + *reinterpret_cast<const f32x4*>(v_bf2 + min(col4_of(g), SW_VD - 4));
    if constexpr (g != GD - 1) return;
    // x2 -> bf16 -> A1 (its last readers, the fc1 stages, finished long ago)
#pragma unroll
    for (int gg = 0; gg < GD; ++gg) {
      const int c4 = col4_of(gg);
      store_bf4(A1, SW_LDA, c4, c4 < d ? x1[gg] : f32x4{0.f, 0.f, 0.f, 0.f});
    }
  };
  auto epi_adj = [&](int g, const f32x4& c) __attribute__((always_inline)) {
    const int c4 = col4_of(g);
    const int cc = min(c4, no - 4);                                 // no % 4 == 0
    const f32x4 ba = *reinterpret_cast<const f32x4*>(v_ba + min(c4, SW_VD - 4));
    f32x4 rv = {0.f, 0.f, 0.f, 0.f};
    if (p.R) rv = *reinterpret_cast<const f32x4*>(p.R + (size_t)row_tok * p.ldr + cc);
    f32x4 v = c + ba;
    if (p.act == SRAD_ACT_LRELU) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : v[e] * p.slope;
    }
    v = v * p.alpha + rv;
    if (c4 < no) *reinterpret_cast<f32x4*>(p.Y + (size_t)row_tok * p.ldy + p.yoff + c4) = v;
  };

  f32x4 c[1];
  static_for<0, n_mlp>([&](auto SI) {
    constexpr int s = decltype(SI)::value;
    constexpr MlpStage sg = Chain::stage(s);
    constexpr int ph = sg.ph, g = sg.g, kg = sg.kg, nch = sg.nch;
    u32x4 (&reg)[RC] = w_reg[(QS + s) % NSETS];
    if constexpr (sg.first) __syncthreads();            // first stage of a phase: the activation tile (A1 / Hs) is complete
    if constexpr (kg == 0) c[0] = f32x4{0.f, 0.f, 0.f, 0.f};
    const bool live = (g * 8 + wave_s) * 16 < (ph == 0 ? d : (ph == 1 ? m : (ph == 2 ? d : no)));
    if constexpr (SPLITK && ph == 3) {
      // ---- adjF, k split: this wave's part of [bf16(x1) | h] against its part of [A | A W2]; the four partial tiles of a
      //      column tile meet in LDS (the LayerNorm2 tile is dead: every wave is past fc1) and waves 0 / 1 add them in part
      //      order - a fixed order, whatever the waves' timing ----
      const int ct = wave_s & 1, pt = wave_s >> 1, p0 = pt * nch;
      const __bf16* ar = Ft + fr * LDF + 8 * fq;
      bf16x8 af[nch];
#pragma unroll
      for (int gq = 0; gq < nch; ++gq) af[gq] = *reinterpret_cast<const bf16x8*>(ar + min(p0 + gq, KF - 1) * 32);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int gq = 0; gq < nch; ++gq) {
        const u32x4 wz = p0 + gq < KF ? reg[gq] : u32x4{0u, 0u, 0u, 0u};
        c[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wz), af[gq], c[0], 0, 0, 0);
      }
      float* const part = reinterpret_cast<float*>(A1);            // [4 parts][2 column tiles][16 rows][16]
      *reinterpret_cast<f32x4*>(part + ((pt * 2 + ct) * 16 + fr) * 16 + 4 * fq) = c[0];
      __syncthreads();
      if (wave_s < 2) {
        const float* src = part + (wave_s * 16 + fr) * 16 + 4 * fq;
        f32x4 sum = *reinterpret_cast<const f32x4*>(src);
#pragma unroll
        for (int q = 1; q < 4; ++q) sum += *reinterpret_cast<const f32x4*>(src + q * 512);
        epi_adj(0, sum);
      }
    } else if constexpr (FOLD && ph == 3) {
      if (live) mma_stage(Ft, LDF, kg * 256, nch, reg, c);
    } else
    if (live) mma_stage(ph == 2 ? Hs : A1, ph == 2 ? SW_LDH : SW_LDA, kg * 256, nch, reg, c);
    // refill this set, NSETS stages ahead; behind an epilogue that other waves wait for (see mlp_block_kernel)
    constexpr bool epi_first = sg.last && !(SPLITK && ph == 3);     // (the split stage is the last and has stored already)
    if constexpr (SPLITK && ph == 3) return;
    if constexpr (!epi_first) load_w(std::integral_constant<int, QS + s + NSETS>{}, reg);
    if constexpr (epi_first) {
      if constexpr (ph == 0) epi_proj(std::integral_constant<int, g>{}, c[0]);
      else if constexpr (ph == 1) epi_fc1(g, c[0]);
      else if constexpr (ph == 2) epi_fc2(std::integral_constant<int, g>{}, c[0]);
      else epi_adj(g, c[0]);
      load_w(std::integral_constant<int, QS + s + NSETS>{}, reg);
    }
  });
}

template <int HDT, int KC, int HEADS, int GD, int KGD, int GM, int KGM, int GN, int KCM, bool FOLD>
int launch_blk(const SwinBlockParams& p, hipStream_t stream) {
  constexpr size_t lds = BlkGeo<HDT, KC, HEADS>::LDS;
  const double T = (double)p.B * p.H * p.W;
  // (FOLD: fc2 d x m and adjust no x d are one no x (d + m) GEMM)
  const double mlp2 = FOLD ? (double)p.no * (p.d + p.m) : (double)p.d * p.m + (double)p.no * p.d;
  const double flops = 2.0 * T * (4.0 * p.d * p.d + (double)p.d * p.m + mlp2) + 4.0 * T * 64.0 * p.d;
  const double bytes = 4.0 * T * (2.0 * p.d + p.no) + 2.0 * (4.0 * p.d * p.d + (double)p.d * p.m + mlp2);
  SradProfScope prof(stream, SRAD_K_SWIN_BLOCK, flops, bytes);
  const int nW = (p.H / 8) * (p.W / 8);
  SRAD_TRY((srad_launch_dyn<swin_block_kernel<HDT, KC, HEADS, GD, KGD, GM, KGM, GN, KCM, FOLD>>(dim3(p.B * nW, 4), dim3(512), lds, stream, p)));
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

// the whole geometry key: head tiles, heads and the MLP chain's stages (instances: swin_tiles.h's table of block shapes)
constexpr bool blk_key_eq(const SwinKey& a, const SwinKey& b) { return a.hdt == b.hdt && a.heads == b.heads && swin_key_mlp_eq(a, b); }
}  // namespace

extern "C" int srad_swin_block_supported(int prec, int ws, int B, int H, int W, int d, int heads, int hidden, int no) {
  if (prec != SRAD_PREC_BF16 || ws != 8 || B < 1 || H < 8 || W < 8 || H % 8 || W % 8 || d % 4 || hidden % 4 || no % 4 || d < 32 || d > 320 ||
      hidden < 32 || hidden > 512 || no < 4 || no > 384 || heads < 1 || d % heads)
    return false;
  if ((long long)B * (H / 8) * (W / 8) * 4 > srad_cu_count()) return false;   // one workgroup per CU, all resident: a quarter window each
  const SwinKey c = swin_key(d, heads, hidden, no);
#define X(d_, h_, m_, no_, wpc_) if (blk_key_eq(c, swin_key(d_, h_, m_, no_))) return true;
  SRAD_SWIN_SHAPES(X)
#undef X
  return false;
}

// Block shapes (d, heads, hidden, adjust outputs) for which tools/swin_block_bench.py measured the single launch faster than
// qkv_attn + mlp_block + one launch boundary at B = 4, 32 x 32 AND the step measured faster with them (with
// compact head rows and one head group d = 276 wins 3.1 us on the bench and 0.03 ms in the step; d = 308 wins 0.4 - 1.0 us on
// the bench and nothing measurable in the step, so it keeps the pair).  The engine takes the new kernel for these only.
bool srad_swin_block_wins(int d, int heads, int hidden, int no) {
  struct Shape { int d, heads, hidden, no; };
  static const Shape wins[] = {{180, 6, 360, 32}, {212, 4, 424, 32}, {244, 2, 488, 32}, {276, 6, 276, 32}};
  for (const Shape& s : wins)
    if (s.d == d && s.heads == heads && s.hidden == hidden && s.no == no) return true;
  return false;
}

// the folded second half (mlp_fold.h): the block shapes with an instance, and of those the ones whose adjF stage form fits -
// one 128-column group takes the k-split stage, which has two column tiles
extern "C" int srad_swin_block_fold_supported(int prec, int ws, int B, int H, int W, int d, int heads, int hidden, int no) {
  return srad_swin_block_supported(prec, ws, B, H, W, d, heads, hidden, no) && (no > SW_SC || no <= 32);
}

static int launch_swin_block(const SwinBlockParams& p, bool fold, hipStream_t stream) {
  SRAD_REQUIRE(!fold || srad_swin_block_fold_supported(SRAD_PREC_BF16, 8, p.B, p.H, p.W, p.d, p.heads, p.m, p.no),
               "swin_block: no folded form for d=%d heads=%d m=%d no=%d", p.d, p.heads, p.m, p.no);
  SRAD_REQUIRE(srad_swin_block_supported(SRAD_PREC_BF16, 8, p.B, p.H, p.W, p.d, p.heads, p.m, p.no),
               "swin_block: unsupported shape %dx%dx%d d=%d heads=%d m=%d no=%d (bf16, window 8, windows x 4 <= CUs)", p.B, p.H, p.W, p.d, p.heads, p.m, p.no);
  SRAD_REQUIRE(p.x && p.ln1_g && p.ln1_b && p.w_qkv && p.b_qkv && p.table && p.w_proj && p.w_fc1 && p.w_fc2 && p.w_adj && p.b_proj && p.b_fc1 &&
                   p.b_fc2 && p.b_adj && p.ln2_g && p.ln2_b && p.Y, "swin_block: null argument");
  SRAD_REQUIRE(p.shift >= 0 && p.shift < 8, "swin_block: shift %d must be in [0, 8)", p.shift);
  SRAD_REQUIRE((p.ldx & 3) == 0 && ((uintptr_t)p.x & 15) == 0 && (p.ldy & 3) == 0 && (p.yoff & 3) == 0 && ((uintptr_t)p.Y & 15) == 0 &&
                   (!p.R || ((p.ldr & 3) == 0 && ((uintptr_t)p.R & 15) == 0)),
               "swin_block: input / output / residual rows must be float4-addressable");
  SRAD_REQUIRE((((uintptr_t)p.b_proj | (uintptr_t)p.b_fc1 | (uintptr_t)p.b_fc2 | (uintptr_t)p.b_adj | (uintptr_t)p.ln2_g | (uintptr_t)p.ln2_b) & 15) == 0,
               "swin_block: bias / LayerNorm2 vectors must be 16-byte aligned");
  // the output may share x's buffer only as the columns behind the block's own (adjust_k); anything else would race with the
  // other workgroups' reads of columns [0, d)
  SRAD_REQUIRE(p.Y != p.x || (p.ldy == p.ldx && p.yoff >= p.d), "swin_block: an in-place output must lie behind the block's %d input columns", p.d);
  const SwinKey c = swin_key(p.d, p.heads, p.m, p.no);
#define X(d_, h_, m_, no_, wpc_) \
  if (constexpr SwinKey k = swin_key(d_, h_, m_, no_); blk_key_eq(c, k)) { \
    if (fold) return launch_blk<k.hdt, k.kc, k.heads, k.gd, k.kgd, k.gm, k.kgm, k.gn, k.kcm, true>(p, stream); \
    return launch_blk<k.hdt, k.kc, k.heads, k.gd, k.kgd, k.gm, k.kgm, k.gn, k.kcm, false>(p, stream); \
  }
  SRAD_SWIN_SHAPES(X)
#undef X
  return srad_set_error(SRAD_ERR_ARG, "swin_block: no kernel instance for this geometry");
}

int srad_launch_swin_block(const SwinBlockParams& p, hipStream_t stream) { return launch_swin_block(p, false, stream); }
// p.w_adj = the fragment pack of [A | A W2], p.b_adj = A b2 + b_a (mlp_fold.h); p.w_fc2 is not read (any non-null pointer)
int srad_launch_swin_block_folded(const SwinBlockParams& p, hipStream_t stream) { return launch_swin_block(p, true, stream); }
