// ops.hip - operator-level C ABI: the single kernels behind the engines, exposed so that each
// row of SURVEY.md §8(a) (A4-A7, A9, B3-B6) can be parity-tested on its own against the oracle.
#include "engine.h"
#include "mlp_fold.h"
#include "../../include/srad.h"

extern "C" {

// Linear / 1x1 conv / 3x3 conv with the fused prologue+epilogue of kernels_gemm.hip.
//   x      : [M_in rows][ldx] fp32 NHWC activations
//   w      : PyTorch-layout fp32 weight [N][Cin][taps] (device), packed into `scratch` first
//   conv   : ntaps = 9 -> 3x3 pad 1 with the given stride over an (B, Hi, Wi) image; ntaps = 1 and
//            stride 1 -> rows are used as they are
//   ln_g/b : optional LayerNorm over the Cin channels of each row (eps 1e-5), ntaps = 1 only
//   epilogue: + bias -> act (0 none, 1 GELU-erf, 2 LeakyReLU(slope), 3 ReLU) -> * alpha -> + r
//   ps     : 0 plain rows [M][ldy] at column yoff; 2 = PixelShuffle(2) scatter
static int op_gemm_params(int precision, const float* x, int ldx, int B, int Hi, int Wi, int Cin, const float* w, int N, int ntaps,
                          int stride, const float* bias, const float* ln_g, const float* ln_b, int act, float slope, float alpha,
                          const float* r, int ldr, float* y, int ldy, int yoff, int ps, void* scratch, size_t scratch_bytes,
                          GemmParams* out) {
  SRAD_REQUIRE(x && w && y && scratch, "op_gemm: null argument");
  SRAD_REQUIRE(ntaps == 1 || ntaps == 9, "op_gemm: ntaps must be 1 or 9");
  SRAD_REQUIRE(stride == 1 || stride == 2, "op_gemm: stride must be 1 or 2");
  const size_t need = srad_packed_bytes(precision, N, Cin, ntaps);
  SRAD_REQUIRE(scratch_bytes >= need, "op_gemm: scratch %zu bytes, %zu needed", scratch_bytes, need);
  GemmParams p{};
  const int pad = ntaps == 9 ? 1 : 0, k = ntaps == 9 ? 3 : 1;
  p.Hi = Hi; p.Wi = Wi;
  p.Ho = (Hi + 2 * pad - k) / stride + 1;
  p.Wo = (Wi + 2 * pad - k) / stride + 1;
  p.stride = stride;
  p.X = x; p.ldx = ldx; p.M = B * p.Ho * p.Wo; p.Cin = Cin; p.Cp = srad_cp(Cin); p.ntaps = ntaps;
  p.ln_g = ln_g; p.ln_b = ln_b; p.ln_eps = 1e-5f;
  p.Wp = scratch; p.N = N; p.bias = bias;
  p.act = act; p.slope = slope; p.alpha = alpha;
  p.R = r; p.ldr = ldr; p.Y = y; p.ldy = ldy; p.yoff = yoff; p.ps = ps;
  p.hsplit_hd = 0; p.hsplit_hdp = 0;
  *out = p;
  return SRAD_OK;
}

int srad_op_gemm(int precision, const float* x, int ldx, int B, int Hi, int Wi, int Cin, const float* w, int N,
                 int ntaps, int stride, const float* bias, const float* ln_g, const float* ln_b, int act, float slope,
                 float alpha, const float* r, int ldr, float* y, int ldy, int yoff, int ps, void* scratch,
                 size_t scratch_bytes, void* stream) {
  GemmParams p;
  SRAD_TRY(op_gemm_params(precision, x, ldx, B, Hi, Wi, Cin, w, N, ntaps, stride, bias, ln_g, ln_b, act, slope, alpha, r, ldr, y, ldy,
                          yoff, ps, scratch, scratch_bytes, &p));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  SRAD_TRY(srad_launch_pack_weight(precision, w, scratch, N, Cin, ntaps, s));
  return srad_launch_gemm(precision, p, s);
}

// The plan of that call (include/srad.h): same arguments, same checks, no launch.
int srad_op_gemm_plan(int precision, const float* x, int ldx, int B, int Hi, int Wi, int Cin, const float* w, int N,
                      int ntaps, int stride, const float* bias, const float* ln_g, const float* ln_b, int act, float slope,
                      float alpha, const float* r, int ldr, float* y, int ldy, int yoff, int ps, void* scratch,
                      size_t scratch_bytes, void* stream, srad_gemm_plan* plan) {
  (void)stream;
  GemmParams p;
  SRAD_TRY(op_gemm_params(precision, x, ldx, B, Hi, Wi, Cin, w, N, ntaps, stride, bias, ln_g, ln_b, act, slope, alpha, r, ldr, y, ldy,
                          yoff, ps, scratch, scratch_bytes, &p));
  return srad_plan_gemm(precision, p, plan);
}

// The 80 -> 80 channel 3x3 convolution with bf16 operands as DRN's bf16 chains issue it (conv80_kernel<XH, RM>): x_h [B*H*W][80]
// bf16; output bf16 (y_h) or fp32 (y); residual operand bf16 (r_h) or fp32 (r) or none, rmode as GemmParams (0 add, 2 the
// LeakyReLU / ReLU mask of a backward); optional per-tile column sums.  Fails if the shape does not take that kernel.
// Bit 16 of `rmode`: the phase-stamp build of the kernel (bf16 input, no residual; synchronous, medians to stderr).
int srad_op_conv80_h(const void* x_h, const float* w, const float* bias, int act, float slope, const void* r_h, const float* r,
                     int rmode, int B, int H, int W, void* y_h, float* y, float* pool_part, void* scratch, size_t scratch_bytes,
                     void* stream) {
  SRAD_REQUIRE(x_h && w && (y_h || y) && scratch, "op_conv80_h: null argument");
  const size_t need = srad_packed_bytes(SRAD_PREC_BF16, 80, 80, 9);
  SRAD_REQUIRE(scratch_bytes >= need, "op_conv80_h: scratch %zu bytes, %zu needed", scratch_bytes, need);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  SRAD_TRY(srad_launch_pack_weight(SRAD_PREC_BF16, w, scratch, 80, 80, 9, s));
  GemmParams p{};
  p.Hi = p.Ho = H; p.Wi = p.Wo = W; p.stride = 1;
  p.Xh = reinterpret_cast<const __bf16*>(x_h); p.ldx = 80; p.M = B * H * W; p.Cin = 80; p.Cp = srad_cp(80); p.ntaps = 9; p.ln_eps = 1e-5f;
  p.Wp = scratch; p.N = 80; p.bias = bias; p.act = act; p.slope = slope; p.alpha = 1.f;
  p.R = r; p.Rh = reinterpret_cast<const __bf16*>(r_h); p.ldr = 80; p.rmode = rmode & 0xffff;
  p.Y = y; p.Yh = reinterpret_cast<__bf16*>(y_h); p.ldy = 80; p.pool_part = pool_part;
  SRAD_REQUIRE(srad_conv80_supported(SRAD_PREC_BF16, p), "op_conv80_h: this shape does not take the 80-channel conv kernel");
  if (rmode & 0x10000) return srad_launch_conv80(p, s, true);
  return srad_launch_gemm(SRAD_PREC_BF16, p, s);
}

// Diagnostic: launch the same GEMM `iters` times back to back on `stream` (weights packed once) and
// return the average device time per launch in microseconds (HIP events; synchronises the stream).
int srad_bench_gemm(int precision, const float* x, int ldx, int B, int Hi, int Wi, int Cin, const float* w, int N,
                    int ntaps, int stride, const float* bias, const float* ln_g, const float* ln_b, int act,
                    const float* r, int ldr, float* y, int ldy, int hsplit_hd, int hsplit_hdp, void* scratch,
                    size_t scratch_bytes, int iters, float* us_out, void* stream) {
  SRAD_REQUIRE(x && w && y && scratch && us_out && iters > 0, "bench_gemm: bad argument");
  const size_t need = srad_packed_bytes(precision, N, Cin, ntaps);
  SRAD_REQUIRE(scratch_bytes >= need, "bench_gemm: scratch %zu bytes, %zu needed", scratch_bytes, need);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  SRAD_TRY(srad_launch_pack_weight(precision, w, scratch, N, Cin, ntaps, s));
  GemmParams p{};
  const int pad = ntaps == 9 ? 1 : 0, k = ntaps == 9 ? 3 : 1;
  p.Hi = Hi; p.Wi = Wi;
  p.Ho = (Hi + 2 * pad - k) / stride + 1;
  p.Wo = (Wi + 2 * pad - k) / stride + 1;
  p.stride = stride;
  p.X = x; p.ldx = ldx; p.M = B * p.Ho * p.Wo; p.Cin = Cin; p.Cp = srad_cp(Cin); p.ntaps = ntaps;
  p.ln_g = ln_g; p.ln_b = ln_b; p.ln_eps = 1e-5f;
  p.Wp = scratch; p.N = N; p.bias = bias;
  p.act = act; p.slope = 0.2f; p.alpha = 1.f;
  p.R = r; p.ldr = ldr; p.Y = y; p.ldy = ldy; p.yoff = 0; p.ps = 0;
  p.hsplit_hd = hsplit_hd; p.hsplit_hdp = hsplit_hdp;
  for (int i = 0; i < 5; ++i) SRAD_TRY(srad_launch_gemm(precision, p, s));
  hipEvent_t a, b;
  SRAD_CHECK_HIP(hipEventCreate(&a));
  SRAD_CHECK_HIP(hipEventCreate(&b));
  SRAD_CHECK_HIP(hipEventRecord(a, s));
  for (int i = 0; i < iters; ++i) SRAD_TRY(srad_launch_gemm(precision, p, s));
  SRAD_CHECK_HIP(hipEventRecord(b, s));
  SRAD_CHECK_HIP(hipEventSynchronize(b));
  float ms = 0.f;
  SRAD_CHECK_HIP(hipEventElapsedTime(&ms, a, b));
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  *us_out = ms * 1e3f / iters;
  return SRAD_OK;
}

int srad_bench_window_attn(int precision, const float* qkv, float* out, const float* table, int B, int H, int W, int ws,
                           int shift, int d, int heads, int hdp, int iters, float* us_out, void* stream) {
  SRAD_REQUIRE(qkv && out && table && us_out && iters > 0, "bench_window_attn: bad argument");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  AttnParams a{qkv, out, table, B, H, W, ws, shift, d, heads, hdp};
  for (int i = 0; i < 5; ++i) SRAD_TRY(srad_launch_window_attn(precision, a, s));
  hipEvent_t e0, e1;
  SRAD_CHECK_HIP(hipEventCreate(&e0));
  SRAD_CHECK_HIP(hipEventCreate(&e1));
  SRAD_CHECK_HIP(hipEventRecord(e0, s));
  for (int i = 0; i < iters; ++i) SRAD_TRY(srad_launch_window_attn(precision, a, s));
  SRAD_CHECK_HIP(hipEventRecord(e1, s));
  SRAD_CHECK_HIP(hipEventSynchronize(e1));
  float ms = 0.f;
  SRAD_CHECK_HIP(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  *us_out = ms * 1e3f / iters;
  return SRAD_OK;
}

// Diagnostic: the fused MLP block on synthetic operands, `iters` back-to-back launches, microseconds per launch.
// scratch must hold the four packed bf16 weights; x/y are [M][320] fp32 buffers.
int srad_bench_mlp_block(int M, int d, int m, int no, const void* attn /* bf16 [M][320] */, const float* shortcut, float* y,
                         const float* w_fp32 /* >= 512*512 floats */, void* scratch, size_t scratch_bytes, int dbg,
                         int iters, float* us_out, void* stream) {
  SRAD_REQUIRE(attn && shortcut && y && w_fp32 && scratch && us_out && iters > 0, "bench_mlp_block: bad argument");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const size_t b1 = srad_align_up(srad_packed_bytes(SRAD_PREC_BF16, d, d, 1), 256), b2 = srad_align_up(srad_packed_bytes(SRAD_PREC_BF16, m, d, 1), 256),
               b3 = srad_align_up(srad_packed_bytes(SRAD_PREC_BF16, d, m, 1), 256), b4 = srad_align_up(srad_packed_bytes(SRAD_PREC_BF16, no, d, 1), 256);
  SRAD_REQUIRE(scratch_bytes >= b1 + b2 + b3 + b4, "bench_mlp_block: scratch too small");
  char* sc = reinterpret_cast<char*>(scratch);
  SRAD_TRY(srad_launch_pack_weight_frag(w_fp32, sc, d, d, s));
  SRAD_TRY(srad_launch_pack_weight_frag(w_fp32, sc + b1, m, d, s));
  SRAD_TRY(srad_launch_pack_weight_frag(w_fp32, sc + b1 + b2, d, m, s));
  SRAD_TRY(srad_launch_pack_weight_frag(w_fp32, sc + b1 + b2 + b3, no, d, s));
  MlpBlockParams q{};
  q.attn_h = reinterpret_cast<const __bf16*>(attn); q.ld_attn = 320; q.shortcut = shortcut; q.ld_short = 320; q.M = M; q.d = d; q.m = m; q.no = no;
  q.w_proj = sc; q.w_fc1 = sc + b1; q.w_fc2 = sc + b1 + b2; q.w_adj = sc + b1 + b2 + b3;
  q.b_proj = q.b_fc1 = q.b_fc2 = q.b_adj = q.ln_g = q.ln_b = w_fp32;
  q.act = SRAD_ACT_LRELU; q.slope = 0.2f; q.alpha = 1.f; q.R = nullptr; q.ldr = 0; q.Y = y; q.ldy = 320; q.yoff = 0; q.dbg = dbg & 0xff;
  q.fm = (dbg >> 8) & 0xff;                         // bits 8..15: rows per workgroup (0 = auto)
  if (dbg & 0x20000) {                              // bit 17: the split-bf16 kernel; `attn` is then an fp32 [M][320] array and the
    char* lo = sc + b1 + b2 + b3 + b4;              // lo packs follow the hi packs in scratch
    SRAD_REQUIRE(scratch_bytes >= 2 * (b1 + b2 + b3 + b4), "bench_mlp_block: scratch too small for the lo packs");
    SRAD_TRY(srad_launch_pack_weight_frag_lo(w_fp32, lo, d, d, s));
    SRAD_TRY(srad_launch_pack_weight_frag_lo(w_fp32, lo + b1, m, d, s));
    SRAD_TRY(srad_launch_pack_weight_frag_lo(w_fp32, lo + b1 + b2, d, m, s));
    SRAD_TRY(srad_launch_pack_weight_frag_lo(w_fp32, lo + b1 + b2 + b3, no, d, s));
    q.split = 1; q.attn_f = reinterpret_cast<const float*>(attn);
    q.w_proj_lo = lo; q.w_fc1_lo = lo + b1; q.w_fc2_lo = lo + b1 + b2; q.w_adj_lo = lo + b1 + b2 + b3;
    q.dbg = 0;
  } else
  if (dbg & 0x40000) {                              // bit 18: the folded second half, [A | A W2] cut from w_fp32 like every weight:
    const MlpFoldLayout l = mf_layout(d, m, no);    // the pack of a [no][32 (KC + KCM)] matrix over the fc2 and adjust packs' space
    SRAD_REQUIRE(srad_mlp_block_fold_has(M, q.fm, d, m, no), "bench_mlp_block: no folded form for this shape");
    SRAD_REQUIRE(b3 + b4 >= (size_t)srad_np(no) * l.kf * 2, "bench_mlp_block: the folded pack does not fit the scratch layout");
    SRAD_TRY(srad_launch_pack_weight_frag(w_fp32, sc + b1 + b2, no, l.kf, s));
    q.w_adj = sc + b1 + b2; q.dbg = 0;
  } else
  if (dbg & 0x100ff) {                              // bit 16 or any switch-off bit: the diagnostic build; its stamps go behind the packed weights
    SRAD_REQUIRE(scratch_bytes >= b1 + b2 + b3 + b4 + (size_t)(M / 16) * 8 * 16 * 8, "bench_mlp_block: scratch too small for the stamps");
    q.stamps = reinterpret_cast<unsigned long long*>(sc + b1 + b2 + b3 + b4);
  }
  const auto launch = (dbg & 0x40000) ? srad_launch_mlp_block_folded : srad_launch_mlp_block;
  for (int i = 0; i < 3; ++i) SRAD_TRY(launch(q, s));
  hipEvent_t a, b;
  SRAD_CHECK_HIP(hipEventCreate(&a));
  SRAD_CHECK_HIP(hipEventCreate(&b));
  SRAD_CHECK_HIP(hipEventRecord(a, s));
  for (int i = 0; i < iters; ++i) SRAD_TRY(launch(q, s));
  SRAD_CHECK_HIP(hipEventRecord(b, s));
  SRAD_CHECK_HIP(hipEventSynchronize(b));
  float ms = 0.f;
  SRAD_CHECK_HIP(hipEventElapsedTime(&ms, a, b));
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  *us_out = ms * 1e3f / iters;
  return SRAD_OK;
}

// ---- the two fused forward kernels of a Swin block (bf16 / split-bf16, window 8), weights in PyTorch layout, packed into
//      scratch: five hi packs, then (split-bf16) the five lo packs ----
static size_t swin_scratch_parts(int d, int heads, int m, int no, size_t* off) {
  size_t o = 0;
  for (int lo = 0; lo < 2; ++lo) {
    off[5 * lo + 0] = o; o += srad_align_up(srad_qkv_frag_bytes(d, heads), 256);
    off[5 * lo + 1] = o; o += srad_align_up(srad_packed_bytes(SRAD_PREC_BF16, d, d, 1), 256);
    off[5 * lo + 2] = o; o += srad_align_up(srad_packed_bytes(SRAD_PREC_BF16, m, d, 1), 256);
    off[5 * lo + 3] = o; o += srad_align_up(srad_packed_bytes(SRAD_PREC_BF16, d, m, 1), 256);
    off[5 * lo + 4] = o; o += srad_align_up(srad_packed_bytes(SRAD_PREC_BF16, no, d, 1), 256);
  }
  return o;
}

size_t srad_op_swin_scratch_bytes(int d, int heads, int m, int no) {
  size_t off[10];
  return swin_scratch_parts(d, heads > 0 ? heads : 1, m > 0 ? m : 4, no > 0 ? no : 4, off);
}

// First half of a Swin block: LayerNorm1 -> qkv Linear -> shifted-window attention (src/drct.py:477-504, 271-299).
//   x [B*H*W][ldx] (columns [0, d)), w_qkv [3d][d], b_qkv [3d], table [225][heads] -> out [B*H*W][d]
int srad_op_qkv_attn(int precision, const float* x, int ldx, int B, int H, int W, int shift, int d, int heads, const float* ln_g,
                     const float* ln_b, const float* w_qkv, const float* b_qkv, const float* table, void* out, int out_bf16,
                     void* scratch, size_t scratch_bytes, void* stream) {
  SRAD_REQUIRE(x && ln_g && ln_b && w_qkv && b_qkv && table && out && scratch, "op_qkv_attn: null argument");
  SRAD_REQUIRE(precision == SRAD_PREC_BF16 || precision == SRAD_PREC_BF16X3, "op_qkv_attn: precision must be bf16 or split-bf16 (fp32 runs the unfused kernels)");
  SRAD_REQUIRE(srad_qkv_attn_supported(precision, 8, H, W, d, heads), "op_qkv_attn: unsupported shape d=%d heads=%d %dx%d", d, heads, H, W);
  const size_t wb = srad_align_up(srad_qkv_frag_bytes(d, heads), 256);
  const bool x3 = precision == SRAD_PREC_BF16X3;
  SRAD_REQUIRE(scratch_bytes >= wb * (x3 ? 2 : 1) && ((uintptr_t)scratch & 255) == 0, "op_qkv_attn: scratch too small or not 256-byte aligned");
  SRAD_REQUIRE(!(x3 && out_bf16), "op_qkv_attn: the split-bf16 kernel writes fp32");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  SRAD_TRY(srad_launch_pack_qkv_frag(w_qkv, scratch, d, heads, s));
  QkvAttnParams a{};
  if (x3) {
    SRAD_TRY(srad_launch_pack_qkv_frag_lo(w_qkv, reinterpret_cast<char*>(scratch) + wb, d, heads, s));
    a.split = 1; a.w_qkv_lo = reinterpret_cast<char*>(scratch) + wb;
  }
  a.x = x; a.ldx = ldx; a.ln_g = ln_g; a.ln_b = ln_b; a.w_qkv = scratch; a.b_qkv = b_qkv; a.table = table;
  if (out_bf16) a.out_h = reinterpret_cast<__bf16*>(out); else a.out = reinterpret_cast<float*>(out);
  a.ld_out = d; a.B = B; a.H = H; a.W = W; a.shift = shift; a.d = d; a.heads = heads;
  return srad_launch_qkv_attn(a, s);
}

int srad_op_qkv_attn_train(const float* x, int ldx, int B, int H, int W, int shift, int d, int heads, const float* ln_g,
                           const float* ln_b, const float* w_qkv, const float* b_qkv, const float* table, void* out_h,
                           float* save_xn, void* save_xn_h, float* save_qkv, int hdp, void* save_qkv_h, int hp_h, int no_qsplit,
                           void* scratch, size_t scratch_bytes, void* stream) {
  SRAD_REQUIRE(x && ln_g && ln_b && w_qkv && b_qkv && table && out_h && scratch, "op_qkv_attn_train: null argument");
  SRAD_REQUIRE(srad_qkv_attn_supported(SRAD_PREC_BF16, 8, H, W, d, heads), "op_qkv_attn_train: unsupported shape d=%d heads=%d %dx%d", d, heads, H, W);
  SRAD_REQUIRE(!save_qkv || (hdp >= d / heads && hdp % 4 == 0), "op_qkv_attn_train: hdp %d must be a multiple of 4 >= the head dim", hdp);
  SRAD_REQUIRE(!save_qkv_h || (hp_h >= d / heads && hp_h % 8 == 0), "op_qkv_attn_train: hp_h %d must be a multiple of 8 >= the head dim", hp_h);
  SRAD_REQUIRE(scratch_bytes >= srad_align_up(srad_qkv_frag_bytes(d, heads), 256) && ((uintptr_t)scratch & 255) == 0,
               "op_qkv_attn_train: scratch too small or not 256-byte aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  SRAD_TRY(srad_launch_pack_qkv_frag(w_qkv, scratch, d, heads, s));
  QkvAttnParams a{};
  a.x = x; a.ldx = ldx; a.ln_g = ln_g; a.ln_b = ln_b; a.w_qkv = scratch; a.b_qkv = b_qkv; a.table = table;
  a.out_h = reinterpret_cast<__bf16*>(out_h); a.ld_out = d;
  a.B = B; a.H = H; a.W = W; a.shift = shift; a.d = d; a.heads = heads; a.no_qsplit = no_qsplit;
  a.save_xn = save_xn; a.save_xn_h = reinterpret_cast<__bf16*>(save_xn_h);
  a.save_qkv = save_qkv; a.hdp = hdp; a.save_qkv_h = reinterpret_cast<__bf16*>(save_qkv_h); a.hp_h = hp_h;
  return srad_launch_qkv_attn(a, s);
}

// Diagnostic twin of srad_bench_mlp_block for the first half: microseconds per launch, back-to-back launches.
int srad_bench_qkv_attn(const float* x, int ldx, int B, int H, int W, int shift, int d, int heads, const float* w_fp32,
                        void* out, void* scratch, size_t scratch_bytes, int iters, float* us_out, void* stream) {
  SRAD_REQUIRE(x && w_fp32 && out && scratch && us_out && iters > 0, "bench_qkv_attn: bad argument");
  SRAD_REQUIRE(srad_qkv_attn_supported(SRAD_PREC_BF16, 8, H, W, d, heads), "bench_qkv_attn: unsupported shape");
  SRAD_REQUIRE(scratch_bytes >= srad_align_up(srad_qkv_frag_bytes(d, heads), 256), "bench_qkv_attn: scratch too small");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  SRAD_TRY(srad_launch_pack_qkv_frag(w_fp32, scratch, d, heads, s));
  QkvAttnParams a{};
  a.x = x; a.ldx = ldx; a.ln_g = w_fp32; a.ln_b = w_fp32; a.w_qkv = scratch; a.b_qkv = w_fp32; a.table = w_fp32;
  a.out_h = reinterpret_cast<__bf16*>(out); a.ld_out = d;        // the hand-off the engines use (bf16, in the caller's buffer)
  a.B = B; a.H = H; a.W = W; a.shift = shift & 0xff; a.d = d; a.heads = heads;
  if (shift & 0x20000) {                            // bit 17 of `shift`: the split-bf16 kernel (fp32 output [T][d], lo pack behind the hi pack)
    const size_t wb = srad_align_up(srad_qkv_frag_bytes(d, heads), 256);
    SRAD_REQUIRE(scratch_bytes >= 2 * wb, "bench_qkv_attn: scratch too small for the lo pack");
    SRAD_TRY(srad_launch_pack_qkv_frag_lo(w_fp32, reinterpret_cast<char*>(scratch) + wb, d, heads, s));
    a.split = 1; a.w_qkv_lo = reinterpret_cast<char*>(scratch) + wb;
    a.out = reinterpret_cast<float*>(out); a.out_h = nullptr;
  } else
  if (shift & 0x10000) {                            // bit 16 of `shift`: the stamp build; stamps go behind the weight pack in scratch
    const size_t wb = srad_align_up(srad_qkv_frag_bytes(d, heads), 256);
    SRAD_REQUIRE(scratch_bytes >= wb + (size_t)B * (H / 8) * (W / 8) * heads * 8 * 16 * 8, "bench_qkv_attn: scratch too small for the stamps");
    a.stamps = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(scratch) + wb);
  }
  for (int i = 0; i < 3; ++i) SRAD_TRY(srad_launch_qkv_attn(a, s));
  hipEvent_t e0, e1;
  SRAD_CHECK_HIP(hipEventCreate(&e0));
  SRAD_CHECK_HIP(hipEventCreate(&e1));
  SRAD_CHECK_HIP(hipEventRecord(e0, s));
  for (int i = 0; i < iters; ++i) SRAD_TRY(srad_launch_qkv_attn(a, s));
  SRAD_CHECK_HIP(hipEventRecord(e1, s));
  SRAD_CHECK_HIP(hipEventSynchronize(e1));
  float ms = 0.f;
  SRAD_CHECK_HIP(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  *us_out = ms * 1e3f / iters;
  return SRAD_OK;
}

// Second half of a Swin block + the RDG's adjust conv (src/drct.py:300, 509-510, 184-190, 389-396):
//   x1 = shortcut + proj(attn); x2 = x1 + fc2(GELU(fc1(LN2(x1)))); Y[:, yoff:yoff+no] = act(adjust(x2)) * alpha (+ R)
//   fm: token rows per workgroup (16 / 32 / 64; 0 = the engine's choice for M)
// folded: the same second half with fc2 folded into the adjust conv (mlp_fold.h; bf16): the two packs the kernel still reads, then
// [A | A W2] and A b2 + b_a composed behind the pair's layout in scratch (from off[5], where the lo packs would start)
static int op_mlp_block(bool folded, int precision, int M, int d, int m, int no, int fm, const void* attn, const float* shortcut, int ld_short,
                        const float* w_proj, const float* b_proj, const float* ln_g, const float* ln_b, const float* w_fc1,
                        const float* b_fc1, const float* w_fc2, const float* b_fc2, const float* w_adj, const float* b_adj, int act,
                        float slope, float alpha, const float* r, int ldr, float* y, int ldy, int yoff, void* scratch, size_t scratch_bytes, void* stream) {
  const char* const who = folded ? "op_mlp_block_folded" : "op_mlp_block";
  SRAD_REQUIRE(attn && shortcut && w_proj && b_proj && ln_g && ln_b && w_fc1 && b_fc1 && w_fc2 && b_fc2 && w_adj && b_adj && y && scratch,
               "%s: null argument", who);
  const bool fm_ok = fm == 0 || ((fm == 16 || fm == 32 || fm == 64) && M % fm == 0);
  if (folded) {
    SRAD_REQUIRE(fm_ok, "op_mlp_block_folded: fm must be 0, 16, 32 or 64 and divide M");
    SRAD_REQUIRE(precision == SRAD_PREC_BF16 && srad_mlp_block_fold_has(M, fm, d, m, no),
                 "op_mlp_block_folded: unsupported: precision %d, M=%d fm=%d d=%d m=%d no=%d (bf16, no <= 32 or > 128, a tile height whose folded tile fits the LDS)",
                 precision, M, fm, d, m, no);
  } else {
    SRAD_REQUIRE(precision == SRAD_PREC_BF16 || precision == SRAD_PREC_BF16X3, "op_mlp_block: precision must be bf16 or split-bf16 (fp32 runs the unfused kernels)");
    SRAD_REQUIRE(srad_mlp_block_supported(precision, M, d, m, no), "op_mlp_block: unsupported shape M=%d d=%d m=%d no=%d", M, d, m, no);
    SRAD_REQUIRE(fm_ok, "op_mlp_block: fm must be 0, 16, 32 or 64 and divide M");
  }
  size_t off[10];
  const size_t packs = swin_scratch_parts(d, 1, m, no, off);
  const MlpFoldLayout l = folded ? mf_layout(d, m, no) : MlpFoldLayout{};
  const size_t need = folded ? off[5] + l.bytes : packs;
  SRAD_REQUIRE(scratch_bytes >= need && ((uintptr_t)scratch & 255) == 0, "%s: scratch %zu bytes, %zu needed (256-byte aligned)", who, scratch_bytes, need);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  char* sc = reinterpret_cast<char*>(scratch);
  SRAD_TRY(srad_launch_pack_weight_frag(w_proj, sc + off[1], d, d, s));
  SRAD_TRY(srad_launch_pack_weight_frag(w_fc1, sc + off[2], m, d, s));
  MlpBlockParams q{};
  q.attn_h = reinterpret_cast<const __bf16*>(attn); q.ld_attn = d; q.shortcut = shortcut; q.ld_short = ld_short; q.M = M; q.d = d; q.m = m; q.no = no;
  q.w_proj = sc + off[1]; q.w_fc1 = sc + off[2];
  q.b_proj = b_proj; q.b_fc1 = b_fc1; q.b_fc2 = b_fc2; q.ln_g = ln_g; q.ln_b = ln_b;
  q.act = act; q.slope = slope; q.alpha = alpha; q.R = r; q.ldr = ldr; q.Y = y; q.ldy = ldy; q.yoff = yoff; q.fm = fm;
  if (folded) {
    char* const fold = sc + off[5];
    SRAD_TRY(srad_mlp_fold_from_sources(l, fold, w_fc2, b_fc2, w_adj, b_adj, s));
    q.w_fc2 = fold + l.pack; q.w_adj = fold + l.pack; q.b_adj = reinterpret_cast<const float*>(fold + l.bias);
    return srad_launch_mlp_block_folded(q, s);
  }
  SRAD_TRY(srad_launch_pack_weight_frag(w_fc2, sc + off[3], d, m, s));
  SRAD_TRY(srad_launch_pack_weight_frag(w_adj, sc + off[4], no, d, s));
  q.w_fc2 = sc + off[3]; q.w_adj = sc + off[4]; q.b_adj = b_adj;
  if (precision == SRAD_PREC_BF16X3) {
    SRAD_TRY(srad_launch_pack_weight_frag_lo(w_proj, sc + off[6], d, d, s));
    SRAD_TRY(srad_launch_pack_weight_frag_lo(w_fc1, sc + off[7], m, d, s));
    SRAD_TRY(srad_launch_pack_weight_frag_lo(w_fc2, sc + off[8], d, m, s));
    SRAD_TRY(srad_launch_pack_weight_frag_lo(w_adj, sc + off[9], no, d, s));
    q.split = 1; q.attn_f = reinterpret_cast<const float*>(attn);
    q.w_proj_lo = sc + off[6]; q.w_fc1_lo = sc + off[7]; q.w_fc2_lo = sc + off[8]; q.w_adj_lo = sc + off[9];
  }
  return srad_launch_mlp_block(q, s);
}
int srad_op_mlp_block(int precision, int M, int d, int m, int no, int fm, const void* attn /* bf16 [M][d]; split-bf16: fp32 */, const float* shortcut, int ld_short,
                      const float* w_proj, const float* b_proj, const float* ln_g, const float* ln_b, const float* w_fc1,
                      const float* b_fc1, const float* w_fc2, const float* b_fc2, const float* w_adj, const float* b_adj, int act,
                      float slope, float alpha, const float* r, int ldr, float* y, int ldy, int yoff, void* scratch, size_t scratch_bytes, void* stream) {
  return op_mlp_block(false, precision, M, d, m, no, fm, attn, shortcut, ld_short, w_proj, b_proj, ln_g, ln_b, w_fc1, b_fc1, w_fc2, b_fc2, w_adj, b_adj,
                      act, slope, alpha, r, ldr, y, ldy, yoff, scratch, scratch_bytes, stream);
}
int srad_op_mlp_block_folded(int precision, int M, int d, int m, int no, int fm, const void* attn /* bf16 [M][d] */, const float* shortcut, int ld_short,
                             const float* w_proj, const float* b_proj, const float* ln_g, const float* ln_b, const float* w_fc1,
                             const float* b_fc1, const float* w_fc2, const float* b_fc2, const float* w_adj, const float* b_adj, int act,
                             float slope, float alpha, const float* r, int ldr, float* y, int ldy, int yoff, void* scratch, size_t scratch_bytes, void* stream) {
  return op_mlp_block(true, precision, M, d, m, no, fm, attn, shortcut, ld_short, w_proj, b_proj, ln_g, ln_b, w_fc1, b_fc1, w_fc2, b_fc2, w_adj, b_adj,
                      act, slope, alpha, r, ldr, y, ldy, yoff, scratch, scratch_bytes, stream);
}

// A whole Swin block + the adjust conv in one launch (kernels_fused_block.hip): the two ops above back to back, x being the shortcut.
// folded: the same block with the folded second half (mlp_fold.h): the three packs the kernel still reads, then [A | A W2] and
// A b2 + b_a composed behind the hi packs' layout in scratch
static int op_swin_block(bool folded, int precision, const float* x, int ldx, int B, int H, int W, int shift, int d, int heads, int m, int no,
                         const float* ln1_g, const float* ln1_b, const float* w_qkv, const float* b_qkv, const float* table,
                         const float* w_proj, const float* b_proj, const float* ln2_g, const float* ln2_b, const float* w_fc1,
                         const float* b_fc1, const float* w_fc2, const float* b_fc2, const float* w_adj, const float* b_adj, int act,
                         float slope, float alpha, const float* r, int ldr, float* y, int ldy, int yoff, void* scratch, size_t scratch_bytes, void* stream) {
  const char* const who = folded ? "op_swin_block_folded" : "op_swin_block";
  SRAD_REQUIRE(x && ln1_g && ln1_b && w_qkv && b_qkv && table && w_proj && b_proj && ln2_g && ln2_b && w_fc1 && b_fc1 && w_fc2 && b_fc2 && w_adj &&
                   b_adj && y && scratch, "%s: null argument", who);
  if (folded)
    SRAD_REQUIRE(srad_swin_block_fold_supported(precision, 8, B, H, W, d, heads, m, no),
                 "op_swin_block_folded: unsupported: precision %d, %dx%dx%d, d=%d heads=%d m=%d no=%d (bf16, 8 x 8 windows, windows x 4 <= CUs, no <= 32 or > 128)",
                 precision, B, H, W, d, heads, m, no);
  else
    SRAD_REQUIRE(srad_swin_block_supported(precision, 8, B, H, W, d, heads, m, no),
                 "op_swin_block: unsupported: precision %d, %dx%dx%d, d=%d heads=%d m=%d no=%d (bf16, 8 x 8 windows, windows x 4 <= CUs)", precision, B, H, W,
                 d, heads, m, no);
  size_t off[10];
  swin_scratch_parts(d, heads, m, no, off);                        // off[5]: where the lo packs would start = the size of the hi packs
  const MlpFoldLayout l = folded ? mf_layout(d, m, no) : MlpFoldLayout{};
  const size_t need = off[5] + (folded ? l.bytes : 0);
  SRAD_REQUIRE(scratch_bytes >= need && ((uintptr_t)scratch & 255) == 0, "%s: scratch %zu bytes, %zu needed (256-byte aligned)", who, scratch_bytes, need);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  char* sc = reinterpret_cast<char*>(scratch);
  SRAD_TRY(srad_launch_pack_qkv_frag(w_qkv, sc + off[0], d, heads, s));
  SRAD_TRY(srad_launch_pack_weight_frag(w_proj, sc + off[1], d, d, s));
  SRAD_TRY(srad_launch_pack_weight_frag(w_fc1, sc + off[2], m, d, s));
  SwinBlockParams q{};
  q.x = x; q.ldx = ldx; q.B = B; q.H = H; q.W = W; q.shift = shift; q.d = d; q.heads = heads; q.m = m; q.no = no;
  q.ln1_g = ln1_g; q.ln1_b = ln1_b; q.w_qkv = sc + off[0]; q.b_qkv = b_qkv; q.table = table;
  q.w_proj = sc + off[1]; q.w_fc1 = sc + off[2];
  q.b_proj = b_proj; q.b_fc1 = b_fc1; q.b_fc2 = b_fc2; q.ln2_g = ln2_g; q.ln2_b = ln2_b;
  q.act = act; q.slope = slope; q.alpha = alpha; q.R = r; q.ldr = ldr; q.Y = y; q.ldy = ldy; q.yoff = yoff;
  if (folded) {
    char* const fold = sc + off[5];
    SRAD_TRY(srad_mlp_fold_from_sources(l, fold, w_fc2, b_fc2, w_adj, b_adj, s));
    q.w_fc2 = fold + l.pack; q.w_adj = fold + l.pack; q.b_adj = reinterpret_cast<const float*>(fold + l.bias);
    return srad_launch_swin_block_folded(q, s);
  }
  SRAD_TRY(srad_launch_pack_weight_frag(w_fc2, sc + off[3], d, m, s));
  SRAD_TRY(srad_launch_pack_weight_frag(w_adj, sc + off[4], no, d, s));
  q.w_fc2 = sc + off[3]; q.w_adj = sc + off[4]; q.b_adj = b_adj;
  return srad_launch_swin_block(q, s);
}
int srad_op_swin_block(int precision, const float* x, int ldx, int B, int H, int W, int shift, int d, int heads, int m, int no,
                       const float* ln1_g, const float* ln1_b, const float* w_qkv, const float* b_qkv, const float* table,
                       const float* w_proj, const float* b_proj, const float* ln2_g, const float* ln2_b, const float* w_fc1,
                       const float* b_fc1, const float* w_fc2, const float* b_fc2, const float* w_adj, const float* b_adj, int act,
                       float slope, float alpha, const float* r, int ldr, float* y, int ldy, int yoff, void* scratch, size_t scratch_bytes, void* stream) {
  return op_swin_block(false, precision, x, ldx, B, H, W, shift, d, heads, m, no, ln1_g, ln1_b, w_qkv, b_qkv, table, w_proj, b_proj, ln2_g, ln2_b,
                       w_fc1, b_fc1, w_fc2, b_fc2, w_adj, b_adj, act, slope, alpha, r, ldr, y, ldy, yoff, scratch, scratch_bytes, stream);
}
int srad_op_swin_block_folded(int precision, const float* x, int ldx, int B, int H, int W, int shift, int d, int heads, int m, int no,
                              const float* ln1_g, const float* ln1_b, const float* w_qkv, const float* b_qkv, const float* table,
                              const float* w_proj, const float* b_proj, const float* ln2_g, const float* ln2_b, const float* w_fc1,
                              const float* b_fc1, const float* w_fc2, const float* b_fc2, const float* w_adj, const float* b_adj,
                              int act, float slope, float alpha, const float* r, int ldr, float* y, int ldy, int yoff, void* scratch, size_t scratch_bytes, void* stream) {
  return op_swin_block(true, precision, x, ldx, B, H, W, shift, d, heads, m, no, ln1_g, ln1_b, w_qkv, b_qkv, table, w_proj, b_proj, ln2_g, ln2_b,
                       w_fc1, b_fc1, w_fc2, b_fc2, w_adj, b_adj, act, slope, alpha, r, ldr, y, ldy, yoff, scratch, scratch_bytes, stream);
}

// Diagnostic twin of srad_bench_qkv_attn + srad_bench_mlp_block for the one-launch block: microseconds per launch, back-to-back
// launches.  x, y: [B*H*W][320] fp32; the output goes to columns [d, d + no) of y (adjust_k's epilogue), or [0, no) where those do not fit.
int srad_bench_swin_block(const float* x, int B, int H, int W, int shift, int d, int heads, int m, int no, const float* w_fp32,
                          float* y, void* scratch, size_t scratch_bytes, int iters, float* us_out, void* stream) {
  SRAD_REQUIRE(x && w_fp32 && y && scratch && us_out && iters > 0, "bench_swin_block: bad argument");
  const bool folded = (shift & 0x20000) != 0;       // bit 17 of `shift`: the folded second half, [A | A W2] cut from w_fp32 like every weight
  shift &= 0xffff;
  SRAD_REQUIRE(srad_swin_block_supported(SRAD_PREC_BF16, 8, B, H, W, d, heads, m, no) && no <= 320, "bench_swin_block: unsupported shape");
  SRAD_REQUIRE(!folded || srad_swin_block_fold_supported(SRAD_PREC_BF16, 8, B, H, W, d, heads, m, no), "bench_swin_block: no folded form for this shape");
  size_t off[10];
  swin_scratch_parts(d, heads, m, no, off);
  SRAD_REQUIRE(scratch_bytes >= off[5] && ((uintptr_t)scratch & 255) == 0, "bench_swin_block: scratch too small or not 256-byte aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  char* sc = reinterpret_cast<char*>(scratch);
  SRAD_TRY(srad_launch_pack_qkv_frag(w_fp32, sc + off[0], d, heads, s));
  SRAD_TRY(srad_launch_pack_weight_frag(w_fp32, sc + off[1], d, d, s));
  SRAD_TRY(srad_launch_pack_weight_frag(w_fp32, sc + off[2], m, d, s));
  SRAD_TRY(srad_launch_pack_weight_frag(w_fp32, sc + off[3], d, m, s));
  SRAD_TRY(srad_launch_pack_weight_frag(w_fp32, sc + off[4], no, d, s));
  SwinBlockParams q{};
  q.x = x; q.ldx = 320; q.B = B; q.H = H; q.W = W; q.shift = shift; q.d = d; q.heads = heads; q.m = m; q.no = no;
  q.ln1_g = q.ln1_b = q.b_qkv = q.table = w_fp32; q.w_qkv = sc + off[0];
  q.w_proj = sc + off[1]; q.w_fc1 = sc + off[2]; q.w_fc2 = sc + off[3]; q.w_adj = sc + off[4];
  q.b_proj = q.b_fc1 = q.b_fc2 = q.b_adj = q.ln2_g = q.ln2_b = w_fp32;
  q.act = SRAD_ACT_LRELU; q.slope = 0.2f; q.alpha = 1.f; q.Y = y; q.ldy = 320; q.yoff = d + no <= 320 ? d : 0;
  if (folded) {                                     // the pack of a [no][32 (KC + KCM)] matrix over the fc2 and adjust packs' space
    const MlpFoldLayout l = mf_layout(d, m, no);
    SRAD_REQUIRE(off[5] - off[3] >= (size_t)srad_np(no) * l.kf * 2, "bench_swin_block: the folded pack does not fit the scratch layout");
    SRAD_TRY(srad_launch_pack_weight_frag(w_fp32, sc + off[3], no, l.kf, s));
    q.w_adj = sc + off[3];
  }
  const auto launch = folded ? srad_launch_swin_block_folded : srad_launch_swin_block;
  for (int i = 0; i < 3; ++i) SRAD_TRY(launch(q, s));
  hipEvent_t e0, e1;
  SRAD_CHECK_HIP(hipEventCreate(&e0));
  SRAD_CHECK_HIP(hipEventCreate(&e1));
  SRAD_CHECK_HIP(hipEventRecord(e0, s));
  for (int i = 0; i < iters; ++i) SRAD_TRY(launch(q, s));
  SRAD_CHECK_HIP(hipEventRecord(e1, s));
  SRAD_CHECK_HIP(hipEventSynchronize(e1));
  float ms = 0.f;
  SRAD_CHECK_HIP(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  *us_out = ms * 1e3f / iters;
  return SRAD_OK;
}

// WgradParams of an op-level call, filled as the engines fill theirs (drn_wgrad, csrc/drn_train.hip): stored extents N / Cin, the
// real ones of dW, the channel groups and dY's first column
static int op_wgrad_params(const char* who, const void* dy, int ldy, int ycol0, int dy_bf16, const void* x, int ldx, int x_bf16, int B,
                           int Hi, int Wi, int N, int Cin, int n_real, int cin_real, int grp_real, int grp_pad, int ntaps, int stride,
                           const float* row_scale, float alpha, float* dw, float* db, WgradParams* out) {
  SRAD_REQUIRE(dy && x && dw, "%s: null argument", who);
  SRAD_REQUIRE(stride == 1 || stride == 2, "%s: stride must be 1 or 2", who);
  WgradParams p{};
  const int pad = ntaps == 9 ? 1 : 0, k = ntaps == 9 ? 3 : 1;
  p.Hi = Hi; p.Wi = Wi; p.Ho = (Hi + 2 * pad - k) / stride + 1; p.Wo = (Wi + 2 * pad - k) / stride + 1; p.stride = stride;
  p.dY = reinterpret_cast<const float*>(dy); p.ldy = ldy; p.ycol0 = ycol0; p.dy_bf16 = dy_bf16 ? 1 : 0;
  p.X = reinterpret_cast<const float*>(x); p.ldx = ldx; p.x_bf16 = x_bf16 ? 1 : 0;
  p.M = B * p.Ho * p.Wo;
  p.N = N; p.Cin = Cin; p.n_real = n_real; p.cin_real = cin_real; p.grp_real = grp_real; p.grp_pad = grp_pad; p.ntaps = ntaps;
  p.row_scale = row_scale; p.rps = p.Ho * p.Wo; p.alpha = alpha; p.dW = dw; p.db = db;
  *out = p;
  return SRAD_OK;
}

static int op_wgrad_run(int precision, const WgradParams& p, void* workspace, void* stream) {
  SRAD_REQUIRE(workspace, "op_wgrad: null argument");
  SRAD_REQUIRE(((uintptr_t)workspace & 255) == 0, "op_wgrad: workspace must be 256-byte aligned");
  WgradQueue q = wgrad_queue_on(reinterpret_cast<float*>(workspace), SRAD_WGRAD_WS_BYTES / sizeof(float));
  SRAD_TRY(srad_launch_wgrad(precision, p, q, reinterpret_cast<hipStream_t>(stream)));
  return srad_wgrad_flush(q, reinterpret_cast<hipStream_t>(stream));
}

int srad_op_wgrad(int precision, const float* dy, int ldy, const float* x, int ldx, int B, int Hi, int Wi, int N,
                  int Cin, int ntaps, int stride, const float* row_scale, float alpha, float* dw, float* db,
                  void* workspace, void* stream) {
  WgradParams p;
  SRAD_TRY(op_wgrad_params("op_wgrad", dy, ldy, 0, 0, x, ldx, 0, B, Hi, Wi, N, Cin, N, Cin, 0, 0, ntaps, stride, row_scale, alpha, dw, db, &p));
  return op_wgrad_run(precision, p, workspace, stream);
}

int srad_op_wgrad_ex(int precision, const float* dy, int ldy, int ycol0, const float* x, int ldx, int B, int Hi, int Wi, int N,
                     int Cin, int n_real, int cin_real, int grp_real, int grp_pad, int ntaps, int stride, const float* row_scale,
                     float alpha, float* dw, float* db, void* workspace, void* stream) {
  WgradParams p;
  SRAD_TRY(op_wgrad_params("op_wgrad", dy, ldy, ycol0, 0, x, ldx, 0, B, Hi, Wi, N, Cin, n_real, cin_real, grp_real, grp_pad, ntaps, stride,
                           row_scale, alpha, dw, db, &p));
  return op_wgrad_run(precision, p, workspace, stream);
}

// The plan of that call (include/srad.h): same parameters, same checks, no launch.  dW is not part of any decision.
int srad_op_wgrad_plan(int precision, const void* dy, int ldy, int ycol0, int dy_bf16, const void* x, int ldx, int x_bf16, int B,
                       int Hi, int Wi, int N, int Cin, int n_real, int cin_real, int grp_real, int grp_pad, int ntaps, int stride,
                       const float* row_scale, srad_wgrad_plan* plan) {
  WgradParams p;
  float* const no_dw = reinterpret_cast<float*>(uintptr_t(256));
  SRAD_TRY(op_wgrad_params("op_wgrad_plan", dy, ldy, ycol0, dy_bf16, x, ldx, x_bf16, B, Hi, Wi, N, Cin, n_real, cin_real, grp_real, grp_pad,
                           ntaps, stride, row_scale, 1.f, no_dw, nullptr, &p));
  return srad_plan_wgrad(precision, p, plan);
}

// Weight / bias gradient of the 80 -> 80 channel 3x3 convolution from bf16 operands (wgrad_conv9_kernel<5, YH, XH>, DRN's bf16
// chains): dy_h [B*H*W][80] bf16, x either bf16 (x_bf16 = 1) or fp32.  Fails if the shape does not take that kernel.
int srad_op_wgrad_conv9_h(const void* dy_h, const void* x, int x_bf16, int B, int H, int W, float* dw, float* db, void* workspace,
                          void* stream) {
  SRAD_REQUIRE(dy_h && x && dw && workspace, "op_wgrad_conv9_h: null argument");
  SRAD_REQUIRE(((uintptr_t)workspace & 255) == 0, "op_wgrad_conv9_h: workspace must be 256-byte aligned");
  WgradParams p{};
  p.Hi = p.Ho = H; p.Wi = p.Wo = W; p.stride = 1;
  p.dY = reinterpret_cast<const float*>(dy_h); p.ldy = 80; p.dy_bf16 = 1;
  p.X = reinterpret_cast<const float*>(x); p.ldx = 80; p.x_bf16 = x_bf16 ? 1 : 0;
  p.M = B * H * W; p.N = p.Cin = p.n_real = p.cin_real = 80; p.ntaps = 9; p.alpha = 1.f; p.dW = dw; p.db = db;
  SRAD_REQUIRE(srad_wgrad_conv9_supported(p), "op_wgrad_conv9_h: this shape does not take the nine-tap kernel");
  WgradQueue q = wgrad_queue_on(reinterpret_cast<float*>(workspace), SRAD_WGRAD_WS_BYTES / sizeof(float));
  SRAD_TRY(srad_launch_wgrad(SRAD_PREC_BF16, p, q, reinterpret_cast<hipStream_t>(stream)));
  return srad_wgrad_flush(q, reinterpret_cast<hipStream_t>(stream));
}

// A Linear layer's weight gradient the way the training step issues it: queued, sent with the (one-layer) deferred launch,
// reduced.  x_bf16 / dy_bf16: the operand pointer is a bf16 array (ld in elements).
int srad_op_wgrad_deferred(int precision, const void* dy, int ldy, int dy_bf16, const void* x, int ldx, int x_bf16, int M, int N,
                           int Cin, const float* row_scale, int rps, float alpha, float* dw, float* db, void* workspace,
                           void* stream) {
  SRAD_REQUIRE(dy && x && dw && workspace, "op_wgrad_deferred: null argument");
  WgradParams p{};
  p.dY = reinterpret_cast<const float*>(dy); p.ldy = ldy; p.X = reinterpret_cast<const float*>(x); p.ldx = ldx; p.M = M;
  p.N = N; p.Cin = Cin; p.n_real = N; p.cin_real = Cin; p.ntaps = 1; p.stride = 1;
  p.row_scale = row_scale; p.rps = rps; p.alpha = alpha; p.dW = dw; p.db = db; p.x_bf16 = x_bf16; p.dy_bf16 = dy_bf16;
  WgradQueue q = wgrad_queue_on(reinterpret_cast<float*>(workspace), SRAD_WGRAD_WS_BYTES / sizeof(float));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  SRAD_TRY(srad_launch_wgrad_deferred(precision, p, q, s));
  SRAD_TRY(srad_wgrad_launch_deferred(precision, q, s));
  return srad_wgrad_flush(q, s);
}

size_t srad_op_wgrad_workspace_bytes(void) { return SRAD_WGRAD_WS_BYTES; }

// WgradParams of a SRAD_WQ_WGRAD_DEFERRED step (i: ldy dy_bf16 ldx x_bf16 M N Cin rps;  p: dy x dw db row_scale)
static WgradParams wq_deferred_params(const srad_wq_step& t) {
  auto F = [](const void* v) { return reinterpret_cast<const float*>(v); };
  auto W = [](const void* v) { return const_cast<float*>(reinterpret_cast<const float*>(v)); };
  const int32_t* a = t.i;
  WgradParams g{};
  g.dY = F(t.p[0]); g.ldy = a[0]; g.dy_bf16 = a[1]; g.X = F(t.p[1]); g.ldx = a[2]; g.x_bf16 = a[3]; g.M = a[4];
  g.N = a[5]; g.Cin = a[6]; g.n_real = a[5]; g.cin_real = a[6]; g.ntaps = 1; g.stride = 1;
  g.row_scale = F(t.p[4]); g.rps = a[7]; g.alpha = t.alpha; g.dW = W(t.p[2]); g.db = W(t.p[3]);
  return g;
}

// The plan of a script's deferred layers (include/srad.h): the steps' own parameters, the launch's own decisions, no launch.
int srad_op_wgrad_deferred_plan(int precision, const srad_wq_step* steps, int nsteps, srad_wgrad_plan* plan) {
  SRAD_REQUIRE(steps && plan, "op_wgrad_deferred_plan: null argument");
  SRAD_REQUIRE(precision == SRAD_PREC_F32 || precision == SRAD_PREC_BF16, "op_wgrad_deferred_plan: precision must be fp32 or bf16");
  SRAD_REQUIRE(nsteps > 0 && nsteps <= SRAD_WGRAD_PLAN_LAYERS, "op_wgrad_deferred_plan: 1 to %d layers, not %d", SRAD_WGRAD_PLAN_LAYERS, nsteps);
  WgradParams layers[SRAD_WGRAD_PLAN_LAYERS];
  for (int i = 0; i < nsteps; ++i) {
    SRAD_REQUIRE(steps[i].kind == SRAD_WQ_WGRAD_DEFERRED, "op_wgrad_deferred_plan: step %d is not a deferred weight gradient", i);
    SRAD_REQUIRE(steps[i].p[0] && steps[i].p[1] && steps[i].p[2], "op_wgrad_deferred_plan: step %d: null argument", i);
    layers[i] = wq_deferred_params(steps[i]);
  }
  return srad_plan_wgrad_deferred(precision, layers, nsteps, plan);
}

// A list of queue steps through ONE WgradQueue whose workspace is the first `budget_floats` floats of `workspace`: what a
// backward pass does to the queue, at sizes where the automatic flushes happen.  Every step kind and pointer is checked before
// anything is launched; a step that fails returns its error at once (nothing queued behind it is reduced).  Ends with the
// deferred launch and a flush.  *n_reduce = reduce launches made, why[i] = SRAD_WQ_FLUSH_* of launch i (the first why_cap).
int srad_op_wgrad_queue_script(int precision, const srad_wq_step* steps, int nsteps, size_t budget_floats, void* workspace,
                               size_t workspace_bytes, int* n_reduce, int* why, int why_cap, void* stream) {
  SRAD_REQUIRE(steps && nsteps > 0 && workspace && n_reduce && (why || why_cap == 0) && why_cap >= 0, "op_wgrad_queue_script: null argument");
  SRAD_REQUIRE(precision == SRAD_PREC_F32 || precision == SRAD_PREC_BF16, "op_wgrad_queue_script: precision must be fp32 or bf16");
  SRAD_REQUIRE(((uintptr_t)workspace & 255) == 0, "op_wgrad_queue_script: workspace must be 256-byte aligned");
  SRAD_REQUIRE(budget_floats > 0 && budget_floats <= workspace_bytes / sizeof(float),
               "op_wgrad_queue_script: a budget of %zu floats does not fit the workspace of %zu bytes", budget_floats, workspace_bytes);
  for (int i = 0; i < nsteps; ++i) {
    const srad_wq_step& t = steps[i];
    const void* const* p = t.p;
    switch (t.kind) {
      case SRAD_WQ_WGRAD: case SRAD_WQ_WGRAD_DEFERRED: SRAD_REQUIRE(p[0] && p[1] && p[2], "op_wgrad_queue_script: step %d: null argument", i); break;
      case SRAD_WQ_LN_BWD: SRAD_REQUIRE(p[0] && p[1] && p[2] && p[4], "op_wgrad_queue_script: step %d: null argument", i); break;
      case SRAD_WQ_ATTN_BWD: SRAD_REQUIRE(p[0] && p[1] && p[2] && p[3] && p[4], "op_wgrad_queue_script: step %d: null argument", i); break;
      case SRAD_WQ_LAUNCH_DEFERRED: case SRAD_WQ_FLUSH: break;
      default: return srad_set_error(SRAD_ERR_ARG, "op_wgrad_queue_script: step %d: unknown step kind %d", i, t.kind);
    }
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  WgradQueue q = wgrad_queue_on(reinterpret_cast<float*>(workspace), budget_floats);
  auto F = [](const void* v) { return reinterpret_cast<const float*>(v); };
  auto W = [](const void* v) { return const_cast<float*>(reinterpret_cast<const float*>(v)); };
  for (int i = 0; i < nsteps; ++i) {
    const srad_wq_step& t = steps[i];
    const int32_t* a = t.i;
    switch (t.kind) {
      case SRAD_WQ_WGRAD: {          // i: ldy ldx B Hi Wi N Cin ntaps stride;  p: dy x dw db row_scale
        const int ntaps = a[7], stride = a[8];
        SRAD_REQUIRE(stride == 1 || stride == 2, "op_wgrad_queue_script: step %d: stride must be 1 or 2", i);
        WgradParams g{};
        const int pad = ntaps == 9 ? 1 : 0, k = ntaps == 9 ? 3 : 1;
        g.Hi = a[3]; g.Wi = a[4]; g.Ho = (g.Hi + 2 * pad - k) / stride + 1; g.Wo = (g.Wi + 2 * pad - k) / stride + 1; g.stride = stride;
        g.dY = F(t.p[0]); g.ldy = a[0]; g.X = F(t.p[1]); g.ldx = a[1]; g.M = a[2] * g.Ho * g.Wo;
        g.N = a[5]; g.Cin = a[6]; g.n_real = a[5]; g.cin_real = a[6]; g.ntaps = ntaps;
        g.row_scale = F(t.p[4]); g.rps = g.Ho * g.Wo; g.alpha = t.alpha; g.dW = W(t.p[2]); g.db = W(t.p[3]);
        SRAD_TRY(srad_launch_wgrad(precision, g, q, s));
        break;
      }
      case SRAD_WQ_WGRAD_DEFERRED: { // i: ldy dy_bf16 ldx x_bf16 M N Cin rps;  p: dy x dw db row_scale
        SRAD_TRY(srad_launch_wgrad_deferred(precision, wq_deferred_params(t), q, s));
        break;
      }
      case SRAD_WQ_LAUNCH_DEFERRED: SRAD_TRY(srad_wgrad_launch_deferred(precision, q, s)); break;
      case SRAD_WQ_LN_BWD: {         // i: ldx accumulate rows C;  p: dxn x gamma dres out dgamma dbeta
        LnBwdParams l{};
        l.dxn = F(t.p[0]); l.ld_dxn = a[3]; l.x = F(t.p[1]); l.ldx = a[0]; l.gamma = F(t.p[2]); l.dres = F(t.p[3]); l.ld_dres = a[3];
        l.out = W(t.p[4]); l.ld_out = a[3]; l.accumulate = a[1]; l.dgamma = W(t.p[5]); l.dbeta = W(t.p[6]); l.rows = a[2]; l.C = a[3]; l.eps = 1e-5f;
        SRAD_TRY(srad_launch_ln_bwd(l, q, s));
        break;
      }
      case SRAD_WQ_ATTN_BWD: {       // i: B H W ws shift d heads hdp;  p: qkv dout dqkv table dtable
        SRAD_REQUIRE(a[6] > 0 && a[3] > 0, "op_wgrad_queue_script: step %d: bad attention geometry", i);
        AttnBwdParams ab{F(t.p[0]), F(t.p[1]), W(t.p[2]), nullptr, F(t.p[3]), W(t.p[4]), a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7]};
        SRAD_TRY(srad_launch_window_attn_bwd(precision, ab, q, s));
        break;
      }
      default: SRAD_TRY(srad_wgrad_flush(q, s)); break;    // SRAD_WQ_FLUSH
    }
  }
  SRAD_TRY(srad_wgrad_launch_deferred(precision, q, s));
  SRAD_TRY(srad_wgrad_flush(q, s));
  *n_reduce = q.log.count;
  for (int i = 0; i < q.log.count && i < why_cap && i < SRAD_WGRAD_LOG; ++i) why[i] = q.log.why[i];
  return SRAD_OK;
}

// tools/wgrad_bench.py: the five weight gradients of one Swin block (qkv, proj, fc1, fc2, adjust) exactly as the training
// step issues them - deferred into one launch, then the reduce - `iters` times.  storage bit 0: X operands are bf16,
// bit 1: dY operands are bf16.  All layers read the same two operand buffers (the timing does not care).
int srad_bench_wgrad_block(int M, int d, int hidden, int KA, int storage, const void* xbuf, const void* ybuf, float* dw,
                           void* workspace, int iters, void* stream) {
  SRAD_REQUIRE(xbuf && ybuf && dw && workspace && M > 0 && iters > 0, "bench_wgrad_block: bad argument");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int N[5] = {3 * d, d, hidden, d, KA}, C[5] = {d, d, d, hidden, d};
  WgradQueue q = wgrad_queue_on(reinterpret_cast<float*>(workspace), SRAD_WGRAD_WS_BYTES / sizeof(float));
  for (int it = 0; it < iters; ++it) {
    float* w = dw;
    for (int l = 0; l < 5; ++l) {
      WgradParams p{};
      p.dY = reinterpret_cast<const float*>(ybuf); p.ldy = N[l]; p.X = reinterpret_cast<const float*>(xbuf); p.ldx = C[l];
      p.M = M; p.N = N[l]; p.Cin = C[l]; p.n_real = N[l]; p.cin_real = C[l]; p.ntaps = 1; p.stride = 1; p.alpha = 1.f;
      p.dW = w; p.x_bf16 = storage & 1; p.dy_bf16 = (storage >> 1) & 1;
      w += (size_t)N[l] * C[l];
      SRAD_TRY(srad_launch_wgrad_deferred(SRAD_PREC_BF16, p, q, s));
    }
    SRAD_TRY(srad_wgrad_launch_deferred(SRAD_PREC_BF16, q, s));
    SRAD_TRY(srad_wgrad_flush(q, s));
  }
  return SRAD_OK;
}

int srad_op_dgrad(int precision, const float* dy, int ldy, int B, int H, int W, int N, const float* w, int Cin,
                  int ntaps, const float* r, int ldr, int rmode, float slope, float alpha, const float* row_scale,
                  float* dx, int ldx, void* scratch, size_t scratch_bytes, void* stream) {
  SRAD_REQUIRE(dy && w && dx && scratch, "op_dgrad: null argument");
  SRAD_REQUIRE((N & 3) == 0 && (Cin & 3) == 0, "op_dgrad: N and Cin must be multiples of 4");
  const size_t need = srad_packed_bytes(precision, Cin, N, ntaps);
  SRAD_REQUIRE(scratch_bytes >= need, "op_dgrad: scratch %zu bytes, %zu needed", scratch_bytes, need);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  SRAD_TRY(srad_launch_pack_weight_transposed(precision, w, scratch, N, Cin, ntaps, N, Cin, s));
  GemmParams p{};
  p.Hi = p.Ho = H; p.Wi = p.Wo = W; p.stride = 1;
  p.X = dy; p.ldx = ldy; p.M = B * H * W; p.Cin = N; p.Cp = srad_cp(N); p.ntaps = ntaps; p.ln_eps = 1e-5f;
  p.Wp = scratch; p.N = Cin; p.slope = slope; p.alpha = alpha;
  p.R = r; p.ldr = ldr; p.rmode = rmode; p.row_scale = row_scale; p.rps = H * W;
  p.Y = dx; p.ldy = ldx;
  return srad_launch_gemm(precision, p, s);
}

int srad_op_layernorm_bwd(const float* dxn, const float* x, int ldx, const float* gamma, const float* dres, float* out,
                          int accumulate, float* dgamma, float* dbeta, int rows, int C, void* workspace, void* stream) {
  SRAD_REQUIRE(dxn && x && gamma && out && workspace, "op_layernorm_bwd: null argument");
  LnBwdParams l{};
  l.dxn = dxn; l.ld_dxn = C; l.x = x; l.ldx = ldx; l.gamma = gamma; l.dres = dres; l.ld_dres = C;
  l.out = out; l.ld_out = C; l.accumulate = accumulate; l.dgamma = dgamma; l.dbeta = dbeta; l.rows = rows; l.C = C; l.eps = 1e-5f;
  WgradQueue q = wgrad_queue_on(reinterpret_cast<float*>(workspace), SRAD_WGRAD_WS_BYTES / sizeof(float));
  SRAD_TRY(srad_launch_ln_bwd(l, q, reinterpret_cast<hipStream_t>(stream)));
  return srad_wgrad_flush(q, reinterpret_cast<hipStream_t>(stream));
}

int srad_op_window_attn_bwd(int precision, const float* qkv, const float* dout, float* dqkv, const float* table, float* dtable,
                            int B, int H, int W, int ws, int shift, int d, int heads, int hdp, void* workspace, void* stream) {
  SRAD_REQUIRE(qkv && dout && dqkv && table && dtable && workspace, "op_window_attn_bwd: null argument");
  AttnBwdParams a{qkv, dout, dqkv, nullptr, table, dtable, B, H, W, ws, shift, d, heads, hdp};
  WgradQueue q = wgrad_queue_on(reinterpret_cast<float*>(workspace), SRAD_WGRAD_WS_BYTES / sizeof(float));
  SRAD_TRY(srad_launch_window_attn_bwd(precision, a, q, reinterpret_cast<hipStream_t>(stream)));
  return srad_wgrad_flush(q, reinterpret_cast<hipStream_t>(stream));
}

// The all-bf16 form (head dim <= 128): qkv_h [T][3][heads][hp] with q already scaled, dout_h [T][heads][hp] (padding columns
// are ignored), dqkv_h [T][3 d] - all bf16; table / dtable fp32.
int srad_op_window_attn_bwd_h(const void* qkv_h, const void* dout_h, void* dqkv_h, const float* table, float* dtable,
                              int B, int H, int W, int ws, int shift, int d, int heads, int hp, void* workspace, void* stream) {
  SRAD_REQUIRE(qkv_h && dout_h && dqkv_h && table && dtable && workspace, "op_window_attn_bwd_h: null argument");
  AttnBwdParams a{nullptr, nullptr, nullptr, reinterpret_cast<__bf16*>(dqkv_h), table, dtable, B, H, W, ws, shift, d, heads,
                  srad_round_up(d / (heads > 0 ? heads : 1), 4)};
  a.qkv_h = reinterpret_cast<const __bf16*>(qkv_h); a.dout_h = reinterpret_cast<const __bf16*>(dout_h); a.hp_h = hp;
  WgradQueue q = wgrad_queue_on(reinterpret_cast<float*>(workspace), SRAD_WGRAD_WS_BYTES / sizeof(float));
  SRAD_TRY(srad_launch_window_attn_bwd(SRAD_PREC_BF16, a, q, reinterpret_cast<hipStream_t>(stream)));
  return srad_wgrad_flush(q, reinterpret_cast<hipStream_t>(stream));
}

static size_t tfrag_bytes(int n, int cin) {   // fragment pack of W^T for W [n][cin]
  return srad_align_up(srad_packed_bytes(SRAD_PREC_BF16, srad_round_up(cin, 4), srad_round_up(n, 4), 1), 256);
}

size_t srad_op_mlp_bwd_scratch_bytes(int d, int m, int KA) {
  return tfrag_bytes(m, d) + tfrag_bytes(d, m) + tfrag_bytes(d, d) + (KA > 0 ? tfrag_bytes(KA, d) : 0);
}

int srad_op_mlp_bwd(int M, int d, int m, float* dx2, const float* hpre, const float* x1, const float* gamma,
                    const float* w_fc1, const float* w_fc2, const float* rs2, int rps, float* dh, float* dx1, float* dgamma,
                    float* dbeta, int KA, const float* dA, int ld_dA, const float* y_act, int ld_y, float slope,
                    float aalpha, const float* w_adj, float* dA_out, const float* w_proj, const float* rs1, float* dO,
                    void* scratch, size_t scratch_bytes, void* workspace, void* stream) {
  SRAD_REQUIRE(dx2 && hpre && x1 && gamma && w_fc1 && w_fc2 && dh && dx1 && scratch && workspace, "op_mlp_bwd: null argument");
  SRAD_REQUIRE(scratch_bytes >= srad_op_mlp_bwd_scratch_bytes(d, m, KA) && ((uintptr_t)scratch & 255) == 0,
               "op_mlp_bwd: scratch too small or not 256-byte aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  char* sp = reinterpret_cast<char*>(scratch);
  MlpBwdParams p{};
  p.M = M; p.d = d; p.m = m; p.dx2 = dx2; p.rs2 = rs2; p.rps = rps; p.hpre = hpre; p.dh = dh; p.x1 = x1; p.ln_g = gamma;
  p.dx1 = dx1; p.dgamma = dgamma; p.dbeta = dbeta;
  p.w_fc1t = sp; SRAD_TRY(srad_launch_pack_weight_frag_t(w_fc1, sp, m, d, s)); sp += tfrag_bytes(m, d);
  p.w_fc2t = sp; SRAD_TRY(srad_launch_pack_weight_frag_t(w_fc2, sp, d, m, s)); sp += tfrag_bytes(d, m);
  if (w_proj) {
    SRAD_REQUIRE(dO, "op_mlp_bwd: dO missing");
    p.w_projt = sp; SRAD_TRY(srad_launch_pack_weight_frag_t(w_proj, sp, d, d, s));
    p.rs1 = rs1; p.dO = dO;
  }
  sp += tfrag_bytes(d, d);
  if (KA > 0) {
    SRAD_REQUIRE(dA && w_adj, "op_mlp_bwd: adjust operands missing");
    p.KA = KA; p.dA = dA; p.ld_dA = ld_dA; p.y_act = y_act; p.ld_y = ld_y; p.slope = slope; p.aalpha = aalpha; p.dA_out = dA_out;
    p.w_adjt = sp; SRAD_TRY(srad_launch_pack_weight_frag_t(w_adj, sp, KA, d, s));
  }
  WgradQueue q = wgrad_queue_on(reinterpret_cast<float*>(workspace), SRAD_WGRAD_WS_BYTES / sizeof(float));
  SRAD_TRY(srad_launch_mlp_bwd(p, q, s));
  return srad_wgrad_flush(q, s);
}

size_t srad_op_lin_ln_bwd_scratch_bytes(int K, int d) { return tfrag_bytes(K, d); }

int srad_op_lin_ln_bwd(int M, int K, int d, const float* dY, const float* w, const float* x, int ldx, const float* gamma,
                       const float* dres, float* out, int ld_out, int accumulate, float* dgamma, float* dbeta, void* scratch,
                       size_t scratch_bytes, void* workspace, void* stream) {
  SRAD_REQUIRE(dY && w && x && gamma && out && scratch && workspace, "op_lin_ln_bwd: null argument");
  SRAD_REQUIRE(scratch_bytes >= tfrag_bytes(K, d) && ((uintptr_t)scratch & 255) == 0, "op_lin_ln_bwd: scratch too small or unaligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  SRAD_TRY(srad_launch_pack_weight_frag_t(w, scratch, K, d, s));
  LinLnBwdParams p{};
  p.M = M; p.K = K; p.d = d; p.dY = dY; p.ld_dy = K; p.w_t = scratch; p.x = x; p.ldx = ldx; p.ln_g = gamma;
  p.dres = dres; p.ld_dres = d; p.out = out; p.ld_out = ld_out; p.accumulate = accumulate; p.dgamma = dgamma; p.dbeta = dbeta;
  WgradQueue q = wgrad_queue_on(reinterpret_cast<float*>(workspace), SRAD_WGRAD_WS_BYTES / sizeof(float));
  SRAD_TRY(srad_launch_lin_ln_bwd(p, q, s));
  return srad_wgrad_flush(q, s);
}

size_t srad_op_gemm_scratch_bytes(int precision, int N, int Cin, int ntaps) {
  return srad_packed_bytes(precision, N, Cin, ntaps);
}

// WindowAttention core (reference src/drct.py:281-299 plus the roll/partition/reverse around it):
// qkv [B*H*W][3][heads][hdp] (head slices padded to hdp floats, hdp % 4 == 0, pad columns never read as data)
// -> out [B*H*W][d], raster token order.
int srad_op_window_attn(int precision, const float* qkv, float* out, const float* table, int B, int H, int W, int ws,
                        int shift, int d, int heads, int hdp, void* stream) {
  SRAD_REQUIRE(qkv && out && table, "op_window_attn: null argument");
  AttnParams a{qkv, out, table, B, H, W, ws, shift, d, heads, hdp};
  return srad_launch_window_attn(precision, a, reinterpret_cast<hipStream_t>(stream));
}

// ---- the two kernels of the 64 x 64-window attention of BASELINE config C5 (bf16), each on its own ----
// the factor q carries into the attention's bf16 operands (head_dim^-0.5 * log2 e), or 0 when this geometry does not take
// the bf16-operand path (srad_window_attn_bf16_in)
float srad_op_window_attn_qscale(int ws, int shift, int d, int heads) {
  float qs = 0.f;
  return srad_window_attn_bf16_in(SRAD_PREC_BF16, ws, shift, d, heads, &qs) ? qs : 0.f;
}
size_t srad_op_ln_qkv_scratch_bytes(int d, int heads) { return srad_align_up(srad_qkv_frag_bytes(d, heads > 0 ? heads : 1), 256); }
// LayerNorm1 + attn.qkv (src/drct.py:477, 278) -> qkv_h [M][3][heads][hdp] bf16: q times qscale, padding columns 0, column
// head_dim of every v slice 1 (ln_qkv_kernel).  M % 64 == 0.
int srad_op_ln_qkv(const float* x, int ldx, int M, int d, int heads, const float* ln_g, const float* ln_b, const float* w_qkv,
                   const float* b_qkv, void* qkv_h, int hdp, float qscale, void* scratch, size_t scratch_bytes, void* stream) {
  SRAD_REQUIRE(x && ln_g && ln_b && w_qkv && b_qkv && qkv_h && scratch, "op_ln_qkv: null argument");
  SRAD_REQUIRE(srad_ln_qkv_supported(SRAD_PREC_BF16, M, d, heads), "op_ln_qkv: unsupported shape M=%d d=%d heads=%d", M, d, heads);
  SRAD_REQUIRE(scratch_bytes >= srad_op_ln_qkv_scratch_bytes(d, heads) && ((uintptr_t)scratch & 255) == 0, "op_ln_qkv: scratch too small or not 256-byte aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  SRAD_TRY(srad_launch_pack_qkv_frag(w_qkv, scratch, d, heads, s));
  LnQkvParams q{};
  q.x = x; q.ldx = ldx; q.M = M; q.d = d; q.heads = heads; q.ln_g = ln_g; q.ln_b = ln_b; q.w_qkv = scratch; q.b_qkv = b_qkv;
  q.qkv_h = reinterpret_cast<__bf16*>(qkv_h); q.hdp = hdp; q.qscale = qscale;
  return srad_launch_ln_qkv(q, s);
}
// the attention on those operands (window_attn_kernel, ROW64 / QH path; src/drct.py:281-299 + roll / partition / reverse):
// qkv_h as above -> out [B*H*W][d] fp32
int srad_op_window_attn_bf16_in(const void* qkv_h, float* out, const float* table, int B, int H, int W, int ws, int shift, int d,
                                int heads, int hdp, void* stream) {
  SRAD_REQUIRE(qkv_h && out && table, "op_window_attn_bf16_in: null argument");
  float qs = 0.f;
  SRAD_REQUIRE(srad_window_attn_bf16_in(SRAD_PREC_BF16, ws, shift, d, heads, &qs), "op_window_attn_bf16_in: this geometry does not take bf16 operands");
  AttnParams a{nullptr, out, table, B, H, W, ws, shift, d, heads, hdp};
  a.qkv_h = reinterpret_cast<const __bf16*>(qkv_h);
  return srad_launch_window_attn(SRAD_PREC_BF16, a, reinterpret_cast<hipStream_t>(stream));
}

int srad_op_layernorm(const float* x, int ldx, float* y, int ldy, int rows, int C, const float* g, const float* b,
                      void* stream) {
  SRAD_REQUIRE(x && y && g && b, "op_layernorm: null argument");
  return srad_launch_layernorm(x, ldx, y, ldy, rows, C, g, b, 1e-5f, reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
