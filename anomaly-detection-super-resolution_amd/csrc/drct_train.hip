// drct_train.hip - DRCT training step on gfx950: forward that keeps what the backward needs, the
// backward itself, and the parameter plumbing around them.  Stands in for loss.backward() /
// optimizer.step() of reference src/trainer.py:186-205 on the model of src/drct.py (DropPath 107-133,
// SwinTransformerBlock.forward 472-512, RDG.forward 388-396, DRCT.forward 886-898).
//
// Memory plan (288 GB of HBM: nothing is recomputed except LayerNorm statistics and the softmax):
//   * parameters live in ONE flat fp32 buffer owned by the caller (PyTorch parameters are views of it),
//     gradients in a second flat buffer with the same offsets; srad_drct_sync_params() refreshes the
//     packed forward weights AND their transposed twins (data-gradient operand) in one launch.
//   * every RDG keeps its dense [T][embed + 4 gc] buffer; every Swin block keeps LN1(x), q|k|v, the
//     attention output, x + attn, LN2(.), fc1 pre-activation, GELU output and the block output.
//     ~2.8 k floats per token per block -> 5.5 GB for DRCT-L at 8 x 32 x 32 tokens.
//   * every parameter gradient (weights, biases, LayerNorm gamma / beta, the attention bias tables) leaves its kernel as split-K
//     partial sums in the queue's workspace (wgrad_queue.h); the reduce kernel sums them in a fixed order and ADDS the sum to the
//     flat gradient buffer: zero it per step.  None goes through an atomic.  What a Swin block takes: drct_train_plan.h.
#include "drct_engine.h"
#include "drct_train_plan.h"

namespace {

// ------------------------------------------------------------------------------------------ workspace
struct BlockSave { float *xn1, *qkv, *attn, *x1, *xn2, *hpre, *hact, *x2; };

struct TrainWs : DrctStemTail {
  std::vector<float*> dense;          // n_rdg + 1 buffers [T][D]
  std::vector<BlockSave> blk;
  // backward temporaries
  float *dimg, *dus, *dc2, *dc1, *dbody, *g0, *g1, *dxn, *dO, *dfeat, *dxin;
  float *dx2[2], *dx1[2], *dA[2], *dh[2], *dqkv[2];   // read by the side stream's weight gradients: two sets, alternating per block
  std::vector<float*> dup;            // gradient of upb[j]
  size_t bytes;
};

TrainWs plan_train_ws(const srad_drct* h, int B, int H, int W, void* base, size_t cap) {
  const srad_drct_config& c = h->cfg;
  const size_t T = (size_t)B * H * W;
  const int E = c.embed_dim, D = E + 4 * c.gc, F = c.num_feat;
  Bump bp(base, cap);
  TrainWs w;
  w.xin = bp.take(T * SRAD_IMG_CPAD);
  w.feat0 = bp.take(T * E);
  for (int i = 0; i <= c.n_rdg; ++i) w.dense.push_back(bp.take(T * D));
  for (const SwinW& sw : h->blocks) {
    BlockSave s;
    const int d = sw.d, q = 3 * sw.heads * hdp_of(d, sw.heads);
    s.xn1 = bp.take(T * d); s.qkv = bp.take(T * q); s.attn = bp.take(T * d); s.x1 = bp.take(T * d);
    s.xn2 = bp.take(T * d); s.hpre = bp.take(T * sw.hidden); s.hact = bp.take(T * sw.hidden); s.x2 = bp.take(T * d);
    w.blk.push_back(s);
  }
  w.body = bp.take(T * E); w.c1 = bp.take(T * E); w.c2 = bp.take(T * F);
  size_t t = T;
  for (size_t j = 0; j < h->up.size(); ++j) { t *= 4; w.upb.push_back(bp.take(t * F)); }
  const size_t Tout = t;
  w.outn = bp.take(Tout * SRAD_IMG_CPAD);
  w.dimg = bp.take(Tout * SRAD_IMG_CPAD);
  t = T;
  for (size_t j = 0; j < h->up.size(); ++j) { t *= 4; w.dup.push_back(bp.take(t * F)); }
  w.dus = bp.take((h->up.empty() ? T : Tout / 4) * 4 * F);
  w.dc2 = bp.take(T * F); w.dc1 = bp.take(T * E); w.dbody = bp.take(T * E);
  w.g0 = bp.take(T * D); w.g1 = bp.take(T * D);
  const BlockGradFloats n = block_grad_floats(T, E, h->dmax, h->hmax);     // what block_grads' placements are held to
  w.dxn = bp.take(n.dx); w.dO = bp.take(n.dx);
  for (int k = 0; k < 2; ++k) {
    w.dx2[k] = bp.take(n.dx); w.dx1[k] = bp.take(n.dx); w.dA[k] = bp.take(n.dA);
    w.dh[k] = bp.take(n.dh); w.dqkv[k] = bp.take(n.dqkv);
  }
  w.dfeat = bp.take(T * E); w.dxin = bp.take(T * SRAD_IMG_CPAD);
  w.bytes = bp.used;
  return w;
}

// dX = dY W : the forward GEMM on the transposed pack (rows = input channels, K = output channels)
GemmParams dgrad_gemm(const srad_drct* h, const ConvW& c, const float* dY, int ldy, int M, float* dX, int ldx) {
  GemmParams p{};
  const int npad = srad_round_up(c.n, 4), cpad = srad_round_up(c.cin, 4);
  p.X = dY; p.ldx = ldy; p.M = M; p.Cin = npad; p.Cp = srad_cp(npad); p.ntaps = c.ntaps;
  p.stride = 1; p.ln_eps = 1e-5f;
  p.Wp = h->ts.tarena + h->ts.t_off[c.w]; p.N = cpad; p.bias = nullptr;
  p.alpha = 1.f; p.Y = dX; p.ldy = ldx;
  return p;
}
WgradParams wgrad_of(const srad_drct* h, const ConvW& c, float* flat_grad, const float* dY, int ldy, int ycol0,
                     const float* X, int ldx, int M) {
  WgradParams p{};
  p.dY = dY; p.ldy = ldy; p.ycol0 = ycol0; p.X = X; p.ldx = ldx; p.M = M;
  p.N = srad_round_up(c.n, 4); p.Cin = srad_round_up(c.cin, 4); p.ntaps = c.ntaps;
  p.n_real = c.n; p.cin_real = c.cin; p.stride = 1; p.alpha = 1.f;
  p.dW = flat_grad + h->ts.flat_off[c.w];
  p.db = c.b >= 0 ? flat_grad + h->ts.flat_off[c.b] : nullptr;
  return p;
}
void geom(WgradParams& p, int H, int W) { p.Hi = p.Ho = H; p.Wi = p.Wo = W; }

// What plan_block (drct_train_plan.h) asks of the rest of the library about Swin block `sw` over T tokens whose adjust conv has
// KA outputs.  Per block and call, in the forward and in the backward: plain predicate calls, nothing allocated.
BlockCaps block_caps(const srad_drct* h, const SwinW& sw, int H, int W, int T, int KA) {
  const int prec = h->pt.prec, ws = h->cfg.window_size, d = sw.d;
  const std::vector<long long>& tf = h->ts.tf_off;
  BlockCaps c{};
  c.bf16 = prec == SRAD_PREC_BF16; c.window8 = ws == 8;
  c.unfused_override = srad_path_override(SRAD_PATH_UNFUSED_BLOCKS); c.fused_forward = h->fuse_mlp;
  c.qkv_attn = srad_qkv_attn_supported(prec, ws, H, W, d, sw.heads); c.mlp_block = srad_mlp_block_supported(prec, T, d, sw.hidden, KA);
  c.mlp_bwd0 = srad_mlp_bwd_supported(prec, T, d, sw.hidden, 0); c.mlp_bwd_ka = srad_mlp_bwd_supported(prec, T, d, sw.hidden, KA);
  c.lin_ln_bwd = srad_lin_ln_bwd_supported(prec, T, 3 * d, d); c.bf16_out = srad_mlp_bwd_bf16_out(T);
  if (!tf.empty()) {
    c.tf_qkv = tf[sw.qkv.w] >= 0; c.tf_proj = tf[sw.proj.w] >= 0; c.tf_fc1 = tf[sw.fc1.w] >= 0; c.tf_fc2 = tf[sw.fc2.w] >= 0;
    c.tf_adjust = tf[sw.adjust.w] >= 0;
  }
  c.hd = d / sw.heads;
  return c;
}
int attn_hp(const SwinW& sw) { return srad_round_up(sw.d / sw.heads, 8); }
const char* tfrag(const srad_drct* h, const ConvW& c) { return h->ts.tarena + h->ts.tf_off[c.w]; }   // fragments of the transposed weight

int train_check(const srad_drct* h, int B, int H, int W) {
  SRAD_REQUIRE(h->ts.ready, "drct training: call srad_drct_train_bind() and srad_drct_sync_params() first");
  SRAD_REQUIRE(B > 0 && H > 0 && W > 0, "drct training: empty input");
  const int ws = h->cfg.window_size;
  SRAD_REQUIRE((ws >= 1 && ws <= 16) || ws == 32 || ws == 64,
               "drct training: window sizes 1 .. 16, 32 and 64 (got %d; the reference's presets build 2, 4, 8, 16, 32 and 64)", ws);
  SRAD_REQUIRE(H % ws == 0 && W % ws == 0, "drct training: input %dx%d is not a multiple of the window size %d", H, W, ws);
  SRAD_REQUIRE((double)B * H * W * h->cfg.upscale * h->cfg.upscale * h->cfg.num_feat * 4.0 < 3.9e9 &&
               (double)B * H * W * 3 * h->dmax * 4.0 < 3.9e9, "drct training: batch too large for 32-bit offsets");
  return SRAD_OK;
}

// One call of the training forward or of the backward, as every stage of it needs it (the queue and the gradient: backward only)
struct Step {
  srad_drct* h; int B, H, W, T;
  const float* keep_scale;
  TrainWs w; hipStream_t s;
  float* G; WgradQueue wq; float* wq_base; size_t wq_half;
};
// Swin block bi = i * 5 + k of the step: its weights, its saves, its DropPath factors, its plan
struct Block {
  int bi, k, KA; const SwinW& sw; const BlockSave& sv; const float *ks1, *ks2; BlockPlan plan;
};
Block block_of(const Step& c, int bi) {
  const srad_drct* h = c.h;
  const int k = bi % 5, KA = k < 4 ? h->cfg.gc : h->cfg.embed_dim;
  const float* ks = c.keep_scale ? c.keep_scale + (size_t)(2 * bi) * c.B : nullptr;
  return {bi, k, KA, h->blocks[bi], c.w.blk[bi], ks, ks ? ks + c.B : nullptr, plan_block(block_caps(h, h->blocks[bi], c.H, c.W, c.T, KA))};
}

// ------------------------------------------------------------------------------------------ forward
// bf16: the two fused launches of the inference path, which also leave what the backward needs (LN1(x), q|k|v, x + attn,
// LN2(.), fc1 pre-activation, GELU(.), block output) and apply DropPath
int forward_block_fused(const Step& c, const Block& b, float* cur, float* nxt) {
  const srad_drct* h = c.h; const BlockSave& sv = b.sv;
  auto as_h = [](float* p) { return reinterpret_cast<__bf16*>(p); };
  QkvAttnParams a = drct_qkv_attn_params(h, b.sw, cur, c.B, c.H, c.W);
  a.out_h = as_h(sv.attn);                                           // bf16 hand-off to mlp_block (and to the proj weight gradient)
  // the tensors only the weight gradients read (LN1(x), LN2(.), GELU(.), the block output) are left as bf16, which is
  // what the MFMA would round them to anyway: half the bytes written here and read (3 - 9 times each) by wgrad
  a.save_xn_h = as_h(sv.xn1); a.hdp = hdp_of(b.sw.d, b.sw.heads);
  if (b.plan.attn_h) { a.save_qkv_h = as_h(sv.qkv); a.hp_h = attn_hp(b.sw); }   // as the MFMA took them
  else a.save_qkv = sv.qkv;
  SRAD_TRY(srad_launch_qkv_attn(a, c.s));
  MlpBlockParams q = drct_mlp_block_params(h, b.sw, b.k, as_h(sv.attn), cur, nxt, c.T);
  q.rs1 = b.ks1; q.rs2 = b.ks2; q.rps = c.H * c.W;
  q.save_x1 = sv.x1;
  if (b.plan.yh_dh) q.save_hpre_h = as_h(sv.hpre);                   // GELU' takes it as bf16 in the bf16-output mlp_bwd
  else q.save_hpre = sv.hpre;
  q.save_xn2_h = as_h(sv.xn2); q.save_hact_h = as_h(sv.hact); q.save_x2_h = as_h(sv.x2);
  return srad_launch_mlp_block(q, c.s);
}

// The eight launches of a block, every save fp32
int forward_block_chain(const Step& c, const Block& b, float* cur, float* nxt) {
  const srad_drct* h = c.h; const srad_drct_config& cf = h->cfg; hipStream_t s = c.s;
  const SwinW& sw = b.sw; const BlockSave& sv = b.sv;
  const int prec = cf.precision, T = c.T, HW = c.H * c.W, D = cf.embed_dim + 4 * cf.gc, d = sw.d, hdp = hdp_of(d, sw.heads);
  SRAD_TRY(srad_launch_layernorm(cur, D, sv.xn1, d, T, d, h->pt.fptr(sw.n1g), h->pt.fptr(sw.n1b), 1e-5f, s));
  GemmParams qkv = drct_gemm(h, sw.qkv, sv.xn1, d, T, sv.qkv, 3 * sw.heads * hdp);
  qkv.hsplit_hd = d / sw.heads; qkv.hsplit_hdp = hdp;
  SRAD_TRY(srad_launch_gemm(prec, qkv, s));
  AttnParams a{sv.qkv, sv.attn, h->pt.fptr(sw.table), c.B, c.H, c.W, cf.window_size, sw.shift, d, sw.heads, hdp};
  SRAD_TRY(srad_launch_window_attn(prec, a, s));
  GemmParams proj = drct_gemm(h, sw.proj, sv.attn, d, T, sv.x1, d);           // x1 = shortcut + drop_path(proj(attn))   (drct.py:300, 509)
  proj.R = cur; proj.ldr = D; proj.row_scale = b.ks1; proj.rps = HW;
  SRAD_TRY(srad_launch_gemm(prec, proj, s));
  SRAD_TRY(srad_launch_layernorm(sv.x1, d, sv.xn2, d, T, d, h->pt.fptr(sw.n2g), h->pt.fptr(sw.n2b), 1e-5f, s));
  GemmParams fc1 = drct_gemm(h, sw.fc1, sv.xn2, d, T, sv.hact, sw.hidden);    // fc1 + GELU, pre-activation kept         (drct.py:185-186)
  fc1.act = SRAD_ACT_GELU; fc1.Ypre = sv.hpre;
  SRAD_TRY(srad_launch_gemm(prec, fc1, s));
  GemmParams fc2 = drct_gemm(h, sw.fc2, sv.hact, sw.hidden, T, sv.x2, d);     // x2 = x1 + drop_path(fc2(.))             (drct.py:188, 510)
  fc2.R = sv.x1; fc2.ldr = d; fc2.row_scale = b.ks2; fc2.rps = HW;
  SRAD_TRY(srad_launch_gemm(prec, fc2, s));
  GemmParams adj = drct_gemm(h, sw.adjust, sv.x2, d, T, b.k < 4 ? cur : nxt, D);
  if (b.k < 4) { adj.yoff = d; adj.act = SRAD_ACT_LRELU; adj.slope = 0.2f; }  // (drct.py:389-392)
  else { adj.alpha = 0.2f; adj.R = cur; adj.ldr = D; }                        // (drct.py:393, 396)
  return srad_launch_gemm(prec, adj, s);
}

// ------------------------------------------------------------------------------------------ backward
// Weight gradient (queued on the caller's stream), then data gradient (dX null: none), of a 3x3 conv over B x hh x ww pixels
int conv_backward(Step& c, const ConvW& cv, const float* dY, int ldy, const float* X, int ldx, int hh, int ww, float* dX, int ld_dx) {
  const int prec = c.h->cfg.precision, M = c.B * hh * ww;
  WgradParams g = wgrad_of(c.h, cv, c.G, dY, ldy, 0, X, ldx, M);
  geom(g, hh, ww);
  SRAD_TRY(srad_launch_wgrad(prec, g, c.wq, c.s));
  if (!dX) return SRAD_OK;
  GemmParams p = dgrad_gemm(c.h, cv, dY, ldy, M, dX, ld_dx);
  geom(p, hh, ww);
  return srad_launch_gemm(prec, p, c.s);
}
// out (+)= dres + LayerNorm'(dxn; x, gamma) over T rows of C channels, dgamma / dbeta into the flat gradient
LnBwdParams ln_bwd_of(const Step& c, int gamma, int beta, int C, const float* dxn, int ld_dxn, const float* x, int ldx,
                      const float* dres, int ld_dres, float* out, int ld_out, int accumulate = 0) {
  LnBwdParams l{};
  l.dxn = dxn; l.ld_dxn = ld_dxn; l.x = x; l.ldx = ldx; l.gamma = c.h->pt.fptr(gamma);
  l.dres = dres; l.ld_dres = ld_dres; l.out = out; l.ld_out = ld_out; l.accumulate = accumulate;
  l.dgamma = c.G + c.h->ts.flat_off[gamma]; l.dbeta = c.G + c.h->ts.flat_off[beta];
  l.rows = c.T; l.C = C; l.eps = 1e-5f;
  return l;
}

// Queues the weight gradient of a Swin block's layer for the block's one launch on the side stream.  dY in the form its view gives
// it (a bf16 dY carries its DropPath factor rs already), X as the forward saved it (bf16 iff the block's forward was fused).
int queue_wgrad(Step& c, const Block& b, hipStream_t side, const ConvW& cv, const Grad& dY, const float* rs, int rps,
                const float* X, int ldx, float alpha = 1.f) {
  WgradParams g = wgrad_of(c.h, cv, c.G, dY.f, dY.ld, 0, X, ldx, c.T);
  g.alpha = alpha; g.row_scale = dY.is_h() ? nullptr : rs; g.rps = rps; g.x_bf16 = b.plan.xh; g.dy_bf16 = dY.is_h();
  return srad_launch_wgrad_deferred(c.h->cfg.precision, g, c.wq, side);
}

// dy -> the gradient of the RDG stack's output in gn[:, :E]: conv_last, the Upsample stages, conv_before_upsample, conv_after_body, norm
int backward_output_end(Step& c, const float* dy, float* gn) {
  const srad_drct* h = c.h; const srad_drct_config& cf = h->cfg; const TrainWs& w = c.w;
  const int E = cf.embed_dim, D = E + 4 * cf.gc, F = cf.num_feat, stages = (int)h->up.size();
  const float zero3[3] = {0.f, 0.f, 0.f};
  int hh = c.H << stages, ww = c.W << stages;
  // dLoss/d(outn) = dy / img_range, NCHW -> NHWC (pad channels zero)           (drct.py:897)
  SRAD_TRY(srad_launch_nchw_to_nhwc(dy, w.dimg, c.B, cf.in_chans, SRAD_IMG_CPAD, hh, ww, zero3, 1.0f / cf.img_range, c.s));
  SRAD_TRY(conv_backward(c, h->conv_last, w.dimg, SRAD_IMG_CPAD, stages ? w.upb[stages - 1] : w.c2, F, hh, ww,      // (drct.py:895)
                         stages ? w.dup[stages - 1] : w.dc2, F));
  for (int j = stages - 1; j >= 0; --j) {   // Upsample stage j: conv F -> 4F + PixelShuffle(2)   (drct.py:694-713)
    hh /= 2; ww /= 2;
    SRAD_TRY(srad_launch_unshuffle(w.dup[j], w.dus, c.B, hh, ww, F, c.s));
    SRAD_TRY(conv_backward(c, h->up[j], w.dus, 4 * F, j ? w.upb[j - 1] : w.c2, F, hh, ww, j ? w.dup[j - 1] : w.dc2, F));
  }
  // conv_before_upsample + LeakyReLU(0.01), then conv_after_body(...) + x      (drct.py:844-845, 893)
  SRAD_TRY(srad_launch_dact(w.dc2, F, w.c2, F, w.dc2, F, c.T, F, 0.01f, c.s));
  SRAD_TRY(conv_backward(c, h->conv_before_up, w.dc2, F, w.c1, E, c.H, c.W, w.dc1, E));
  SRAD_TRY(conv_backward(c, h->conv_after_body, w.dc1, E, w.body, E, c.H, c.W, w.dbody, E));
  // norm                                                                        (drct.py:881)
  SRAD_TRY(srad_launch_ln_bwd(ln_bwd_of(c, h->norm_g, h->norm_b, E, w.dbody, E, w.dense[cf.n_rdg], D, nullptr, 0, gn, D), c.wq, c.s));
  return srad_wgrad_flush(c.wq, c.s);
}

// One Swin block with its adjust conv, on buffer set `set`: gn = the RDG's output gradient, gc = the running gradient of its dense
// buffer `cur`, which gc[:, :d] gains this block's input gradient in.  The data-gradient chain goes on the caller's stream; the
// five weight gradients are queued as they become ready and go out as one launch on the side stream at the end.
int backward_block(Step& c, BwdStreams& bs, const Block& b, int set, const float* cur, float* gn, float* gc) {
  srad_drct* h = c.h; const srad_drct_config& cf = h->cfg; const TrainWs& w = c.w; hipStream_t s = c.s, side = bs.side;
  const SwinW& sw = b.sw; const BlockSave& sv = b.sv; const BlockPlan& plan = b.plan;
  const int prec = cf.precision, T = c.T, HW = c.H * c.W, D = cf.embed_dim + 4 * cf.gc, d = sw.d, KA = b.KA;
  const int saved = h->saved_h[b.bi];     // what form the forward left this block's saves in (see srad_drct_forward_train)
  if (plan.xh && saved != block_saved_form(plan))
    return srad_set_error(SRAD_ERR_STATE, "drct_backward: block %d was saved by the forward for other backward kernels than this call "
                          "takes (q|k|v %s, fc1 pre-activation %s): the unfused_blocks path override must not change between the two",
                          b.bi, (saved & DRCT_SAVED_QKV_H) ? "bf16" : "fp32", (saved & DRCT_SAVED_HPRE_H) ? "bf16" : "fp32");
  SRAD_REQUIRE(block_grads_fit(plan, block_grad_floats(T, cf.embed_dim, h->dmax, h->hmax), T, d, sw.hidden, KA),
               "drct_backward: block %d: the bf16 gradients do not fit their buffers", b.bi);
  SRAD_TRY(bs.main_waits_set(set));                   // block n - 2 fully consumed
  SRAD_TRY(srad_wgrad_rebind(c.wq, "drct_backward", c.wq_base + (size_t)set * c.wq_half, c.wq_half));   // peak restarts: it is per block
  const BlockGrads g = block_grads(plan, {w.dx2[set], w.dx1[set], w.dA[set], w.dh[set], w.dqkv[set], w.dO, sv.qkv, sv.hpre}, T, d, sw.hidden, KA);
  // ---- adjust_k: 1x1 conv (+ LeakyReLU 0.2 | * 0.2)                        (drct.py:389-393)
  // adjust1-4 take their slice of gc through LeakyReLU' (a launch here, or mlp_bwd's prologue); adjust5 takes gn times 0.2: the
  // weight gradient reads gn itself (fp32, ld D), or with bf16 forms the copy mlp_bwd leaves behind the bf16 dh (every layer of
  // the deferred launch is bf16 then)
  const float aalpha = b.k < 4 ? 1.f : 0.2f;
  const Grad dA = b.k < 4 ? g.dA : plan.yh_dx2 ? g.dA5 : Grad{gn, nullptr, D};
  if (b.k < 4 && !plan.fuse_adj) SRAD_TRY(srad_launch_dact(gc + d, D, cur + d, D, dA.f, KA, T, KA, 0.2f, s));
  SRAD_TRY(queue_wgrad(c, b, side, sw.adjust, dA, nullptr, 0, sv.x2, d, aalpha));
  if (!plan.fuse_adj) {
    GemmParams p = dgrad_gemm(h, sw.adjust, dA.f, dA.ld, T, g.dx2.f, d);
    p.alpha = aalpha;
    SRAD_TRY(srad_launch_gemm(prec, p, s));
  }
  // ---- MLP branch: x2 = x1 + rs2 * fc2(gelu(fc1(LN2(x1))))                 (drct.py:510, 184-190)
  // the gradients only the weight gradients (and bf16 MFMA stagings) read go out as bf16 too: dh always when the MLP
  // backward is fused, dx2 (pre-multiplied by its DropPath factor) when the adjust prologue computes it in that launch
  SRAD_TRY(queue_wgrad(c, b, side, sw.fc2, g.dx2, b.ks2, HW, sv.hact, sw.hidden));
  SRAD_TRY(queue_wgrad(c, b, side, sw.fc1, g.dh, nullptr, 0, sv.xn2, d));
  if (plan.fuse_mlp) {   // both data gradients and the LayerNorm2 backward in one launch (kernels_fused_bwd.hip)
    MlpBwdParams mb{};
    mb.M = T; mb.d = d; mb.m = sw.hidden; mb.dx2 = g.dx2.f; mb.dx2s_h = g.dx2.h; mb.rs2 = b.ks2; mb.rps = HW;
    mb.w_fc2t = tfrag(h, sw.fc2); mb.hpre = g.hpre.f; mb.hpre_h = g.hpre.h; mb.dh = g.dh.f; mb.dh_h = g.dh.h;
    mb.w_fc1t = tfrag(h, sw.fc1); mb.x1 = sv.x1; mb.ln_g = h->pt.fptr(sw.n2g); mb.dx1 = g.dx1.f; mb.dx1s_h = g.dx1s.h;
    mb.dgamma = c.G + h->ts.flat_off[sw.n2g]; mb.dbeta = c.G + h->ts.flat_off[sw.n2b];
    if (plan.fuse_adj) {   // ... and the adjust conv's data gradient (with its LeakyReLU') in front of them
      mb.KA = KA; mb.w_adjt = tfrag(h, sw.adjust); mb.aalpha = aalpha; mb.slope = 0.2f;
      if (b.k < 4) { mb.dA = gc + d; mb.ld_dA = D; mb.y_act = cur + d; mb.ld_y = D; mb.dA_out = g.dA.f; mb.dA_out_h = g.dA.h; }
      else { mb.dA = gn; mb.ld_dA = D; mb.dA_out_h = g.dA5.h; }
    }
    if (plan.fuse_proj) { mb.w_projt = tfrag(h, sw.proj); mb.rs1 = b.ks1; mb.dO = g.dO.f; }
    if (plan.attn_h) { mb.dO_h = g.dO.h; mb.dO_heads = sw.heads; mb.dO_hp = attn_hp(sw); }
    SRAD_TRY(srad_launch_mlp_bwd(mb, c.wq, s));
  } else {
    GemmParams p = dgrad_gemm(h, sw.fc2, g.dx2.f, d, T, g.dh.f, sw.hidden);
    p.row_scale = b.ks2; p.rps = HW; p.R = sv.hpre; p.ldr = sw.hidden; p.rmode = SRAD_RMODE_DGELU;
    SRAD_TRY(srad_launch_gemm(prec, p, s));
    SRAD_TRY(srad_launch_gemm(prec, dgrad_gemm(h, sw.fc1, g.dh.f, sw.hidden, T, w.dxn, d), s));
    // dx1 = dx2 + dLN2(dxn)
    SRAD_TRY(srad_launch_ln_bwd(ln_bwd_of(c, sw.n2g, sw.n2b, d, w.dxn, d, sv.x1, d, g.dx2.f, d, g.dx1.f, d), c.wq, s));
  }
  // ---- attention branch: x1 = x + rs1 * proj(attn(LN1(x)))                  (drct.py:477-509)
  SRAD_TRY(queue_wgrad(c, b, side, sw.proj, plan.yh_dx1 ? g.dx1s : g.dx1, b.ks1, HW, sv.attn, d));   // (yh_dx1: dx1 * rs1 as bf16, from mlp_bwd)
  if (!plan.fuse_proj) {
    GemmParams p = dgrad_gemm(h, sw.proj, g.dx1.f, d, T, g.dO.f, d);
    p.row_scale = b.ks1; p.rps = HW;
    SRAD_TRY(srad_launch_gemm(prec, p, s));
  }
  // dqkv as bf16 when both of its readers take it that way (the fused qkv + LayerNorm1 backward and the weight gradient)
  AttnBwdParams a{sv.qkv, g.dO.f, g.dqkv.f, g.dqkv.h, h->pt.fptr(sw.table), c.G + h->ts.flat_off[sw.table], c.B, c.H, c.W, cf.window_size,
                  sw.shift, d, sw.heads, hdp_of(d, sw.heads)};
  if (plan.attn_h) { a.qkv_h = g.qkv.h; a.dout_h = g.dO.h; a.hp_h = attn_hp(sw); }
  SRAD_TRY(srad_launch_window_attn_bwd(prec, a, c.wq, s));
  SRAD_TRY(queue_wgrad(c, b, side, sw.qkv, g.dqkv, nullptr, 0, sv.xn1, d));
  if (plan.fuse_qkv) {
    // gc[:, :d] += dx1 + dLN1(dqkv . Wqkv): data gradient + LayerNorm1 backward in one launch (kernels_fused_bwd.hip)
    LinLnBwdParams lb{};
    lb.M = T; lb.K = 3 * d; lb.d = d; lb.dY = g.dqkv.f; lb.ld_dy = 3 * d; lb.dy_bf16 = g.dqkv.is_h(); lb.w_t = tfrag(h, sw.qkv);
    lb.x = cur; lb.ldx = D; lb.ln_g = h->pt.fptr(sw.n1g); lb.dres = g.dx1.f; lb.ld_dres = d;
    lb.out = gc; lb.ld_out = D; lb.accumulate = 1;
    lb.dgamma = c.G + h->ts.flat_off[sw.n1g]; lb.dbeta = c.G + h->ts.flat_off[sw.n1b];
    SRAD_TRY(srad_launch_lin_ln_bwd(lb, c.wq, s));
  } else {
    SRAD_TRY(srad_launch_gemm(prec, dgrad_gemm(h, sw.qkv, g.dqkv.f, 3 * d, T, w.dxn, d), s));
    // gc[:, :d] += dx1 + dLN1(dxn)
    SRAD_TRY(srad_launch_ln_bwd(ln_bwd_of(c, sw.n1g, sw.n1b, d, w.dxn, d, cur, D, g.dx1.f, d, gc, D, 1), c.wq, s));
  }
  // this block's five weight gradients as ONE launch on the side stream (all their operands exist now), then
  // the reduce of their partials and of the LayerNorm / bias-table column sums the caller's stream has written
  SRAD_TRY(bs.side_waits_main());
  SRAD_TRY(srad_wgrad_launch_deferred(prec, c.wq, side));
  SRAD_TRY(srad_wgrad_flush(c.wq, side));
  h->ts.wgrad_block_peak = std::max(h->ts.wgrad_block_peak, c.wq.peak);
  return bs.set_done(set);
}

// gn = the gradient of the first RDG's input -> patch_embed.norm, conv_first, dx (null: no data gradient of conv_first)
int backward_input_end(Step& c, const float* gn, float* dx) {
  const srad_drct* h = c.h; const srad_drct_config& cf = h->cfg; const TrainWs& w = c.w;
  const int E = cf.embed_dim, D = E + 4 * cf.gc;
  const float zero3[3] = {0.f, 0.f, 0.f};
  // patch_embed.norm, joined by the long skip of conv_after_body(...) + x      (drct.py:873, 893)
  SRAD_TRY(srad_launch_ln_bwd(ln_bwd_of(c, h->pe_g, h->pe_b, E, gn, D, w.feat0, E, w.dc1, E, w.dfeat, E), c.wq, c.s));
  SRAD_TRY(conv_backward(c, h->conv_first, w.dfeat, E, w.xin, SRAD_IMG_CPAD, c.H, c.W, dx ? w.dxin : nullptr, SRAD_IMG_CPAD));   // (drct.py:892)
  if (dx) SRAD_TRY(srad_launch_nhwc_to_nchw(w.dxin, SRAD_IMG_CPAD, dx, c.B, cf.in_chans, c.H, c.W, zero3, cf.img_range, c.s));
  return srad_wgrad_flush(c.wq, c.s);
}

}  // namespace

extern "C" {

int srad_drct_train_param_floats(srad_drct_t* h, int64_t* total) {
  SRAD_REQUIRE(h && total, "train_param_floats: null argument");
  return train_param_floats(h->pt, h->ts, total);
}

int srad_drct_train_param_offset(srad_drct_t* h, int idx, int64_t* off_floats) {
  int64_t tot = 0;
  SRAD_REQUIRE(h, "train_param_offset: null argument");
  SRAD_TRY(train_param_floats(h->pt, h->ts, &tot));
  SRAD_REQUIRE(off_floats && idx >= 0 && idx < (int)h->pt.entries.size(), "train_param_offset: index %d out of range", idx);
  *off_floats = h->ts.flat_off[idx];
  return SRAD_OK;
}

int srad_drct_train_arena_bytes(srad_drct_t* h, size_t* bytes) {
  SRAD_REQUIRE(h && bytes, "train_arena_bytes: null argument");
  return train_arena_bytes(h->pt, h->ts, bytes);
}

// Binds the caller-owned training arena (transposed weight packs + the descriptor table of the sync kernel +
// the split-K workspace).  Synchronous; call once after srad_drct_bind_arena.
int srad_drct_train_bind(srad_drct_t* h, void* train_arena, size_t bytes) {
  SRAD_REQUIRE(h, "train_bind: null argument");
  h->saved_h.assign(h->blocks.size(), 0);          // no training forward has saved anything yet
  return train_bind(h->pt, h->ts, train_arena, bytes);
}

int srad_drct_train_set_wgrad_budget(srad_drct_t* h, size_t bytes) {
  SRAD_REQUIRE(h, "train_set_wgrad_budget: null argument");
  SRAD_REQUIRE(bytes > 0 && bytes % 512 == 0 && bytes <= SRAD_WGRAD_WS_BYTES,
               "train_set_wgrad_budget: %zu bytes: a multiple of 512 up to the %zu bytes the training arena holds", bytes, (size_t)SRAD_WGRAD_WS_BYTES);
  h->ts.wgrad_budget = bytes;
  return SRAD_OK;
}

int srad_drct_train_wgrad_stats(const srad_drct_t* h, int launches[3], size_t* block_peak_floats) {
  SRAD_REQUIRE(h && launches && block_peak_floats, "train_wgrad_stats: null argument");
  for (int i = 0; i < 3; ++i) launches[i] = h->ts.wgrad_log.by_why[i];
  *block_peak_floats = h->ts.wgrad_block_peak;
  return SRAD_OK;
}

// Refreshes every packed weight (forward and transposed) and raw parameter from the flat fp32 master buffer:
// one launch, to be called after each optimizer step (and once after loading a checkpoint).
int srad_drct_sync_params(srad_drct_t* h, const float* flat_params, void* stream) {
  SRAD_REQUIRE(h, "sync_params: null argument");
  SRAD_TRY(train_sync_params(h->pt, h->ts, flat_params, reinterpret_cast<hipStream_t>(stream)));
  h->gc.reset();
  return SRAD_OK;
}

int srad_drct_train_workspace_bytes(const srad_drct_t* h, int B, int H, int W, size_t* bytes) {
  SRAD_REQUIRE(h && bytes && B > 0 && H > 0 && W > 0, "train_workspace_bytes: bad argument");
  *bytes = plan_train_ws(h, B, H, W, nullptr, 0).bytes;
  return SRAD_OK;
}

// Gradient buckets in the order the backward completes them: 0 = everything after the RDGs (norm ...
// conv_last), 1 .. n_rdg = layers.(n_rdg-1) ... layers.0, n_rdg + 1 = conv_first + patch_embed.norm.
int srad_drct_num_buckets(const srad_drct_t* h) { return h ? h->cfg.n_rdg + 2 : 0; }

int srad_drct_bucket_range(srad_drct_t* h, int bucket, int64_t* off_floats, int64_t* n_floats) {
  SRAD_REQUIRE(h && off_floats && n_floats, "bucket_range: null argument");
  int64_t tot = 0;
  SRAD_TRY(train_param_floats(h->pt, h->ts, &tot));
  const int R = h->cfg.n_rdg;
  SRAD_REQUIRE(bucket >= 0 && bucket < R + 2, "bucket_range: bucket %d out of range", bucket);
  auto start_of_rdg = [&](int i) { return i < R ? h->ts.flat_off[h->blocks[i * 5].n1g] : h->ts.flat_off[h->norm_g]; };
  int64_t a, b;
  if (bucket == 0) { a = h->ts.flat_off[h->norm_g]; b = tot; }
  else if (bucket <= R) { const int i = R - bucket; a = start_of_rdg(i); b = start_of_rdg(i + 1); }
  else { a = 0; b = start_of_rdg(0); }
  *off_floats = a; *n_floats = b - a;
  return SRAD_OK;
}

// Training-mode DRCT.forward: as srad_drct_forward, with DropPath (src/drct.py:107-133) applied through
// `keep_scale` ([2 * n_blocks][B] floats: 0 or 1/keep_prob per sample, row 2j for the attention branch of
// block j and 2j+1 for its MLP branch; null = no DropPath) and every tensor the backward needs left in
// `workspace`, which the caller must hand unchanged to srad_drct_backward.
int srad_drct_forward_train(srad_drct_t* h, const float* x, int B, int H, int W, float* y, const float* keep_scale,
                            void* workspace, size_t workspace_bytes, void* stream) {
  SRAD_REQUIRE(h && x && y && workspace, "drct_forward_train: null argument");
  SRAD_TRY(train_check(h, B, H, W));
  SRAD_REQUIRE(((uintptr_t)workspace & 255) == 0, "drct_forward_train: workspace must be 256-byte aligned");
  const Step c{h, B, H, W, B * H * W, keep_scale, plan_train_ws(h, B, H, W, workspace, workspace_bytes), reinterpret_cast<hipStream_t>(stream)};
  const TrainWs& w = c.w;
  SRAD_REQUIRE(w.bytes <= workspace_bytes, "drct_forward_train: workspace %zu bytes, %zu needed", workspace_bytes, w.bytes);
  SRAD_TRY(drct_stem(h, x, B, H, W, w, w.dense[0], c.s));
  for (int bi = 0; bi < 5 * h->cfg.n_rdg; ++bi) {
    const Block b = block_of(c, bi);
    float *cur = w.dense[bi / 5], *nxt = w.dense[bi / 5 + 1];
    h->saved_h[bi] = (char)block_saved_form(b.plan);      // what srad_drct_backward must find its kernels take
    SRAD_TRY(b.plan.xh ? forward_block_fused(c, b, cur, nxt) : forward_block_chain(c, b, cur, nxt));
  }
  return drct_tail(h, w.dense[h->cfg.n_rdg], B, H, W, w, SRAD_IMG_CPAD, y, c.s);
}

// Backward of srad_drct_forward_train.  dy [B,C,H*s,W*s] is dLoss/dy; parameter gradients are ACCUMULATED
// into flat_grad (same offsets as the flat parameter buffer); dx (optional) receives dLoss/dx.
// `on_bucket(user, bucket)` (optional) is called on the host right after the last kernel that writes bucket
// `bucket` (srad_drct_bucket_range) has been enqueued - the hook a data-parallel trainer uses to start that
// bucket's all-reduce on another stream while the rest of the backward is still running.
int srad_drct_backward(srad_drct_t* h, const float* dy, int B, int H, int W, const float* keep_scale, float* dx,
                       float* flat_grad, void* workspace, size_t workspace_bytes, void* stream,
                       srad_bucket_fn on_bucket, void* user) {
  SRAD_REQUIRE(h && dy && flat_grad && workspace, "drct_backward: null argument");
  SRAD_TRY(train_check(h, B, H, W));
  // split-K partials of the weight gradients, reduced once per Swin block: each of the two buffer sets has half the workspace
  Step c{h, B, H, W, B * H * W, keep_scale, plan_train_ws(h, B, H, W, workspace, workspace_bytes), reinterpret_cast<hipStream_t>(stream),
         flat_grad, train_wgrad_queue(h->ts)};
  c.wq_base = c.wq.ws; c.wq_half = c.wq.ws_floats / 2;
  SRAD_REQUIRE(c.w.bytes <= workspace_bytes, "drct_backward: workspace %zu bytes, %zu needed", workspace_bytes, c.w.bytes);
  const int R = h->cfg.n_rdg, E = h->cfg.embed_dim, D = E + 4 * h->cfg.gc;
  // Two streams: the data-gradient chain (each kernel needs the previous one's output) stays on the caller's stream;
  // the weight gradients, which nothing in the backward waits for, run on a side stream and fill the idle CUs.
  // (default priority: a low-priority side stream gained nothing here, and a process that had created one ran later
  //  hipGraph replays of other models at half speed - measured with bench.py's C3 leg)
  BwdStreams& bs = h->bwd;
  SRAD_TRY(bs.begin(c.s));
  // a flush that a reservation makes in the middle of a block reduces column sums the caller's stream wrote: it goes there even
  // when the reservation is a deferred layer's (whose own launch, on the side stream, comes after side_waits_main)
  wgrad_queue_flush_on(c.wq, c.s);
  h->ts.wgrad_block_peak = 0;
  float *gn = c.w.g0, *gc = c.w.g1;     // gradient of the RDG stack's output lives in gn[:, :E]
  SRAD_TRY(backward_output_end(c, dy, gn));
  if (on_bucket) on_bucket(user, 0);
  int blk_count = 0;
  for (int i = R - 1; i >= 0; --i) {
    // gc = [ gn[:, :E] | 0 ]: the residual path of out = 0.2 x5 + x               (drct.py:396)
    SRAD_TRY(srad_launch_copy_cols(gn, D, gc, D, c.T, E, c.s));
    for (int k = 4; k >= 0; --k, ++blk_count) SRAD_TRY(backward_block(c, bs, block_of(c, i * 5 + k), blk_count & 1, c.w.dense[i], gn, gc));
    SRAD_TRY(bs.main_waits_side());                         // the RDG's gradients are final on the caller's stream
    std::swap(gn, gc);
    if (on_bucket) on_bucket(user, R - i);
  }
  SRAD_TRY(srad_wgrad_rebind(c.wq, "drct_backward", c.wq_base, 2 * c.wq_half));     // the remaining layers run on the caller's stream only
  SRAD_TRY(backward_input_end(c, gn, dx));
  h->ts.wgrad_log = c.wq.log;
  if (on_bucket) on_bucket(user, R + 1);
  return SRAD_OK;
}

}  // extern "C"
