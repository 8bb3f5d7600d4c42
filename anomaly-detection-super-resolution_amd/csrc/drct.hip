// drct.hip - DRCT-L forward engine + its C ABI (include/srad.h).
// Follows reference src/drct.py: DRCT.forward 886-898, forward_features 870-884, RDG.forward
// 388-396, SwinTransformerBlock.forward 472-512, Upsample 694-713.
//
// HBM layout: everything is NHWC == token-major [T = B*H*W][C] fp32, so PatchEmbed /
// PatchUnEmbed (drct.py:650-654,687-690) are no-ops.  Each RDG works in one dense buffer
// [T][embed+4*gc]: swin_k reads channels [0, d_k) and adjust_k writes channels [d_k, d_k+gc),
// which is exactly torch.cat((x, x1, ..), -1) without any copy.  Two dense buffers ping-pong
// between RDGs (adjust5 writes 0.2*x5 + x into the next one).
#include "../../include/srad.h"
#include <math.h>
#include <stdlib.h>
#include <new>

#include "drct_engine.h"

namespace {

struct DrctWs : DrctStemTail {
  float *dense0, *dense1, *qkv, *attn, *x1, *hid, *x2;
  size_t bytes;
};

DrctWs plan_ws(const srad_drct* h, int B, int H, int W, void* base, size_t cap) {
  const srad_drct_config& c = h->cfg;
  const size_t T = (size_t)B * H * W;
  const int E = c.embed_dim, D = E + 4 * c.gc;
  Bump bp(base, cap);
  DrctWs w;
  w.xin = bp.take(T * SRAD_IMG_CPAD);
  w.feat0 = bp.take(T * E);
  w.dense0 = bp.take(T * D);
  w.dense1 = bp.take(T * D);
  w.qkv = bp.take(T * h->qkvmax);
  w.attn = bp.take(T * h->dmax);
  w.x1 = bp.take(T * h->dmax);
  w.hid = bp.take(T * h->hmax);
  w.x2 = bp.take(T * h->dmax);
  w.body = bp.take(T * E);
  w.c1 = bp.take(T * E);
  w.c2 = bp.take(T * c.num_feat);
  size_t t = T;
  for (size_t j = 0; j < h->up.size(); ++j) {
    t *= 4;
    w.upb.push_back(bp.take(t * c.num_feat));
  }
  w.outn = bp.take(t * c.in_chans);
  w.bytes = bp.used;
  return w;
}

// How one Swin block of an inference forward runs: decided in drct_block_path, launched in forward_body.  First half (LayerNorm1,
// qkv, attention): in the one-launch block | qkv_attn | ln_qkv (bf16 q | k | v out; split-bf16: fp32 out) or the tiled GEMM, then
// the attention.  qkv_bf16 (64 x 64 windows, bf16): q | k | v are written as the attention's bf16 MFMA operands, scaled by qscale.
enum DrctFirstHalf { DRCT_H1_IN_BLOCK, DRCT_H1_QKV_ATTN, DRCT_H1_LN_QKV, DRCT_H1_LN_QKV_SPLIT, DRCT_H1_GEMM };
// Second half (proj .. adjust_k): in the block or as mlp_block, fc2 as it is or folded into the adjust conv | the four-GEMM chain
enum DrctSecondHalf { DRCT_H2_IN_BLOCK, DRCT_H2_IN_BLOCK_FOLDED, DRCT_H2_MLP_BLOCK, DRCT_H2_MLP_BLOCK_FOLDED, DRCT_H2_CHAIN };
struct DrctBlockPath { DrctFirstHalf first; DrctSecondHalf second; bool qkv_bf16; float qscale; };
// (no allocation and no string: this runs for every block of every eager forward)
DrctBlockPath drct_block_path(const srad_drct* h, const SwinW& sw, int k, int B, int H, int W, const DrctPaths& paths) {
  const srad_drct_config& c = h->cfg;
  const int prec = c.precision, ws = c.window_size, T = B * H * W, d = sw.d, no = k < 4 ? c.gc : c.embed_dim;
  DrctBlockPath p{DRCT_H1_GEMM, DRCT_H2_CHAIN, false, 1.f};
  const bool mlp_fused = h->fuse_mlp && srad_mlp_block_supported(prec, T, d, sw.hidden, no);
  // the whole block as ONE launch (kernels_fused_block.hip) where the windows' quarters fit the chip in one wave of workgroups
  // and the block shape measured a win over the pair below; this path has no saves and no DropPath
  if (mlp_fused && srad_swin_block_supported(prec, ws, B, H, W, d, sw.heads, sw.hidden, no) && srad_swin_block_wins(d, sw.heads, sw.hidden, no) &&
      !srad_path_override(SRAD_PATH_BLOCK_TWO_LAUNCHES)) {
    const bool folded = paths.mfold && srad_swin_block_fold_supported(prec, ws, B, H, W, d, sw.heads, sw.hidden, no);
    return DrctBlockPath{DRCT_H1_IN_BLOCK, folded ? DRCT_H2_IN_BLOCK_FOLDED : DRCT_H2_IN_BLOCK, false, 1.f};
  }
  if (h->fuse_mlp && srad_qkv_attn_supported(prec, ws, H, W, d, sw.heads)) p.first = DRCT_H1_QKV_ATTN;
  else {
    p.qkv_bf16 = srad_window_attn_bf16_in(prec, ws, sw.shift, d, sw.heads, &p.qscale);
    const auto ln_qkv = [&] { return srad_ln_qkv_supported(prec, T, d, sw.heads) && !srad_path_override(SRAD_PATH_QKV_VIA_GEMM); };
    if (p.qkv_bf16 && h->pt.frag_ptr(sw.qkv.w) && ln_qkv()) p.first = DRCT_H1_LN_QKV;
    else if (prec == SRAD_PREC_BF16X3 && ws == 64 && h->pt.frag_ptr(sw.qkv.w) && h->pt.frag_lo_ptr(sw.qkv.w) && ln_qkv()) p.first = DRCT_H1_LN_QKV_SPLIT;
  }
  // mlp_block folded on 16-row tiles only - the form the one-launch block's second half has: a forward on 32- or
  // 64-row tiles keeps the chain (tests/test_gpu_mlp_fold.py; the wider folded instances exist at the op level)
  if (mlp_fused)
    p.second = paths.mfold && srad_mlp_block_rows(T) == 16 && srad_mlp_block_fold_supported(prec, T, d, sw.hidden, no) ? DRCT_H2_MLP_BLOCK_FOLDED : DRCT_H2_MLP_BLOCK;
  return p;
}

// w_adj / b_adj of a folded launch: the pack [A | A W2] and the bias A b2 + b_a in block blk's region
template <class Params> void drct_fold_adjust(const srad_drct* h, int blk, Params& p) {
  const char* const reg = h->pt.arena + h->derived.region(DRCT_BLOCK_FOLD, blk).off;
  p.w_adj = reg + h->mfold[blk].pack; p.b_adj = reinterpret_cast<const float*>(reg + h->mfold[blk].bias);
}

// parts (drct_engine.h): the whole forward, or its entry / interior / exit alone; only the entry reads x, only the exit writes y
int forward_body(srad_drct* h, const float* x, int B, int H, int W, float* y, const DrctWs& w, hipStream_t s, const DrctPaths& paths,
                 int parts = DRCT_ALL) {
  const srad_drct_config& c = h->cfg;
  const int prec = c.precision, T = B * H * W, E = c.embed_dim, D = E + 4 * c.gc;
  SRAD_TRY(drct_stem(h, x, B, H, W, w, w.dense0, s, parts));
  float *cur = w.dense0, *nxt = w.dense1;
  // an odd number of RDGs leaves the last residual stream in dense1
  if (!(parts & DRCT_INTERIOR)) return drct_tail(h, c.n_rdg % 2 ? nxt : cur, B, H, W, w, c.in_chans, y, s, paths, parts);
  for (int i = 0; i < c.n_rdg; ++i) {
    for (int k = 0; k < 5; ++k) {
      const SwinW& sw = h->blocks[i * 5 + k];
      const int d = sw.d, hdp = hdp_of(d, sw.heads);
      const DrctBlockPath bp = drct_block_path(h, sw, k, B, H, W, paths);
      // the attention output is handed to the fused second half as bf16 (what its MFMA rounds it to anyway: half the bytes);
      // split-bf16: as fp32, both fused kernels with their lo weight packs
      const bool x3 = prec == SRAD_PREC_BF16X3;
      __bf16* const attn_h = reinterpret_cast<__bf16*>(w.attn);
      const bool hand_h = bp.second != DRCT_H2_CHAIN && !x3;
      switch (bp.first) {
        case DRCT_H1_IN_BLOCK: {
          SwinBlockParams b = drct_swin_block_params(drct_qkv_attn_params(h, sw, cur, B, H, W), drct_mlp_block_params(h, sw, k, attn_h, cur, nxt, T));
          if (bp.second == DRCT_H2_IN_BLOCK_FOLDED) drct_fold_adjust(h, i * 5 + k, b);
          SRAD_TRY(bp.second == DRCT_H2_IN_BLOCK_FOLDED ? srad_launch_swin_block_folded(b, s) : srad_launch_swin_block(b, s));
          continue;
        }
        case DRCT_H1_QKV_ATTN: {
          // norm1 + qkv + shifted-window attention of one (window, head) per workgroup, one launch (drct.py:477-504, 278-299)
          QkvAttnParams a = drct_qkv_attn_params(h, sw, cur, B, H, W);
          a.out = w.attn; a.out_h = hand_h ? attn_h : nullptr;
          a.split = x3; a.w_qkv_lo = h->pt.frag_lo_ptr(sw.qkv.w);
          SRAD_TRY(srad_launch_qkv_attn(a, s));
          break;
        }
        // norm1 + qkv                                   (drct.py:477, 278)
        case DRCT_H1_LN_QKV:
        case DRCT_H1_LN_QKV_SPLIT: {
          // one launch, 64 rows per workgroup against the whole weight (kernels_fused_attn.hip ln_qkv_kernel); split-bf16: hi + lo
          // planes and packs, fp32 q | k | v out (the split attention kernel scales and splits them)
          const bool split = bp.first == DRCT_H1_LN_QKV_SPLIT;
          LnQkvParams q{};
          q.x = cur; q.ldx = D; q.M = T; q.d = d; q.heads = sw.heads; q.ln_g = h->pt.fptr(sw.n1g); q.ln_b = h->pt.fptr(sw.n1b);
          q.w_qkv = h->pt.frag_ptr(sw.qkv.w); q.w_qkv_lo = split ? h->pt.frag_lo_ptr(sw.qkv.w) : nullptr; q.b_qkv = h->pt.fptr(sw.qkv.b);
          if (split) q.qkv_f = w.qkv; else q.qkv_h = reinterpret_cast<__bf16*>(w.qkv);
          q.hdp = hdp; q.qscale = split ? 1.f : bp.qscale;
          SRAD_TRY(srad_launch_ln_qkv(q, s));
          break;
        }
        case DRCT_H1_GEMM: {
          GemmParams p = drct_gemm(h, sw.qkv, cur, D, T, w.qkv, 3 * sw.heads * hdp);
          p.hsplit_hd = d / sw.heads; p.hsplit_hdp = hdp;      // head-padded q|k|v rows for the attention kernel
          p.ln_g = h->pt.fptr(sw.n1g); p.ln_b = h->pt.fptr(sw.n1b);
          if (bp.qkv_bf16) { p.Yh = reinterpret_cast<__bf16*>(w.qkv); p.hsplit_heads = sw.heads; p.hsplit_qscale = bp.qscale; }
          SRAD_TRY(srad_launch_gemm(prec, p, s));
          break;
        }
      }
      // shifted-window attention                      (drct.py:481-504, 281-299)
      if (bp.first != DRCT_H1_QKV_ATTN) {
        AttnParams a{w.qkv, w.attn, h->pt.fptr(sw.table), B, H, W, c.window_size, sw.shift, d, sw.heads, hdp};
        if (hand_h) a.out_h = attn_h;
        if (bp.qkv_bf16) a.qkv_h = reinterpret_cast<const __bf16*>(w.qkv);
        SRAD_TRY(srad_launch_window_attn(prec, a, s));
      }
      if (bp.second != DRCT_H2_CHAIN) {
        // proj + shortcut -> norm2 -> fc1 -> GELU -> fc2 + residual -> adjust_k, one launch (drct.py:300, 509-510, 184-190, 389-396)
        MlpBlockParams q = drct_mlp_block_params(h, sw, k, attn_h, cur, nxt, T);
        if (bp.second == DRCT_H2_MLP_BLOCK_FOLDED) {
          drct_fold_adjust(h, i * 5 + k, q);
          SRAD_TRY(srad_launch_mlp_block_folded(q, s));
          continue;
        }
        q.split = x3; q.attn_f = w.attn;
        q.w_proj_lo = h->pt.frag_lo_ptr(sw.proj.w); q.w_fc1_lo = h->pt.frag_lo_ptr(sw.fc1.w); q.w_fc2_lo = h->pt.frag_lo_ptr(sw.fc2.w);
        q.w_adj_lo = h->pt.frag_lo_ptr(sw.adjust.w);
        SRAD_TRY(srad_launch_mlp_block(q, s));
        continue;
      }
      // proj + shortcut                               (drct.py:300, 509)
      GemmParams p1 = drct_gemm(h, sw.proj, w.attn, d, T, w.x1, d);
      p1.R = cur; p1.ldr = D;
      SRAD_TRY(srad_launch_gemm(prec, p1, s));
      // norm2 + fc1 + GELU                            (drct.py:510, 185-186)
      GemmParams p2 = drct_gemm(h, sw.fc1, w.x1, d, T, w.hid, sw.hidden);
      p2.ln_g = h->pt.fptr(sw.n2g); p2.ln_b = h->pt.fptr(sw.n2b); p2.act = SRAD_ACT_GELU;
      SRAD_TRY(srad_launch_gemm(prec, p2, s));
      // fc2 + residual                                (drct.py:188, 510)
      GemmParams p3 = drct_gemm(h, sw.fc2, w.hid, sw.hidden, T, w.x2, d);
      p3.R = w.x1; p3.ldr = d;
      SRAD_TRY(srad_launch_gemm(prec, p3, s));
      // adjust_k 1x1 conv (+ LeakyReLU 0.2) into the dense buffer (drct.py:389-392); adjust5: *0.2 + x into the next (drct.py:393, 396)
      GemmParams p4 = drct_gemm(h, sw.adjust, w.x2, d, T, k < 4 ? cur : nxt, D);
      if (k < 4) { p4.yoff = d; p4.act = SRAD_ACT_LRELU; p4.slope = 0.2f; }
      else { p4.alpha = 0.2f; p4.R = cur; p4.ldr = D; }
      SRAD_TRY(srad_launch_gemm(prec, p4, s));
    }
    float* t = cur; cur = nxt; nxt = t;
  }
  return drct_tail(h, cur, B, H, W, w, c.in_chans, y, s, paths, parts);
}

// Which inference-only forms this forward runs.  Inference handles only: one bound for training gets its weights through
// srad_drct_sync_params, which neither passes the folds' sources on nor refreshes the ends packs.  Overrides are read per call.
DrctPaths drct_paths(const srad_drct* h, int B, int H, int W) {
  const srad_drct_config& c = h->cfg;
  DrctPaths p;
  if (h->ts.tarena || h->ts.ready) return p;
  p.fold = h->derived.has(DRCT_TAIL_FOLD) && H >= 2 && W >= 2 && !srad_path_override(SRAD_PATH_TAIL_CHAIN);
  p.ends = h->ends_ok && srad_drct_ends_supported(c.precision, c.embed_dim, c.num_feat, c.in_chans, B, H, W) && !srad_path_override(SRAD_PATH_ENDS_CHAIN);
  p.mfold = h->derived.has(DRCT_BLOCK_FOLD) && !srad_path_override(SRAD_PATH_FC2_CHAIN);
  return p;
}

}  // namespace

// ---- shared with the training forward (drct_train.hip) ----
static void drct_mean(const srad_drct_config& c, float m[3]) {   // MeanShift: the RGB mean, none for gray images  (drct.py:887, 897)
  const float rgb[3] = {0.4488f, 0.4371f, 0.4040f};
  for (int i = 0; i < 3; ++i) m[i] = c.in_chans == 3 ? rgb[i] : 0.f;
}

int drct_stem(const srad_drct* h, const float* x, int B, int H, int W, const DrctStemTail& w, float* dense0, hipStream_t s,
              int parts) {
  const srad_drct_config& c = h->cfg;
  const int T = B * H * W, E = c.embed_dim, D = E + 4 * c.gc;
  float mean3[3]; drct_mean(c, mean3);
  // (x - mean) * img_range, NCHW -> NHWC            (drct.py:887-888)
  if (parts & DRCT_ENTRY) SRAD_TRY(srad_launch_nchw_to_nhwc(x, w.xin, B, c.in_chans, SRAD_IMG_CPAD, H, W, mean3, c.img_range, s));
  if (!(parts & DRCT_INTERIOR)) return SRAD_OK;
  // conv_first                                       (drct.py:892)
  GemmParams p = drct_gemm(h, h->conv_first, w.xin, SRAD_IMG_CPAD, T, w.feat0, E);
  p.Cin = SRAD_IMG_CPAD;                 // padded image channels; the packed weight is zero there
  geom(p, H, W);
  SRAD_TRY(srad_launch_gemm(c.precision, p, s));
  // patch_embed.norm -> residual stream in dense0[:, :E]   (drct.py:873, 650-654)
  return srad_launch_layernorm(w.feat0, E, dense0, D, T, E, h->pt.fptr(h->pe_g), h->pt.fptr(h->pe_b), 1e-5f, s);
}

int drct_tail(const srad_drct* h, const float* dense, int B, int H, int W, const DrctStemTail& w, int ld_outn, float* y,
              hipStream_t s, const DrctPaths& paths, int parts) {
  const srad_drct_config& c = h->cfg;
  const int prec = c.precision, T = B * H * W, E = c.embed_dim, D = E + 4 * c.gc, F = c.num_feat;
  const bool interior = (parts & DRCT_INTERIOR) != 0, last = (parts & DRCT_EXIT) != 0;
  if (interior && paths.ends) {      // (not interior: the launches ahead of the last one belong to another call)
    // norm, conv_after_body + x and conv_before_upsample + LeakyReLU(0.01) as one launch into c2 (kernels_drct_ends.hip)
    DrctBodyEndParams p{};
    p.X = dense; p.ldx = D; p.ln_g = h->pt.fptr(h->norm_g); p.ln_b = h->pt.fptr(h->norm_b);
    p.w1 = h->pt.ends_ptr(h->conv_after_body.w); p.b1 = h->pt.fptr(h->conv_after_body.b);
    p.w2 = h->pt.ends_ptr(h->conv_before_up.w); p.b2 = h->pt.fptr(h->conv_before_up.b);
    p.feat0 = w.feat0; p.Y = w.c2; p.B = B; p.H = H; p.W = W; p.E = E;
    SRAD_TRY(srad_launch_drct_body_end(p, s));
  } else if (interior) {
    // norm                                              (drct.py:881)
    SRAD_TRY(srad_launch_layernorm(dense, D, w.body, E, T, E, h->pt.fptr(h->norm_g), h->pt.fptr(h->norm_b), 1e-5f, s));
    // conv_after_body(...) + x                          (drct.py:893)
    GemmParams p1 = drct_gemm(h, h->conv_after_body, w.body, E, T, w.c1, E);
    geom(p1, H, W); p1.R = w.feat0; p1.ldr = E;
    SRAD_TRY(srad_launch_gemm(prec, p1, s));
    // conv_before_upsample + LeakyReLU(0.01)            (drct.py:844-845, 894)
    GemmParams p2 = drct_gemm(h, h->conv_before_up, w.c1, E, T, w.c2, F);
    geom(p2, H, W); p2.act = SRAD_ACT_LRELU; p2.slope = 0.01f;
    SRAD_TRY(srad_launch_gemm(prec, p2, s));
  }
  float mean3[3]; drct_mean(c, mean3);
  // Upsample, conv_last and x / img_range + mean as one 5 x 5 convolution of c2 (kernels_tail_fold.hip; drct.py:694-713, 895-897)
  if (paths.fold)
    return last ? srad_launch_tail_fold(h->fold, h->pt.arena + h->derived.region(DRCT_TAIL_FOLD, 0).off, w.c2, B, H, W, y, 1.0f / c.img_range, mean3, s) : SRAD_OK;
  // Upsample: conv 64->256 + PixelShuffle(2) per stage (drct.py:694-713)
  const float* src = w.c2;
  int hh = H, ww = W;
  for (size_t j = 0; j < h->up.size(); ++j) {
    if (interior) {
      GemmParams p = drct_gemm(h, h->up[j], src, F, B * hh * ww, w.upb[j], F);
      geom(p, hh, ww); p.ps = 2;
      SRAD_TRY(srad_launch_gemm(prec, p, s));
    }
    src = w.upb[j];
    hh *= 2; ww *= 2;
  }
  // conv_last                                         (drct.py:895)
  if (interior) {
    GemmParams p = drct_gemm(h, h->conv_last, src, F, B * hh * ww, w.outn, ld_outn);
    geom(p, hh, ww);
    SRAD_TRY(srad_launch_gemm(prec, p, s));
  }
  // x / img_range + mean, NHWC -> NCHW                (drct.py:897)
  return last ? srad_launch_nhwc_to_nchw(w.outn, ld_outn, y, B, c.in_chans, hh, ww, mean3, 1.0f / c.img_range, s) : SRAD_OK;
}

QkvAttnParams drct_qkv_attn_params(const srad_drct* h, const SwinW& sw, const float* cur, int B, int H, int W) {
  QkvAttnParams a{};
  a.x = cur; a.ldx = h->cfg.embed_dim + 4 * h->cfg.gc; a.ln_g = h->pt.fptr(sw.n1g); a.ln_b = h->pt.fptr(sw.n1b);
  a.w_qkv = h->pt.frag_ptr(sw.qkv.w); a.b_qkv = h->pt.fptr(sw.qkv.b); a.table = h->pt.fptr(sw.table);
  a.ld_out = sw.d; a.B = B; a.H = H; a.W = W; a.shift = sw.shift; a.d = sw.d; a.heads = sw.heads;
  return a;
}

MlpBlockParams drct_mlp_block_params(const srad_drct* h, const SwinW& sw, int k, const __bf16* attn_h, float* cur, float* nxt, int T) {
  const int D = h->cfg.embed_dim + 4 * h->cfg.gc;
  MlpBlockParams q{};
  q.attn_h = attn_h; q.ld_attn = sw.d; q.shortcut = cur; q.ld_short = D;
  q.M = T; q.d = sw.d; q.m = sw.hidden; q.no = k < 4 ? h->cfg.gc : h->cfg.embed_dim;
  q.w_proj = h->pt.frag_ptr(sw.proj.w); q.w_fc1 = h->pt.frag_ptr(sw.fc1.w); q.w_fc2 = h->pt.frag_ptr(sw.fc2.w);
  q.w_adj = h->pt.frag_ptr(sw.adjust.w);
  q.b_proj = h->pt.fptr(sw.proj.b); q.b_fc1 = h->pt.fptr(sw.fc1.b); q.b_fc2 = h->pt.fptr(sw.fc2.b); q.b_adj = h->pt.fptr(sw.adjust.b);
  q.ln_g = h->pt.fptr(sw.n2g); q.ln_b = h->pt.fptr(sw.n2b);
  // adjust_k (+ LeakyReLU 0.2) into the dense buffer; adjust5: * 0.2 + x into the next   (drct.py:389-396)
  if (k < 4) { q.act = SRAD_ACT_LRELU; q.slope = 0.2f; q.alpha = 1.f; q.Y = cur; q.ldy = D; q.yoff = sw.d; }
  else { q.act = SRAD_ACT_NONE; q.alpha = 0.2f; q.R = cur; q.ldr = D; q.Y = nxt; q.ldy = D; q.yoff = 0; }
  return q;
}

SwinBlockParams drct_swin_block_params(const QkvAttnParams& a, const MlpBlockParams& q) {
  SwinBlockParams b{};
  b.x = a.x; b.ldx = a.ldx; b.B = a.B; b.H = a.H; b.W = a.W; b.shift = a.shift; b.d = a.d; b.heads = a.heads; b.m = q.m; b.no = q.no;
  b.ln1_g = a.ln_g; b.ln1_b = a.ln_b; b.w_qkv = a.w_qkv; b.b_qkv = a.b_qkv; b.table = a.table;
  b.w_proj = q.w_proj; b.w_fc1 = q.w_fc1; b.w_fc2 = q.w_fc2; b.w_adj = q.w_adj;
  b.b_proj = q.b_proj; b.b_fc1 = q.b_fc1; b.b_fc2 = q.b_fc2; b.b_adj = q.b_adj; b.ln2_g = q.ln_g; b.ln2_b = q.ln_b;
  b.act = q.act; b.slope = q.slope; b.alpha = q.alpha; b.R = q.R; b.ldr = q.ldr; b.Y = q.Y; b.ldy = q.ldy; b.yoff = q.yoff;
  return b;
}

extern "C" {

int srad_version(void) { return 100; }

int srad_drct_create(const srad_drct_config* cfg, srad_drct_t** out) {
  SRAD_REQUIRE(cfg && out, "drct_create: null argument");
  SRAD_REQUIRE(cfg->in_chans == 1 || cfg->in_chans == 3, "drct_create: in_chans must be 1 or 3 (got %d)", cfg->in_chans);
  SRAD_REQUIRE(cfg->upscale >= 1 && (cfg->upscale & (cfg->upscale - 1)) == 0, "drct_create: upscale %d is not 2^n", cfg->upscale);
  SRAD_REQUIRE(cfg->window_size >= 1 && cfg->window_size <= 128, "drct_create: window_size %d out of range", cfg->window_size);
  SRAD_REQUIRE(cfg->embed_dim > 0 && cfg->embed_dim % 4 == 0 && cfg->gc % 4 == 0, "drct_create: embed_dim/gc must be multiples of 4");
  SRAD_REQUIRE(cfg->embed_dim % cfg->num_heads == 0, "drct_create: embed_dim %d not divisible by num_heads %d", cfg->embed_dim, cfg->num_heads);
  SRAD_REQUIRE(cfg->precision == SRAD_PREC_F32 || cfg->precision == SRAD_PREC_BF16 || cfg->precision == SRAD_PREC_BF16X3,
               "drct_create: bad precision %d", cfg->precision);
  srad_drct* h = new (std::nothrow) srad_drct();
  if (!h) return srad_set_error(SRAD_ERR_NOMEM, "drct_create: out of host memory");
  h->cfg = *cfg;
  h->pt.prec = cfg->precision;
  h->fuse_mlp = !srad_path_override(SRAD_PATH_UNFUSED_BLOCKS);
  const int E = cfg->embed_dim, C = cfg->in_chans, ws = cfg->window_size, F = cfg->num_feat;
  h->conv_first = h->pt.add_layer("conv_first", E, C, 9, true);
  h->pe_g = h->pt.add_raw("patch_embed.norm.weight", E);
  h->pe_b = h->pt.add_raw("patch_embed.norm.bias", E);
  h->dmax = 0; h->hmax = 0; h->qkvmax = 0;
  for (int i = 0; i < cfg->n_rdg; ++i) {
    for (int k = 0; k < 5; ++k) {
      SwinW sw;
      sw.d = E + k * cfg->gc;
      sw.heads = k == 0 ? cfg->num_heads : cfg->num_heads - (sw.d % cfg->num_heads);   // drct.py:337-367
      if (sw.heads <= 0 || sw.d % sw.heads != 0) {
        delete h;
        return srad_set_error(SRAD_ERR_ARG, "drct_create: block %d dim %d has no valid head count", k + 1, sw.d);
      }
      sw.hidden = (int)(sw.d * (k < 3 ? cfg->mlp_ratio : 1.0f));
      sw.shift = (k == 1 || k == 3) ? ws / 2 : 0;
      const std::string p = "layers." + std::to_string(i) + ".swin" + std::to_string(k + 1) + ".";
      sw.n1g = h->pt.add_raw(p + "norm1.weight", sw.d);
      sw.n1b = h->pt.add_raw(p + "norm1.bias", sw.d);
      sw.table = h->pt.add_raw(p + "attn.relative_position_bias_table", (int64_t)(2 * ws - 1) * (2 * ws - 1) * sw.heads);
      sw.qkv = h->pt.add_layer(p + "attn.qkv", 3 * sw.d, sw.d, 1, true);
      if (cfg->precision == SRAD_PREC_BF16) h->pt.entries[sw.qkv.w].tfrag = true;   // operand of the fused qkv + LayerNorm1 backward
      const bool frag = cfg->precision == SRAD_PREC_BF16 || cfg->precision == SRAD_PREC_BF16X3;   // operands of the fused block kernels
      if (frag && sw.d % sw.heads == 0) h->pt.add_qkv_frag(sw.qkv, sw.d, sw.heads);   // fused attention kernel
      sw.proj = frag ? h->pt.add_layer_frag(p + "attn.proj", sw.d, sw.d, true) : h->pt.add_layer(p + "attn.proj", sw.d, sw.d, 1, true);
      sw.n2g = h->pt.add_raw(p + "norm2.weight", sw.d);
      sw.n2b = h->pt.add_raw(p + "norm2.bias", sw.d);
      const std::string an = "layers." + std::to_string(i) + ".adjust" + std::to_string(k + 1);
      const int ao = k < 4 ? cfg->gc : E;
      sw.fc1 = frag ? h->pt.add_layer_frag(p + "mlp.fc1", sw.hidden, sw.d, true) : h->pt.add_layer(p + "mlp.fc1", sw.hidden, sw.d, 1, true);
      sw.fc2 = frag ? h->pt.add_layer_frag(p + "mlp.fc2", sw.d, sw.hidden, true) : h->pt.add_layer(p + "mlp.fc2", sw.d, sw.hidden, 1, true);
      sw.adjust = frag ? h->pt.add_layer_frag(an, ao, sw.d, true) : h->pt.add_layer(an, ao, sw.d, 1, true);
      if (sw.d > h->dmax) h->dmax = sw.d;
      if (3 * sw.heads * hdp_of(sw.d, sw.heads) > h->qkvmax) h->qkvmax = 3 * sw.heads * hdp_of(sw.d, sw.heads);
      if (sw.hidden > h->hmax) h->hmax = sw.hidden;
      h->blocks.push_back(sw);
    }
  }
  h->norm_g = h->pt.add_raw("norm.weight", E);
  h->norm_b = h->pt.add_raw("norm.bias", E);
  h->conv_after_body = h->pt.add_layer("conv_after_body", E, E, 9, true);
  h->conv_before_up = h->pt.add_layer("conv_before_upsample.0", F, E, 9, true);
  int stages = 0;
  for (int s = cfg->upscale; s > 1; s >>= 1) ++stages;
  for (int j = 0; j < stages; ++j) h->up.push_back(h->pt.add_layer("upsample." + std::to_string(2 * j), 4 * F, F, 9, true));
  h->conv_last = h->pt.add_layer("conv_last", C, F, 9, true);
  // the body end's two fragment packs (kernels_drct_ends.hip), refreshed by set_param like every other pack
  h->ends_ok = srad_drct_ends_supported_cus(cfg->precision, E, F, C, 1, 1, 1, 1) != 0;
  if (h->ends_ok) {
    h->pt.add_ends_pack(h->conv_after_body);
    h->pt.add_ends_pack(h->conv_before_up);
  }
  // the composed weights behind the table's packs (drct_derived.h): the folded output end where the model has one ...
  h->derived.end = h->pt.bytes;
  if (srad_tail_fold_supported(cfg->precision, F, C, cfg->upscale)) {
    h->fold = tf_layout(F, C, cfg->upscale);
    drct_derived_add_tail(h->derived, h->fold);
  }
  // ... then the blocks' folded second halves (any window size: the one-launch block keeps its own check, srad_swin_block_fold_supported)
  if (cfg->precision == SRAD_PREC_BF16 && h->fuse_mlp)
    for (int i = 0; i < cfg->n_rdg; ++i)
      for (int k = 0; k < 5; ++k) {
        const SwinW& sw = h->blocks[i * 5 + k];
        h->mfold.push_back(mf_layout(sw.d, sw.hidden, k < 4 ? cfg->gc : E));
        drct_derived_add_block(h->derived, i, k, h->mfold.back());
      }
  *out = h;
  return SRAD_OK;
}

void srad_drct_destroy(srad_drct_t* h) {
  if (!h) return;
  h->gc.reset();
  delete h;
}

int srad_drct_arena_bytes(const srad_drct_t* h, size_t* bytes) {
  SRAD_REQUIRE(h && bytes, "drct_arena_bytes: null argument");
  *bytes = h->derived.end;      // the parameter table's packs, then the regions of the composed weights
  return SRAD_OK;
}

int srad_drct_bind_arena(srad_drct_t* h, void* arena, size_t bytes) {
  SRAD_REQUIRE(h && arena, "drct_bind_arena: null argument");
  SRAD_REQUIRE(bytes >= h->derived.end, "drct_bind_arena: %zu bytes given, %zu needed", bytes, h->derived.end);
  SRAD_REQUIRE(((uintptr_t)arena & 255) == 0, "drct_bind_arena: arena must be 256-byte aligned");
  h->pt.arena = reinterpret_cast<char*>(arena);
  h->pt.arena_bytes = bytes;
  h->derived.mark_all();
  h->gc.reset();
  return SRAD_OK;
}

int srad_drct_num_params(const srad_drct_t* h) { return h ? (int)h->pt.entries.size() : 0; }

int srad_drct_param_info(const srad_drct_t* h, int idx, const char** name, int64_t* numel) {
  SRAD_REQUIRE(h && idx >= 0 && idx < (int)h->pt.entries.size(), "drct_param_info: index %d out of range", idx);
  if (name) *name = h->pt.entries[idx].name.c_str();
  if (numel) *numel = h->pt.entries[idx].numel;
  return SRAD_OK;
}

int srad_drct_set_param(srad_drct_t* h, const char* name, const float* dev_src, int64_t numel, void* stream) {
  SRAD_REQUIRE(h && name && dev_src, "drct_set_param: null argument");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  SRAD_TRY(h->pt.set(name, dev_src, numel, s));
  if (const DrctDerivedSource* src = h->derived.find(name)) {      // a source of a composed weight: keep its fp32 copy, rebuild before the next forward
    SRAD_CHECK_HIP(hipMemcpyAsync(h->pt.arena + h->derived.regions[src->region].off + src->off, dev_src, (size_t)numel * 4, hipMemcpyDeviceToDevice, s));
    h->derived.mark(src->region);
  }
  return SRAD_OK;
}

static int drct_check_shape(const srad_drct_t* h, int B, int H, int W) {
  SRAD_REQUIRE(B > 0 && H > 0 && W > 0, "drct: empty input %dx%dx%d", B, H, W);
  SRAD_REQUIRE(H % h->cfg.window_size == 0 && W % h->cfg.window_size == 0,
               "drct: input %dx%d is not a multiple of the window size %d", H, W, h->cfg.window_size);
  SRAD_REQUIRE((int64_t)B * H * W * h->cfg.upscale * h->cfg.upscale < (1LL << 31), "drct: problem too large for 32-bit pixel indices");
  return SRAD_OK;
}

int srad_drct_workspace_bytes(const srad_drct_t* h, int B, int H, int W, size_t* bytes) {
  SRAD_REQUIRE(h && bytes, "drct_workspace_bytes: null argument");
  SRAD_TRY(drct_check_shape(h, B, H, W));
  *bytes = plan_ws(h, B, H, W, nullptr, 0).bytes;
  return SRAD_OK;
}

int srad_drct_forward(srad_drct_t* h, const float* x, int B, int H, int W, float* y, void* workspace,
                      size_t workspace_bytes, void* stream) {
  SRAD_REQUIRE(h && x && y && workspace, "drct_forward: null argument");
  if (!h->pt.arena) return srad_set_error(SRAD_ERR_STATE, "drct_forward: no weight arena bound");
  SRAD_TRY(drct_check_shape(h, B, H, W));
  SRAD_REQUIRE(((uintptr_t)workspace & 255) == 0, "drct_forward: workspace must be 256-byte aligned");
  const DrctWs w = plan_ws(h, B, H, W, workspace, workspace_bytes);
  SRAD_REQUIRE(w.bytes <= workspace_bytes, "drct_forward: workspace %zu bytes, %zu needed", workspace_bytes, w.bytes);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // the forms this call runs: decided per call; a recorded graph holds one form of each
  const DrctPaths paths = drct_paths(h, B, H, W);
  if (paths != h->graph_paths) { h->gc.reset(); h->graph_paths = paths; }
  // their stale folds are rebuilt here - on the stream, ahead of the forward, never inside a capture or as a node of the graph
  const unsigned kinds = (paths.fold ? 1u << DRCT_TAIL_FOLD : 0) | (paths.mfold ? 1u << DRCT_BLOCK_FOLD : 0);
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (s && h->derived.stale(kinds)) SRAD_CHECK_HIP(hipStreamIsCapturing(s, &st));
  const int built = h->derived.refresh(kinds, st != hipStreamCaptureStatusNone, [&](const DrctDerivedRegion& r) {
    return r.kind == DRCT_TAIL_FOLD ? srad_launch_tail_fold_build(h->fold, h->pt.arena + r.off, s)
                                    : srad_launch_mlp_fold_build(h->mfold[r.index], h->pt.arena + r.off, s);
  });
  if (built == DRCT_DERIVED_CAPTURING)
    return srad_set_error(SRAD_ERR_STATE, "drct_forward: %s is stale and the stream is capturing: run one forward outside the capture first",
                          h->derived.stale(paths.fold ? 1u << DRCT_TAIL_FOLD : 0) ? "the folded output end" : "a folded block weight");
  SRAD_TRY(built);
  // Graph replay: only the interior is recorded, keyed on the workspace and the shape; the entry and the exit launch on the stream
  // either side of it.  (The legacy default stream cannot be captured: there, and with the graph off, it is one eager sequence.)
  if (!h->cfg.use_graph || s == nullptr) return forward_body(h, x, B, H, W, y, w, s, paths);
  SRAD_TRY(forward_body(h, x, B, H, W, y, w, s, paths, DRCT_ENTRY));
  SRAD_TRY(srad_run_with_graph(h->gc, true, workspace, B, H, W, s,
                               [&](hipStream_t cs) { return forward_body(h, nullptr, B, H, W, nullptr, w, cs, paths, DRCT_INTERIOR); }));
  return forward_body(h, x, B, H, W, y, w, s, paths, DRCT_EXIT);
}

int srad_drct_graph_captures(const srad_drct_t* h) { return h ? h->gc.captures : 0; }

int srad_drct_flops(const srad_drct_t* h, int B, int H, int W, double* flops) {
  SRAD_REQUIRE(h && flops, "drct_flops: null argument");
  const srad_drct_config& c = h->cfg;
  const double T = (double)B * H * W;
  const double N = (double)c.window_size * c.window_size;
  double f = 0;
  auto conv = [&](const ConvW& l, double pix) { f += 2.0 * pix * l.n * l.cin * l.ntaps; };
  conv(h->conv_first, T);
  for (const SwinW& sw : h->blocks) {
    conv(sw.qkv, T); conv(sw.proj, T); conv(sw.fc1, T); conv(sw.fc2, T); conv(sw.adjust, T);
    f += 2.0 * 2.0 * T * N * sw.d;      // q k^T and p v
  }
  conv(h->conv_after_body, T); conv(h->conv_before_up, T);
  double pix = T;
  for (const ConvW& u : h->up) { conv(u, pix); pix *= 4; }
  conv(h->conv_last, pix);
  *flops = f;
  return SRAD_OK;
}

}  // extern "C"
