// drct_train_plan.h - what one Swin block of the DRCT training step takes.  Host-only: no HIP include
// (tests/host/drct_train_plan_check.cpp; __bf16 is the compiler's storage type).  drct_train.hip asks the library's predicates
// once per block and call (block_caps), decides here (plan_block), and launches what the plan says on the buffers in the form
// block_grads gives them.  The training forward and the backward ask with the same inputs and get the same answer; the forward
// records block_saved_form and the backward refuses another.
//
//   flag       set when                                                       then
//   xh         fused forward built, qkv_attn and mlp_block have the shape     LN1(x), attention output, LN2(.), GELU(.), x2 saved as bf16
//   (every fuse_* needs bf16, window 8, no unfused_blocks override, and the transposed fragment pack of each layer it folds)
//   fuse_mlp   fc1, fc2 packs, mlp_bwd at KA = 0                              fc2 / fc1 data gradients + LayerNorm2 backward: one launch
//   fuse_proj  fuse_mlp, proj pack                                            ... with the projection's data gradient behind them (dO)
//   fuse_adj   fuse_mlp, adjust pack, mlp_bwd at the block's KA               ... and the adjust conv's in front (dx2 made in the launch)
//   fuse_qkv   qkv pack, lin_ln_bwd                                           qkv data gradient + LayerNorm1 backward: one launch
//   yh_qkv     xh, fuse_qkv                                                   dqkv as bf16 for both of its readers
//   attn_h     xh, fuse_proj, yh_qkv, bf16-out rows, head dim <= 128          q | k | v SAVED as bf16, dO as bf16 per head
//   yh_dh      xh, fuse_mlp, bf16-out rows                                    dh as bf16, the fc1 pre-activation SAVED as bf16
//   yh_dx2     yh_dh, fuse_adj                                                dx2 * rs2 and dA as bf16, adjust5's dA copy behind dh
//   yh_dx1     yh_dx2, fuse_proj                                              dx1 * rs1 as bf16 behind dx2
#pragma once
#include <stddef.h>

struct BlockCaps {               // the answers plan_block needs, as plain values
  bool bf16, window8;            // precision is bf16; the window is 8 x 8
  bool unfused_override;         // the unfused_blocks path override is on for this call
  bool fused_forward;            // the handle was built with the fused block kernels (srad_drct::fuse_mlp)
  bool qkv_attn, mlp_block;      // srad_qkv_attn_supported, srad_mlp_block_supported at the block's KA
  bool mlp_bwd0, mlp_bwd_ka;     // srad_mlp_bwd_supported at KA = 0 and at the block's KA
  bool lin_ln_bwd, bf16_out;     // srad_lin_ln_bwd_supported, srad_mlp_bwd_bf16_out
  bool tf_qkv, tf_proj, tf_fc1, tf_fc2, tf_adjust;   // the layer has a transposed fragment pack (tf_off >= 0)
  int hd;                        // head dimension
};

struct BlockPlan { bool xh, fuse_mlp, fuse_proj, fuse_adj, fuse_qkv, attn_h, yh_dh, yh_dx2, yh_qkv, yh_dx1; };

inline BlockPlan plan_block(const BlockCaps& c) {
  // (windows other than 8 x 8 - the 32 / 64 / 256 px presets of src/main.py:218-219,286 - take the unfused forward, so they take
  // the unfused backward with it: fp32 saves, the general attention backward kernel)
  const bool fused_bwd = c.bf16 && c.window8 && !c.unfused_override;
  BlockPlan b{};
  b.xh = c.fused_forward && c.qkv_attn && c.mlp_block;
  b.fuse_mlp = fused_bwd && c.tf_fc1 && c.tf_fc2 && c.mlp_bwd0;
  b.fuse_proj = b.fuse_mlp && c.tf_proj;
  b.fuse_adj = b.fuse_mlp && c.tf_adjust && c.mlp_bwd_ka;
  b.fuse_qkv = fused_bwd && c.tf_qkv && c.lin_ln_bwd;
  b.yh_qkv = b.xh && b.fuse_qkv;
  b.attn_h = b.xh && b.fuse_proj && b.yh_qkv && c.bf16_out && c.hd <= 128 && c.window8;
  b.yh_dh = b.xh && b.fuse_mlp && c.bf16_out;
  b.yh_dx2 = b.yh_dh && b.fuse_adj;
  b.yh_dx1 = b.yh_dx2 && b.fuse_proj;
  return b;
}

// What the forward saved as bf16 for the backward kernels of this plan, beyond what xh always saves that way (srad_drct::saved_h)
enum { DRCT_SAVED_QKV_H = 1, DRCT_SAVED_HPRE_H = 2 };
inline int block_saved_form(const BlockPlan& b) { return b.xh ? (b.attn_h ? DRCT_SAVED_QKV_H : 0) | (b.yh_dh ? DRCT_SAVED_HPRE_H : 0) : 0; }

// The backward's per-block temporaries: two sets, alternating per block (the side stream's weight gradients read them), dO shared;
// and the two buffers of the forward's saves whose form follows the plan.
struct BlockGradBufs { float *dx2, *dx1, *dA, *dh, *dqkv, *dO, *qkv, *hpre; };
struct BlockGradFloats { size_t dx, dA, dh, dqkv; };      // floats the planner gives dx2 / dx1 / dO each, dA, dh, dqkv
inline BlockGradFloats block_grad_floats(size_t T, int E, int dmax, int hmax) { return {T * dmax, T * E, T * hmax, T * 3 * dmax}; }

// One gradient in the form the plan gives it.  f: its address as the launches that take "const float* + a bf16 flag" want it
// (weight gradients, lin_ln_bwd) and as the fp32 writers want it; h: the same address typed, set iff the tensor is bf16; ld in
// elements of that form.  Null f: the plan has no such tensor.
struct Grad { float* f; __bf16* h; int ld; int is_h() const { return h != nullptr; } };
struct BlockGrads {
  Grad dx2;      // fp32, or dx2 * rs2 as bf16 (yh_dx2) at the front of its buffer
  Grad dx1;      // fp32 always
  Grad dx1s;     // yh_dx1: dx1 * rs1 as bf16, BEHIND the bf16 dx2 in the dx2 buffer
  Grad dh;       // fp32, or bf16 (yh_dh) at the front of its buffer
  Grad dA5;      // yh_dx2: the bf16 copy of adjust5's incoming gradient, BEHIND the bf16 dh in the dh buffer
  Grad dA;       // adjust1-4's incoming gradient after LeakyReLU': fp32, or bf16 (yh_dx2)
  Grad dqkv;     // fp32, or bf16 (yh_qkv)
  Grad dO;       // fp32 [T][d], or bf16 per head [T][heads][hp] (attn_h): ld = d either way, the launches take heads and hp
  Grad qkv;      // SAVED q | k | v: fp32 [T][3][heads][hdp], or bf16 [T][3][heads][hp] (attn_h); ld = 0, the launches take the row
  Grad hpre;     // SAVED fc1 pre-activation: fp32, or bf16 (yh_dh)
};
// The capacity rule of the two "behind" placements: the bf16 dh plus the dA5 copy fit the dh buffer, the bf16 dx2 plus dx1 * rs1
// the dx2 buffer (2 bytes an element against 4 a float).  With block_grad_floats the second always holds (d <= dmax); the
// first asks KA <= 2 hmax - hidden of the model.
inline bool block_grads_fit(const BlockPlan& b, const BlockGradFloats& cap, size_t T, int d, int hidden, int KA) {
  return (!b.yh_dx2 || T * (size_t)(hidden + KA) <= 2 * cap.dh) && (!b.yh_dx1 || T * (size_t)(2 * d) <= 2 * cap.dx);
}
inline BlockGrads block_grads(const BlockPlan& b, const BlockGradBufs& w, size_t T, int d, int hidden, int KA) {
  auto front = [](float* buf, bool bf16, int ld) { return Grad{buf, bf16 ? reinterpret_cast<__bf16*>(buf) : nullptr, ld}; };
  auto behind = [&](float* buf, size_t elems_in_front, int ld) {
    return front(reinterpret_cast<float*>(reinterpret_cast<__bf16*>(buf) + elems_in_front), true, ld); };
  BlockGrads g{};
  g.dx2 = front(w.dx2, b.yh_dx2, d);
  g.dx1 = front(w.dx1, false, d);
  if (b.yh_dx1) g.dx1s = behind(w.dx2, T * d, d);
  g.dh = front(w.dh, b.yh_dh, hidden);
  if (b.yh_dx2) g.dA5 = behind(w.dh, T * hidden, KA);
  g.dA = front(w.dA, b.yh_dx2, KA);
  g.dqkv = front(w.dqkv, b.yh_qkv, 3 * d);
  g.dO = front(w.dO, b.attn_h, d);
  g.qkv = front(w.qkv, b.attn_h, 0);
  g.hpre = front(w.hpre, b.yh_dh, hidden);
  return g;
}
