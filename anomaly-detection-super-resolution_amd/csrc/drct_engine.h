// drct_engine.h - the DRCT handle shared by the inference engine (drct.hip) and the training engine
// (drct_train.hip), and the pieces of the forward both run: stem, tail, fused-block parameters (defined in drct.hip).
#pragma once
#include "train_common.h"
#include "drct_derived.h"
#include "../../include/srad.h"
#include <string>

struct SwinW {
  int d, heads, hidden, shift;
  int n1g, n1b, n2g, n2b, table;
  ConvW qkv, proj, fc1, fc2, adjust;
};

static inline int hdp_of(int d, int heads) { return srad_round_up(d / heads, 4); }

// Which of the inference-only forms one forward runs: fold = all after conv_before_upsample as the one folded launch, ends = norm,
// conv_after_body and conv_before_upsample as the one body-end launch, mfold = fc2 folded into the adjust conv in the blocks whose
// launch has that form.  Decided per call (drct_paths) and passed as an argument, never read back out of the handle.
struct DrctPaths {
  bool fold = false, ends = false, mfold = false;
  bool operator!=(const DrctPaths& o) const { return fold != o.fold || ends != o.ends || mfold != o.mfold; }
};

struct srad_drct {
  srad_drct_config cfg;
  ParamTable pt;
  ConvW conv_first, conv_after_body, conv_before_up, conv_last;
  std::vector<ConvW> up;
  int pe_g, pe_b, norm_g, norm_b;
  std::vector<SwinW> blocks;      // n_rdg * 5
  int dmax, hmax, qkvmax;         // widest block dim / hidden / head-padded qkv row
  std::vector<char> saved_h;      // per Swin block, what the last training forward saved as bf16: 1 q | k | v, 2 the fc1 pre-activation (plan_block)
  bool fuse_mlp = true;           // bf16: second half of each Swin block as one launch (kernels_fused.hip)
  // The composed weights (drct_derived.h): the folded output end (kernels_tail_fold.hip) and the Swin blocks' folded second halves
  // (mlp_fold.h), where the model has them.  srad_drct_set_param copies a changed fp32 source in and marks its region;
  // srad_drct_forward rebuilds the stale regions of the forms the call runs before it runs or replays anything.
  DrctDerived derived;
  TailFoldLayout fold{};
  std::vector<MlpFoldLayout> mfold;           // per block: where in its region the launches find the pack and the bias
  bool ends_ok = false;           // the model's shape has the body-end launch (kernels_drct_ends.hip; its packs are table entries' ends packs)
  GraphCache gc;
  DrctPaths graph_paths;          // what gc's graph was recorded with: a recorded graph holds one form of each
  TrainState ts;                  // training (drct_train.hip)
  BwdStreams bwd;                 // the backward's side stream for the weight gradients, and its events
};

// GemmParams of a Linear / 1x1 / 3x3 layer of the forward over M token rows (3x3: geom() adds the image geometry)
static inline GemmParams drct_gemm(const srad_drct* h, const ConvW& c, const float* X, int ldx, int M, float* Y, int ldy) {
  GemmParams p{};
  p.X = X; p.ldx = ldx; p.M = M; p.Cin = c.cin; p.Cp = srad_cp(c.cin); p.ntaps = c.ntaps;
  p.stride = 1; p.ln_eps = 1e-5f;
  p.Wp = h->pt.ptr(c.w); p.N = c.n; p.bias = h->pt.fptr(c.b);
  p.alpha = 1.f; p.Y = Y; p.ldy = ldy;
  return p;
}
static inline void geom(GemmParams& p, int H, int W) { p.Hi = p.Ho = H; p.Wi = p.Wo = W; }

// The stem's and the tail's tensors, in the workspace of either forward
struct DrctStemTail {
  float *xin, *feat0, *body, *c1, *c2, *outn;
  std::vector<float*> upb;
};
// The forward's launches in three parts: the entry is the one launch that reads x, the exit the one launch that writes y,
// the interior everything between them, which touches the workspace and the weight arena only.  The inference forward
// records just the interior into its graph (drct.hip), so the graph does not depend on the call's x and y.
enum : int { DRCT_ENTRY = 1, DRCT_INTERIOR = 2, DRCT_EXIT = 4, DRCT_ALL = 7 };
// (x - mean) * img_range -> conv_first -> patch_embed.norm into dense0[:, :embed]            (drct.py:887-892, 873)
// parts: DRCT_ENTRY the layout launch off x, DRCT_INTERIOR the rest
int drct_stem(const srad_drct* h, const float* x, int B, int H, int W, const DrctStemTail& w, float* dense0, hipStream_t s,
              int parts = DRCT_ALL);
// norm -> conv_after_body + x -> conv_before_upsample -> Upsample -> conv_last (into outn, row stride ld_outn) -> y   (drct.py:881, 893-897)
// paths: fold and ends as decided for this call (the fold is fresh); parts: DRCT_EXIT the last launch, DRCT_INTERIOR all before it
int drct_tail(const srad_drct* h, const float* dense, int B, int H, int W, const DrctStemTail& w, int ld_outn, float* y,
              hipStream_t s, const DrctPaths& paths = DrctPaths(), int parts = DRCT_ALL);
// The fields both forwards set for Swin block `sw` of an RDG, block k of its five: weights, biases, LayerNorm, geometry, and
// (mlp_block) the adjust conv's residual and output in the dense buffers cur / nxt; the one-launch block takes the two together
QkvAttnParams drct_qkv_attn_params(const srad_drct* h, const SwinW& sw, const float* cur, int B, int H, int W);
MlpBlockParams drct_mlp_block_params(const srad_drct* h, const SwinW& sw, int k, const __bf16* attn_h, float* cur, float* nxt, int T);
SwinBlockParams drct_swin_block_params(const QkvAttnParams& a, const MlpBlockParams& q);
