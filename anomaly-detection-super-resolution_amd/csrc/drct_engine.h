// drct_engine.h - the DRCT handle shared by the inference engine (drct.hip) and the training engine
// (drct_train.hip), and the pieces of the forward both run: stem, tail, fused-block parameters (defined in drct.hip).
#pragma once
#include "train_common.h"
#include "tail_fold.h"
#include "mlp_fold.h"
#include "../../include/srad.h"
#include <string>
#include <unordered_map>
#include <utility>

struct SwinW {
  int d, heads, hidden, shift;
  int n1g, n1b, n2g, n2b, table;
  ConvW qkv, proj, fc1, fc2, adjust;
};

static inline int hdp_of(int d, int heads) { return srad_round_up(d / heads, 4); }

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
  // The folded output end (kernels_tail_fold.hip): its region follows the parameter table's in the weight arena and is no
  // entry of the table.  srad_drct_set_param copies the fp32 sources in and marks the fold stale; srad_drct_forward rebuilds a
  // stale fold before it runs or replays anything.  A handle bound for training keeps the chain of launches.
  bool fold_ok = false, fold_stale = true, fold_in_graph = false;
  TailFoldLayout fold{};
  size_t fold_off = 0;
  // The body-end launch (kernels_drct_ends.hip): ends_ok = the model's shape has it (its packs are entries' ends packs in the
  // table); which forwards take it is decided per call, and a recorded graph holds one of the two forms.
  bool ends_ok = false, ends_in_graph = false;
  // The folded second halves of the Swin blocks (mlp_fold.h): one region per block behind the folded output
  // end's, same rules - set_param copies a block's four fp32 sources in and marks it stale, srad_drct_forward rebuilds stale
  // blocks before it runs or replays anything, a handle bound for training keeps the chain.  The handle keeps both packs.
  bool mfold_ok = false, mfold_stale = true, mfold_in_graph = false;
  std::vector<MlpFoldLayout> mfold;           // per block
  std::vector<size_t> mfold_off;              // per block: byte offset of its region in the arena
  std::vector<char> mfold_dirty;              // per block: a source changed since its last build
  std::unordered_map<std::string, std::pair<int, size_t>> mfold_src;   // parameter name -> (block, byte offset in its region)
  size_t mfold_end = 0;                       // end of the last region
  GraphCache gc;
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
// fold: everything after conv_before_upsample as the one folded launch (the caller has checked drct_fold_active and freshness)
// ends: norm, conv_after_body and conv_before_upsample as the one body-end launch (the caller has checked drct_ends_active)
// parts: DRCT_EXIT the last launch (the folded launch, or the chain's layout launch into y), DRCT_INTERIOR all before it
int drct_tail(const srad_drct* h, const float* dense, int B, int H, int W, const DrctStemTail& w, int ld_outn, float* y,
              hipStream_t s, bool fold = false, bool ends = false, int parts = DRCT_ALL);
// The fields both forwards set for Swin block `sw` of an RDG, block k of its five: weights, biases, LayerNorm, geometry, and
// (mlp_block) the adjust conv's residual and output in the dense buffers cur / nxt
QkvAttnParams drct_qkv_attn_params(const srad_drct* h, const SwinW& sw, const float* cur, int B, int H, int W);
MlpBlockParams drct_mlp_block_params(const srad_drct* h, const SwinW& sw, int k, const __bf16* attn_h, float* cur, float* nxt, int T);
