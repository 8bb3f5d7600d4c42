/* srad.h - C ABI of libsrad, the MI355X (gfx950) engine for the SR forward / scorer hot path of
 * Benedict3007/anomaly-detection-super-resolution.
 *
 * The reference has no FFI layer; its seam for this path is Python (`make_model(opt)` /
 * `Model.forward`, reference src/model.py:46-52,95-100; `ssim_numpy`/`psnr_numpy`,
 * src/metrics.py:15-67; `roc_auc_score` call sites src/evaluate.py:245,263-265).  Each entry
 * point below names the reference interface it stands in for.  INTEGRATION.md shows the
 * ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure; `srad_last_error()` gives the
 *     thread-local message.  Nothing aborts.
 *   - all pointers named `dev_*`, `x`, `y`, `workspace`, `arena` are DEVICE pointers owned by the
 *     caller (e.g. PyTorch's caching allocator).  The library allocates no device memory.
 *   - `stream` is a `hipStream_t` passed as `void*`; all work is enqueued on it asynchronously.
 *     Functions that return host scalars say so and synchronise that stream.
 *   - a handle is not thread-safe: one per process / rank.
 *   - images are fp32 NCHW in [0, rgb_range], exactly what the reference modules take/return.
 */
#ifndef SRAD_H
#define SRAD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRAD_PRECISION_F32 0  /* v_mfma_f32_16x16x4_f32: exact fp32, the parity mode            */
#define SRAD_PRECISION_BF16 1 /* v_mfma_f32_16x16x32_bf16, fp32 accumulate, fp32 residual stream */
#define SRAD_PRECISION_BF16X3 2 /* split-bf16: every MFMA operand as hi + lo bf16 terms, three bf16 MFMAs per product
                                 * (hi.hi + hi.lo + lo.hi), fp32 accumulate - fp32-grade outputs (the 1e-3 / AUC +-0.002 bar)
                                 * from the bf16 matrix pipe.  Inference only (forward / scoring); training is fp32 or bf16. */

const char* srad_last_error(void);
int srad_version(void);

/* ------------------------------------------------------------------ DRCT-L (src/drct.py:716-898) */
typedef struct srad_drct srad_drct_t;
typedef struct {
  int32_t in_chans;    /* opt.n_colors                          */
  int32_t img_size;    /* opt.img_size (LR side built for)      */
  int32_t window_size; /* opt.window_size = img_size // 4       */
  int32_t upscale;     /* opt.upscale (2^n)                     */
  int32_t embed_dim;   /* 180                                   */
  int32_t n_rdg;       /* len(opt.depths) = 12                  */
  int32_t num_heads;   /* 6                                     */
  int32_t gc;          /* 32                                    */
  int32_t num_feat;    /* 64                                    */
  float mlp_ratio;     /* 2                                     */
  float img_range;     /* 1.0                                   */
  int32_t precision;   /* SRAD_PRECISION_*                      */
  int32_t use_graph;   /* replay the forward from a hipGraph when shapes/pointers repeat */
} srad_drct_config;

/* DRCT.__init__ (src/drct.py:718-849) */
int srad_drct_create(const srad_drct_config* cfg, srad_drct_t** out);
void srad_drct_destroy(srad_drct_t* h);
/* packed-weight arena the caller must provide before loading parameters */
int srad_drct_arena_bytes(const srad_drct_t* h, size_t* bytes);
int srad_drct_bind_arena(srad_drct_t* h, void* arena, size_t bytes);
/* state_dict surface: fp32 tensors in the reference's key names (src/model.py:114-116,155-170) */
int srad_drct_num_params(const srad_drct_t* h);
int srad_drct_param_info(const srad_drct_t* h, int idx, const char** name, int64_t* numel);
int srad_drct_set_param(srad_drct_t* h, const char* name, const float* dev_src, int64_t numel, void* stream);
int srad_drct_workspace_bytes(const srad_drct_t* h, int B, int H, int W, size_t* bytes);
/* DRCT.forward (src/drct.py:886-898): x [B,C,H,W] -> y [B,C,H*s,W*s]; H, W multiples of the window */
int srad_drct_forward(srad_drct_t* h, const float* x, int B, int H, int W, float* y, void* workspace,
                      size_t workspace_bytes, void* stream);
/* read-only: hipGraphs this handle has instantiated so far (use_graph: one per workspace and shape, whatever x and y are) */
int srad_drct_graph_captures(const srad_drct_t* h);
/* FLOPs (2 per MAC) of one forward at this shape, for roofline accounting */
int srad_drct_flops(const srad_drct_t* h, int B, int H, int W, double* flops);

/* ------------------------------------------------------------------ DRCT training step (src/trainer.py:152-222)
 * loss.backward() and optimizer.step() for the DRCT model.  Parameters and gradients live in two flat fp32
 * device buffers owned by the caller (PyTorch parameters / .grad are views into them): entry idx of
 * srad_drct_param_info starts at srad_drct_train_param_offset(idx) floats, total srad_drct_train_param_floats. */
int srad_drct_train_param_floats(srad_drct_t* h, int64_t* total);
int srad_drct_train_param_offset(srad_drct_t* h, int idx, int64_t* off_floats);
/* second caller-owned arena: transposed weight packs for the data gradients (bind after srad_drct_bind_arena) */
int srad_drct_train_arena_bytes(srad_drct_t* h, size_t* bytes);
int srad_drct_train_bind(srad_drct_t* h, void* train_arena, size_t bytes);
/* Split-K workspace the backward may use out of what the training arena holds (the default: all of it), in bytes, a multiple
 * of 512; each Swin block works in one half of it.  Less only costs extra reduce launches until a single reservation no longer
 * fits, which srad_drct_backward reports as an error.  For tests of those launches; outputs do not depend on it. */
int srad_drct_train_set_wgrad_budget(srad_drct_t* h, size_t bytes);
/* Reduce launches of the last srad_drct_backward by reason (SRAD_WQ_FLUSH_*, host bookkeeping), and the most floats a Swin
 * block had reserved in its half at once */
int srad_drct_train_wgrad_stats(const srad_drct_t* h, int launches[3], size_t* block_peak_floats);
/* refresh all packed weights from the flat fp32 parameters: call after loading and after every optimizer step */
int srad_drct_sync_params(srad_drct_t* h, const float* dev_flat_params, void* stream);
int srad_drct_train_workspace_bytes(const srad_drct_t* h, int B, int H, int W, size_t* bytes);
/* model.train() forward (src/drct.py:886-898 with DropPath 107-133 active): keep_scale is a device array
 * [2 * n_rdg * 5][B] of per-sample factors floor(keep + U) / keep (rows 2j / 2j+1: attention / MLP branch of
 * block j), or NULL for no DropPath.  Leaves the saved activations in `workspace` for srad_drct_backward. */
int srad_drct_forward_train(srad_drct_t* h, const float* x, int B, int H, int W, float* y, const float* keep_scale,
                            void* workspace, size_t workspace_bytes, void* stream);
/* loss.backward() (src/trainer.py:198): dy = dLoss/dy [B,C,H*s,W*s]; parameter gradients are ACCUMULATED into
 * dev_flat_grad; dx (optional) receives dLoss/dx.  on_bucket (optional) is called on the host as soon as the
 * last kernel writing gradient bucket b has been enqueued (buckets: srad_drct_bucket_range, in completion
 * order) so a data-parallel caller can start that bucket's all-reduce while the backward continues. */
typedef void (*srad_bucket_fn)(void* user, int bucket);
int srad_drct_num_buckets(const srad_drct_t* h);
int srad_drct_bucket_range(srad_drct_t* h, int bucket, int64_t* off_floats, int64_t* n_floats);
int srad_drct_backward(srad_drct_t* h, const float* dy, int B, int H, int W, const float* keep_scale, float* dx,
                       float* dev_flat_grad, void* workspace, size_t workspace_bytes, void* stream,
                       srad_bucket_fn on_bucket, void* user);
/* gradient seed of nn.L1Loss(reduction='mean') (src/loss.py:84): out = scale * sign(a - b), scale = 1/numel */
int srad_l1_grad(const float* a, const float* b, float* out, int64_t n, float scale, void* stream);
/* torch.optim.Adam.step on flat buffers (src/trainer.py:49-59; L2 weight decay, amsgrad off); step counts from 1;
 * grad_scale multiplies the gradient first (1/world_size after a summing all-reduce) */
int srad_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                   float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale, void* stream);
/* the same step with the per-step scalars in device memory: dev_hyper = [lr, 1 - beta1^step, sqrt(1 - beta2^step),
 * grad_scale] (4 floats), so a hipGraph capturing a whole training step can be replayed for every step */
int srad_adam_step_dev(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float beta1,
                       float beta2, float eps, float weight_decay, const float* dev_hyper, void* stream);
/* Both steps with the exponential moving average of the weights kept by the same launch (BasicSR's model_ema: no warm-up, no
 * bias correction).  params, exp_avg and exp_avg_sq end with the bits of the plain step; then, with p' the fp32 parameter
 * just stored and omd = (float)(1.0 - (double)ema_decay), ema[i] = fl(fl(ema_decay * ema[i]) + fl(omd * p')): three separately
 * rounded IEEE fp32 operations, no fused multiply-add.  Refused before anything is launched: a null ema, ema_decay outside
 * [0, 1) or NaN, ema overlapping any of the four other buffers, and what the plain steps refuse. */
int srad_adam_ema_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n, float lr,
                       float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale, float ema_decay,
                       void* stream);
int srad_adam_ema_step_dev(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                           float beta1, float beta2, float eps, float weight_decay, float ema_decay, const float* dev_hyper,
                           void* stream);
/* Guarded step: global-norm gradient clipping and a skip of every step whose gradients hold an inf or a NaN, decided on
 * the device so that the step stays free of host reads and replays inside a hipGraph.  One device workspace per optimizer,
 * 16-byte aligned, laid out as
 *     bytes  0..31  state : int64 applied, int64 skipped, int64 clipped, double last_norm   (zero it once; it lives on)
 *     bytes 32..63  record: float[4] = [lr, 1 - beta1^t, sqrt(1 - beta2^t), grad_scale * coef], int32 apply, 12 bytes unused
 *     bytes 64..    one fp64 partial sum per slot
 * srad_grad_guard_workspace: *slots = the slots the pass over n floats writes (a function of n alone), *bytes = 64 + 8 *slots
 * (either may be NULL; several tensors under one norm need 64 + 8 * the sum of their slots).
 * srad_grad_guard_partials: slot first_slot + k = workgroup k's share of sum grads[i]^2, every square and sum in fp64 (exact
 * squares, no overflow), fixed order, no atomics, no pre-zeroed buffer; grads needs float alignment only.
 * srad_grad_guard_finalize: sums the slots 0 .. n_slots - 1 in a fixed order; norm = grad_scale * sqrt(sum), non-finite
 * exactly when some element is; coef = min(1, max_norm / (norm + 1e-6)) in fp64 (max_norm = +inf: exactly 1).  lr and
 * grad_scale are dev_hyper[0] and dev_hyper[3] (device memory, srad_set4).  A finite norm sets apply = 1, t = ++applied,
 * counts clipped when coef < 1 and writes the record with both bias corrections formed in fp64 from the fp32 betas; a
 * non-finite one sets apply = 0 and counts skipped.  last_norm = norm either way.
 * srad_adam_guarded_step / srad_adam_ema_guarded_step: srad_adam_step_dev / srad_adam_ema_step_dev on the record's four
 * scalars, the same bits; with apply = 0 no buffer is read or written.
 * Refused before anything is launched: null pointers, n <= 0, first_slot < 0, n_slots < 1, max_norm <= 0 or NaN, a
 * workspace that is misaligned or smaller than the slots named, a workspace overlapping grads or dev_hyper, the state and
 * record overlapping any Adam buffer, and what the unguarded steps refuse. */
int srad_grad_guard_workspace(int64_t n, int* slots, size_t* bytes);
int srad_grad_guard_partials(const float* grads, int64_t n, void* workspace, size_t workspace_bytes, int first_slot,
                             void* stream);
int srad_grad_guard_finalize(void* workspace, size_t workspace_bytes, int n_slots, const float* dev_hyper, float beta1,
                             float beta2, double max_norm, void* stream);
int srad_adam_guarded_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float beta1,
                           float beta2, float eps, float weight_decay, const void* workspace, void* stream);
int srad_adam_ema_guarded_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                               float beta1, float beta2, float eps, float weight_decay, float ema_decay, const void* workspace,
                               void* stream);
/* dst[0..3] = (a, b, c, d), passed by value through a kernel launch (no host copy, no synchronisation) */
int srad_set4(float* dst, float a, float b, float c, float d, void* stream);

/* ------------------------------------------------------------------ DRN-L (src/drn.py:160-270) */
typedef struct srad_drn srad_drn_t;
typedef struct {
  int32_t n_colors;  /* opt.n_colors                */
  int32_t scale;     /* max(opt.scale): 2, 4 or 8   */
  int32_t n_blocks;  /* opt.n_blocks                */
  int32_t n_feats;   /* opt.n_feats                 */
  float negval;      /* opt.negval = 0.2            */
  float rgb_range;   /* opt.rgb_range = 255         */
  int32_t precision;
  int32_t use_graph;
} srad_drn_config;

int srad_drn_create(const srad_drn_config* cfg, srad_drn_t** out);
void srad_drn_destroy(srad_drn_t* h);
int srad_drn_arena_bytes(const srad_drn_t* h, size_t* bytes);
int srad_drn_bind_arena(srad_drn_t* h, void* arena, size_t bytes);
int srad_drn_num_params(const srad_drn_t* h);
int srad_drn_param_info(const srad_drn_t* h, int idx, const char** name, int64_t* numel);
int srad_drn_set_param(srad_drn_t* h, const char* name, const float* dev_src, int64_t numel, void* stream);
int srad_drn_workspace_bytes(const srad_drn_t* h, int B, int H, int W, size_t* bytes);
/* DRN.forward (src/drn.py:241-270): returns phase+1 images coarse -> fine; ys[i] is the device
 * pointer of output i with shape [B, C, H*2^i*..]: ys[0] = LR size, ys[phase] = H*scale. */
int srad_drn_forward(srad_drn_t* h, const float* x, int B, int H, int W, float* const* ys, int n_out,
                     void* workspace, size_t workspace_bytes, void* stream);
int srad_drn_flops(const srad_drn_t* h, int B, int H, int W, double* flops);

/* Dual regression model DownBlock(opt, 2) (src/model.py:8-44,78-82): two bias-free 3x3 convs,
 * the first stride 2 + LeakyReLU(negval).  w0 [n_feats,C,3,3], w1 [C,n_feats,3,3] fp32 device.
 * x [B,C,H,W] -> y [B,C,H/2,W/2].  workspace >= srad_dual_workspace_bytes. */
int srad_dual_workspace_bytes(int B, int C, int H, int W, int n_feats, size_t* bytes);
int srad_dual_forward(const float* w0, const float* w1, int C, int n_feats, float negval, const float* x, int B,
                      int H, int W, float* y, void* workspace, size_t workspace_bytes, int precision, void* stream);

/* ------------------------------------------------------------------ DRN training step (src/trainer.py:161-205)
 * Same scheme as the DRCT training entry points: flat fp32 parameter / gradient buffers with the offsets of
 * srad_drn_train_param_offset, a second caller-owned arena, srad_drn_sync_params after every optimizer step.
 * n_feats must be a multiple of 4 (the x2 / x4 presets). */
int srad_drn_train_param_floats(srad_drn_t* h, int64_t* total);
int srad_drn_train_param_offset(srad_drn_t* h, int idx, int64_t* off_floats);
int srad_drn_train_arena_bytes(srad_drn_t* h, size_t* bytes);
int srad_drn_train_bind(srad_drn_t* h, void* train_arena, size_t bytes);
int srad_drn_sync_params(srad_drn_t* h, const float* dev_flat_params, void* stream);
int srad_drn_train_workspace_bytes(const srad_drn_t* h, int B, int H, int W, size_t* bytes);
/* model.train() forward of DRN (src/drn.py:241-270); saved activations stay in `workspace` for srad_drn_backward */
int srad_drn_forward_train(srad_drn_t* h, const float* x, int B, int H, int W, float* const* ys, int n_out,
                           void* workspace, size_t workspace_bytes, void* stream);
/* dys[j] = dLoss/d(output j) (NCHW device pointers, NULL when output j is not in the loss); parameter gradients are
 * ACCUMULATED into dev_flat_grad (incl. the trainable MeanShift layers, hazard H4).  on_bucket (optional): as
 * srad_drct_backward - called on the host when the last kernel writing gradient bucket b has been enqueued; buckets
 * (srad_drn_bucket_range, completion order): 0 = tail convs, 1..phase = up phases finest first, phase + 1 = the rest. */
int srad_drn_num_buckets(const srad_drn_t* h);
int srad_drn_bucket_range(srad_drn_t* h, int bucket, int64_t* off_floats, int64_t* n_floats);
int srad_drn_backward(srad_drn_t* h, const float* const* dys, int n_out, int B, int H, int W, float* dev_flat_grad,
                      void* workspace, size_t workspace_bytes, void* stream, srad_bucket_fn on_bucket, void* user);
/* Backward of the dual regression model (srad_dual_forward; src/trainer.py:168-185 back-propagates through it into the
 * SR outputs): dw0 [n_feats,C,3,3] / dw1 [C,n_feats,3,3] accumulated, dx [B,C,H,W] optional; H and W even */
int srad_dual_backward_workspace_bytes(int B, int C, int H, int W, int n_feats, size_t* bytes);
int srad_dual_backward(const float* w0, const float* w1, int C, int n_feats, float negval, const float* x, int B, int H,
                       int W, const float* dy, float* dx, float* dw0, float* dw1, void* workspace, size_t workspace_bytes,
                       int precision, void* stream);

/* ------------------------------------------------------------------ self-ensemble x8 (DESIGN.md "Self-ensemble")
 * Member t in 0..7 of x [B,C,H,W] is T^(t>>2 & 1)( h^(t>>1 & 1)( v^(t & 1)(x) ) ) with v = flip along W, h = flip along H,
 * T = swap H and W.  srad_ensemble_inputs writes all eight in one launch (x is read once): members 0..3 to out_a
 * [4,B,C,H,W], members 4..7 to out_b [4,B,C,W,H].  srad_ensemble_mean undoes each member's transform on y_a [4,B,C,H,W] /
 * y_b [4,B,C,W,H] (H, W are the OUTPUT's) and writes out [B,C,H,W] = (((z0 + z1) + z2) + ... + z7) * 0.125f: seven fp32
 * additions in member order and one exact scaling, so out is defined bit for bit by its inputs.  The b half may directly
 * follow the a half (a square stack [8,B,C,H,W]: out_b == out_a + 4*B*C*H*W); out must not overlap an input.  Any H, W >= 1;
 * B*C*H*W*8 < 2^31.  Stream-ordered: no host synchronisation, no allocation, no atomics. */
int srad_ensemble_inputs(const float* x, int B, int C, int H, int W, float* out_a /* [4,B,C,H,W] */,
                         float* out_b /* [4,B,C,W,H] */, void* stream);
int srad_ensemble_mean(const float* y_a /* [4,B,C,H,W] */, const float* y_b /* [4,B,C,W,H] */, int B, int C, int H, int W,
                       float* out /* [B,C,H,W] */, void* stream);

/* ------------------------------------------------------------------ tiled inference (DESIGN.md "Tiled inference")
 * An LR image [h, w] is covered with overlapping tiles, the network runs on the tiles, and the tile outputs are blended into the
 * image's output.  srad_tile_plan is the one place where the cover is decided (host only, needs no GPU); the two kernels'
 * launchers call it themselves, so a caller passes the same six numbers everywhere.  Per axis, for an extent n:
 *   padded extent p = ceil(n / granule) * granule; tile extent t = min(tile, p); stride S = tile - overlap;
 *   origins = 0, S, 2S, ... below p - t, then p - t (the last tile snapped to the edge, no origin twice): origin k = min(kS, p - t);
 *   padded coordinate i reads source coordinate r(i): j = i mod 2n, r = j < n ? j : 2n - 1 - j (symmetric reflection with the
 *   edge sample repeated, periodic, so defined for any n >= 1).
 * Tiles are numbered row-major (y outer, x inner), image-major across a batch.  Refused: tile < 1, overlap outside [0, tile),
 * granule < 1 or tile % granule != 0, scale < 1, overlap * scale > 4094 (every blend weight a <= 4095 and every product a_y * a_x
 * stays an exact fp32 integer), and extents that do not fit 32 bits.  The two kernels also refuse 2^31 tiles or more in a batch;
 * their element offsets are 64-bit. */
typedef struct {
  int32_t h, w, tile, overlap, granule, scale; /* as asked */
  int32_t ph, pw;                              /* padded extents */
  int32_t ty, tx;                              /* tile extents (LR) */
  int32_t stride;                              /* tile - overlap */
  int32_t ny, nx;                              /* tiles per axis */
} srad_tile_geom;
#define SRAD_TILE_BLEND_MEAN 0
#define SRAD_TILE_BLEND_FEATHER 1
int srad_tile_plan(int h, int w, int tile, int overlap, int granule, int scale, srad_tile_geom* geom);
int srad_tile_origins(const srad_tile_geom* geom, int32_t* oy /* [ny] */, int32_t* ox /* [nx] */);
/* x [B,C,h,w] -> tiles [B*ny*nx, C, ty, tx]: a copy through r(), the padding included; no arithmetic.  tiles must not overlap x. */
int srad_tile_gather(const float* x, int B, int C, int h, int w, int tile, int overlap, int granule, float* tiles, void* stream);
/* y [B*ny*nx, C, ty*scale, tx*scale] (the network's outputs for the tiles of srad_tile_gather) -> out [B,C,h*scale,w*scale], the
 * padding cropped away.  Gather form: every output pixel sums the tiles that cover it, in tile order, without atomics, so out is
 * defined bit for bit by its inputs.  With v_k the covering tiles' values at the pixel, every product and sum rounded to fp32:
 *   SRAD_TILE_BLEND_MEAN:    acc = v_0; acc = acc + v_k; out = acc / (float)count
 *   SRAD_TILE_BLEND_FEATHER: w_k = a_y * a_x with a(U) = min(U + 1, E - U, overlap * scale + 1) at local HR coordinate U of a tile
 *                            of HR extent E; acc = (float)w_0 * v_0; acc = acc + (float)w_k * v_k; out = acc / (float)(sum of w_k)
 * (the divisions correctly rounded).  A pixel that one tile covers is that tile's value; overlap 0 makes both modes a copy.
 * out must not overlap y.  Stream-ordered: no host synchronisation, no allocation. */
int srad_tile_blend(const float* y, int B, int C, int h, int w, int tile, int overlap, int granule, int scale, int mode, float* out,
                    void* stream);

/* ------------------------------------------------------------------ 8-bit resize, equal to PIL.Image.resize (DESIGN.md "Resize
 * on the device"; scripts/prepare_mvtec_data.py:22-33 calls it with LANCZOS).  A table holds one axis: for every output index the
 * first source index and tap count (bounds [out_size][2]) and the taps as int32 with 22 fractional bits (coeffs
 * [out_size][ksize]), computed on the HOST by srad_resample_coeffs in Pillow's own arithmetic; neither function needs a GPU.
 * srad_resize_u8 resizes u8 images src [n,H,W,C] (C = 1..4) to dst [n,h,w,C]: the horizontal pass first, rounded to u8 in tmp
 * [n,H,w,C], then the vertical pass; a pass whose sizes agree is skipped (its table may be NULL, and tmp when only one pass
 * runs), both skipped is a copy.  Every table carries its bounds twice: `bounds` on the host, which the call checks against the
 * source before it launches, and `dev_bounds` / `dev_coeffs`, the device copies the kernels read.  dst and tmp must overlap
 * neither src nor each other.  Integer arithmetic only (int32 accumulators, as Pillow), 64-bit offsets, stream-ordered, no
 * allocation. */
#define SRAD_RESAMPLE_LANCZOS 0
#define SRAD_RESAMPLE_BICUBIC 1
typedef struct {
  int32_t in_size, out_size, ksize;
  const int32_t* bounds;     /* host   [out_size][2] */
  const int32_t* dev_bounds; /* device [out_size][2] */
  const int32_t* dev_coeffs; /* device [out_size][ksize] */
} srad_resample_table;
int srad_resample_ksize(int in_size, int out_size, int filter, int* ksize);
int srad_resample_coeffs(int in_size, int out_size, int filter, int32_t* bounds /* [out_size][2] */,
                         int32_t* coeffs /* [out_size][ksize] */);
int srad_resize_u8(const uint8_t* src, int n, int H, int W, int C, uint8_t* dst, int h, int w, const srad_resample_table* x_table,
                   const srad_resample_table* y_table, uint8_t* tmp, void* stream);

/* ------------------------------------------------------------------ float32 resize, equal to PIL's mode-F Image.resize (DESIGN.md
 * "Maps and masks at source size").  Pillow resamples float32 images with the taps in double, divided by their sum and not
 * brought to fixed point; a pass is `ss = 0.0; for x < xmax: ss += (double)src[xmin + x] * k[x]; out = (float)ss` - sequential
 * fp64 products and sums, no fused multiply-add - horizontal first, its result rounded to float32.  A table holds one axis:
 * bounds [out_size][2] as above and the taps as double (coeffs [out_size][ksize], zero from xmax on), computed on the HOST by
 * srad_resample_coeffs_f64; neither table function needs a GPU.  These functions take BILINEAR as well (the 8-bit ones refuse
 * it).  srad_resize_f32 resizes maps src [n,H,W] to dst [n,h,w] through tmp [n,H,w]: a pass whose sizes agree is skipped (its
 * table may be NULL, and tmp when only one pass runs), both skipped is a copy.  A table carries `bounds` on the host, which the
 * call checks against the source before it launches, and the device copies the kernels read.  dst and tmp must overlap
 * neither src nor each other.  One thread per output value, 64-bit offsets, stream-ordered, no allocation, no host
 * synchronisation; one launch per pass, which takes n * H < 2^26 (horizontal), n * h < 2^24 (vertical) and w < 2^22.  NaN and
 * infinities travel as in Pillow: through every output whose taps reach them. */
#define SRAD_RESAMPLE_BILINEAR 2
typedef struct {
  int32_t in_size, out_size, ksize;
  const int32_t* bounds;     /* host   [out_size][2] */
  const int32_t* dev_bounds; /* device [out_size][2] */
  const double* dev_coeffs;  /* device [out_size][ksize] */
} srad_resample_table_f;
int srad_resample_ksize_f64(int in_size, int out_size, int filter, int* ksize);
int srad_resample_coeffs_f64(int in_size, int out_size, int filter, int32_t* bounds /* [out_size][2] */,
                             double* coeffs /* [out_size][ksize] */);
int srad_resize_f32(const float* src, int n, int H, int W, float* dst, int h, int w, const srad_resample_table_f* x_table,
                    const srad_resample_table_f* y_table, float* tmp, void* stream);

/* ------------------------------------------------------------------ overlay (DESIGN.md "Maps and masks at source size")
 * out u8 [n,H,W,3] = the images src u8 [n,H,W,Cs] (Cs = 1: gray, replicated; Cs = 3) under a heat map and a mask outline.  Per
 * pixel: q = maps * scale (one fp32 multiply), level = q >= 255 ? 255 : q > 0 ? (int)q : 0 (a NaN map value gives level 0),
 * (r, g, b, a) = lut[level] (lut: DEVICE u8 [256][4]) and out_c = (src_c * (255 - a) + lut_c * a + 127) / 255 in integers.  A
 * pixel whose mask (u8 [n,H,W]) is nonzero and which has, within Chebyshev distance contour_radius (0 .. 4), a pixel with mask 0
 * or one outside the image takes the contour colour (each 0 .. 255) instead; radius 0 draws no contour.  out must overlap no
 * input.  One thread per pixel, 64-bit offsets, stream-ordered, no atomics, no workspace. */
int srad_overlay_rgb(const uint8_t* src, int n, int H, int W, int Cs, const float* maps, const uint8_t* masks, const uint8_t* lut,
                     float scale, int contour_radius, int contour_r, int contour_g, int contour_b, uint8_t* out, void* stream);

/* ------------------------------------------------------------------ scorer (src/evaluate.py:204-265) */
/* `mul(255/range).clamp(0,255).byte()` TRUNCATING u8 conversion + NCHW->HWC (evaluate.py:214-215). */
int srad_to_u8_hwc(const float* x, int B, int C, int H, int W, float rgb_range, uint8_t* out, void* stream);
/* quantize (src/trainer.py:45-47): mul, clamp, round-half-even, div; in-place allowed */
int srad_quantize(const float* x, float* y, int64_t n, float rgb_range, void* stream);
/* Per-pair scores for `n_img` u8 HWC image pairs (sr, hr, each [n_img,H,W,C]):
 *   ssim_out[i*n_ws + j] = ssim_numpy(hr_i/255, sr_i/255, ws[j])   (src/metrics.py:26-67)
 *   mse_out[i] = mean((sr_i/255 - hr_i/255)^2), psnr_out[i] = psnr_numpy (inf when mse == 0)
 * Outputs are DEVICE double arrays; workspace >= srad_score_workspace_bytes. */
int srad_score_workspace_bytes(int n_img, int H, int W, size_t* bytes);
/* The path srad_score_pairs takes for n_img H x W pairs: *kernel = the SSIM sweep's evaluation kernel (0 = the LDS sweep for
 * power-of-two widths 64..1024, 1 = the corner kernel for other multiples of 64 wide, 2 = the kernel for any width), *chunk =
 * images per summed-area table chunk (the pairs run in ceil(n_img / chunk) chunks).  Host only, no device needed. */
int srad_score_plan(int n_img, int H, int W, int* kernel, int* chunk);
int srad_score_pairs(const uint8_t* sr, const uint8_t* hr, int n_img, int H, int W, int C, const int32_t* ws_host,
                     int n_ws, double* ssim_out, double* mse_out, double* psnr_out, void* workspace,
                     size_t workspace_bytes, void* stream);
/* Validation metrics of Trainer.test (src/metrics.py:70-108) on fp32 NCHW tensors, one value per
 * image, device double outputs; reproduces the zero padding, 4-px shave and the 255^2 constants.  A shape the shave leaves
 * no row of (W > 8, H <= 8; the reference's PSNR is NaN there and its SSIM raises) is refused with SRAD_ERR_ARG. */
int srad_val_metrics(const float* sr, const float* hr, int B, int C, int H, int W, float rgb_range,
                     double* psnr_out, double* ssim_out, void* workspace, size_t workspace_bytes, void* stream);
/* Binary ROC-AUC == sklearn.metrics.roc_auc_score (ties count one half).  labels/scores are HOST
 * arrays (n is the number of test images, a few hundred); returns non-zero if one class is absent. */
int srad_roc_auc(const int32_t* labels, const double* scores, int n, double* auc);
/* Binary average precision == sklearn.metrics.average_precision_score (the sum over distinct scores from the highest down of
 * (R_k - R_k-1) * P_k), and the best F1 = 2 tp / (tp + fp + P) over the same thresholds, compared exactly in integers.  HOST
 * arrays like srad_roc_auc; returns non-zero for a NaN score and when no label is positive. */
int srad_average_precision(const int32_t* labels, const double* scores, int n, double* ap, double* f1max);
/* Per-pixel anomaly maps for `n_img` u8 HWC image pairs (sr, hr, each [n_img,H,W,C]) at ONE window size `ws`:
 *   map_out[i, y, x] = 1 - ssim_map(hr_i/255, sr_i/255, ws)[y, x]      (src/metrics.py:26-67; the array line 66 averages)
 * with the arithmetic of srad_score_pairs: luminance, float64 box sums with numpy "reflect" padding, C1 = 1e-4, C2 = 9e-4, the
 * per-pixel fp32 operations in the order of metrics.py:58-66.  map_out is a DEVICE float32 array [n_img, H, W]; window sizes
 * srad_score_pairs rejects are rejected; workspace >= srad_anomaly_map_workspace_bytes.  Any width. */
int srad_anomaly_map_workspace_bytes(int n_img, int H, int W, size_t* bytes);
int srad_anomaly_maps(const uint8_t* sr, const uint8_t* hr, int n_img, int H, int W, int C, int ws, float* map_out,
                      void* workspace, size_t workspace_bytes, void* stream);
/* Multi-scale anomaly maps: the maps of srad_anomaly_maps at the `n_ws` >= 1 window sizes of the HOST list `ws_host` (any
 * length; duplicates count twice), reduced per pixel in one pass over the tables - no map per size is stored.  With
 * d_k = 1 - ssim_map at ws_host[k - 1], every step one IEEE fp32 operation:
 *   reduce 0 (mean): a_1 = d_1, a_k = a_(k-1) + d_k in LIST ORDER, map_out = a_K * (float)(1.0 / n_ws)
 *   reduce 1 (max):  a_1 = d_1, a_k = fmaxf(a_(k-1), d_k), map_out = a_K
 * so map_out is bit for bit the srad_anomaly_maps outputs accumulated that way, and n_ws = 1 gives srad_anomaly_maps itself.
 * Every size must pass the window check of srad_anomaly_maps; workspace >= srad_anomaly_map_workspace_bytes. */
int srad_anomaly_maps_multi(const uint8_t* sr, const uint8_t* hr, int n_img, int H, int W, int C, const int32_t* ws_host,
                            int n_ws, int reduce, float* map_out, void* workspace, size_t workspace_bytes, void* stream);
/* Squared-error maps, the per-pixel form of the MSE score (src/evaluate.py:251-265), for `n_img` u8 HWC image pairs at ONE
 * window size `ws`: with e[y, x] = sum_c (sr - hr)^2 (an integer) and S = the sum of e over the window of srad_anomaly_maps
 * (numpy "reflect" padding, rows y - ws/2 .. y + ws - 1 - ws/2, columns likewise; an exact integer),
 *   map_out[i, y, x] = (float)((double)S * inv),   inv = 1.0 / (C * ws * ws * 65025) in double
 * - one fp64 multiply and one rounding, so the map is defined bit for bit; values lie in [0, 1].  ws = 1 is the raw per-pixel
 * squared error (its mean is the image's MSE) and needs no table.  map_out is a DEVICE float32 array [n_img, H, W]; the window
 * check is that of srad_anomaly_maps; workspace >= srad_error_map_workspace_bytes.  Any width. */
int srad_error_map_workspace_bytes(int n_img, int H, int W, size_t* bytes);
int srad_error_maps(const uint8_t* sr, const uint8_t* hr, int n_img, int H, int W, int C, int ws, float* map_out,
                    void* workspace, size_t workspace_bytes, void* stream);
/* Multi-scale squared-error maps (src/evaluate.py:251-265 per pixel and window): the maps d_k of srad_error_maps at the `n_ws`
 * >= 1 sizes of the HOST list `ws_host`, reduced per pixel exactly as srad_anomaly_maps_multi reduces its maps (reduce 0: fp32
 * sum in LIST ORDER times (float)(1.0 / n_ws); reduce 1: fmaxf), so map_out is bit for bit the srad_error_maps outputs
 * accumulated that way and n_ws = 1 gives srad_error_maps itself.  workspace >= srad_error_map_workspace_bytes. */
int srad_error_maps_multi(const uint8_t* sr, const uint8_t* hr, int n_img, int H, int W, int C, const int32_t* ws_host,
                          int n_ws, int reduce, float* map_out, void* workspace, size_t workspace_bytes, void* stream);
/* Gradient-magnitude similarity maps (GMSD, Xue et al. 2014; multi-scale as RIAD's MSGMS, Zavrtanik et al. 2021) of `n_img` u8
 * HWC image pairs over `levels` = L in 1..4 pyramid levels; H and W multiples of 2^(L-1), H >> (L-1) and W >> (L-1) >= 2.
 * Every step is one IEEE operation in the stated precision (no contraction), so the map is defined up to the device's sqrt
 * and division, both correctly rounded:
 *   s_0[y, x] = sum_c u8 (an integer <= 765); s_l = the 2x2 block sums of s_(l-1) (exact integers <= 765 * 4^l)
 *   per level and stack, numpy "reflect" padding by one pixel, the Prewitt sums as tap-pair differences
 *     Gx = (p[y-1,x+1] - p[y-1,x-1]) + (p[y,x+1] - p[y,x-1]) + (p[y+1,x+1] - p[y+1,x-1]), Gy likewise along the other axis,
 *     M = Gx * Gx + Gy * Gy in int64 (past 2^32 at level 3)
 *   with Ma of sr, Mb of hr, K_l = 3 * C * 255 * 4^l and cK2_l = 0.0026 * K_l * K_l (a host double), in float64
 *     r = sqrt((double)Ma) - sqrt((double)Mb);   d_l = (r * r) / ((double)(Ma + Mb) + cK2_l)
 *   which is 1 - (2 ga gb + c) / (ga^2 + gb^2 + c) for magnitudes in [0, 1] units without the cancellation: exactly 0 for
 *   identical inputs, never negative, below 1, bit-symmetric in (sr, hr)
 *   levels l >= 1 are upsampled bilinearly (align_corners = False) with f = 2^l: o = (y + 0.5) / f - 0.5, i0 = floor(o),
 *     t = o - i0 (dyadic, exact), both neighbour indices clamped to [0, h_l - 1],
 *     u_l = (d[i0,j0] * (1 - tx) + d[i0,j1] * tx) * (1 - ty) + (d[i1,j0] * (1 - tx) + d[i1,j1] * tx) * ty   in float64, this order
 *   map_out = (float)((d_0 + u_1 + ... + u_(L-1)) * (1.0 / L)), summed in level order: one rounding to fp32.
 * map_out is a DEVICE float32 array [n_img, H, W]; any width, the stacks may start at any byte.  The workspace is linear in
 * n_img (no chunks): workspace >= srad_gms_map_workspace_bytes.  All argument checks come before any launch. */
int srad_gms_map_workspace_bytes(int n_img, int H, int W, int levels, size_t* bytes);
int srad_gms_maps(const uint8_t* sr, const uint8_t* hr, int n_img, int H, int W, int C, int levels,
                  float* map_out, void* workspace, size_t workspace_bytes, void* stream);
/* Exact ROC-AUC of `n` DEVICE float32 scores against DEVICE u8 labels (labels[i] != 0 = positive), n < 2^31:
 * sklearn.metrics.roc_auc_score as the Mann-Whitney U with ties counted one half (a device radix sort, no binning).
 *   counts_out (DEVICE, 4 x u64) = {n_pos, n_neg, n_nan, twice_U};  *auc_out (DEVICE double) = twice_U / (2 n_pos n_neg),
 *   NaN when a class is absent.  NaN scores are left out of n_pos, n_neg and twice_U and counted in n_nan.
 * Stream-ordered like the other scorer entry points; workspace >= srad_pixel_auc_workspace_bytes(n) (about 17 bytes per score). */
int srad_pixel_auc_workspace_bytes(int64_t n, size_t* bytes);
int srad_pixel_roc_auc(const float* scores, const uint8_t* labels, int64_t n, uint64_t* counts_out, double* auc_out,
                       void* workspace, size_t workspace_bytes, void* stream);
/* Exact precision-recall of `n` DEVICE float32 scores against DEVICE u8 labels (labels[i] != 0 = positive), n < 2^31: every
 * distinct score s (-0.0 == +0.0) is a threshold "predict iff score >= s", from the highest down (DESIGN.md "Precision-recall").
 *   counts_out (DEVICE, 7 x u64) = {n_pos, n_neg, n_nan, n_points, best_tp, best_fp, best_score_bits}: the point of the highest
 *   F1 = 2 tp / (tp + fp + n_pos), compared exactly in integers, the higher threshold keeping a tie, and the float32 bits of its
 *   score;  *ap_out (DEVICE double) = sklearn.metrics.average_precision_score, NaN when n_pos == 0.
 *   curve_precision / curve_recall (DEVICE double) and curve_score (DEVICE float32), all three or none NULL, receive the first
 *   min(curve_cap, n_points) points (no (1, 0) end point is appended).
 * NaN scores are left out of every count but n_nan.  Stream-ordered, no host sync; the same device sort and scan as
 * srad_pixel_roc_auc; workspace >= srad_pixel_pr_workspace_bytes(n) (about 17 bytes per score). */
int srad_pixel_pr_workspace_bytes(int64_t n, size_t* bytes);
int srad_pixel_pr(const float* scores, const uint8_t* labels, int64_t n, uint64_t* counts_out, double* ap_out,
                  double* curve_precision, double* curve_recall, float* curve_score, int64_t curve_cap, void* workspace,
                  size_t workspace_bytes, void* stream);
/* Regions of DEVICE u8 masks [n_img, H, W] (nonzero = defect), n_img x H x W in [1, 2^31): the 8-connected components of each
 * image's mask (scipy.ndimage.label with a 3 x 3 structure, per image; nothing connects across images).
 *   region_size_out[i] (DEVICE u32) = |region of pixel i|, 0 where mask == 0;
 *   counts_out (DEVICE, 3 x u64) = {n_regions, n_ok, n_defect}.
 * Stream-ordered; workspace >= srad_mask_regions_workspace_bytes (4 bytes per pixel). */
int srad_mask_regions_workspace_bytes(int n_img, int H, int W, size_t* bytes);
int srad_mask_regions(const uint8_t* masks, int n_img, int H, int W, uint32_t* region_size_out, uint64_t* counts_out,
                      void* workspace, size_t workspace_bytes, void* stream);
/* AU-PRO (Bergmann et al., IJCV 2021) of DEVICE float32 scores [n_img, H, W] against DEVICE u8 masks of the same shape: the area
 * under the per-region overlap curve up to fpr_limit (in (0, 1]), divided by fpr_limit.  Every distinct score is a threshold
 * (-0.0 == +0.0); the curve is (0,0), (fpr, pro) at each threshold from the highest down, (1,1) (DESIGN.md "AU-PRO").
 *   counts_out (DEVICE, 5 x u64) = {n_regions, n_ok, n_defect, n_nan, n_curve_points};
 *   *aupro_out (DEVICE double) = the normalised AU-PRO, NaN when n_regions == 0 or n_ok == 0;
 *   curve_fpr / curve_pro (DEVICE double, both or neither may be NULL) receive the first min(curve_cap, n_curve_points) points.
 * NaN scores are left out of the curve and counted in n_nan.  Stream-ordered, no host sync; workspace >=
 * srad_pixel_pro_workspace_bytes (about 17 bytes per pixel). */
int srad_pixel_pro_workspace_bytes(int n_img, int H, int W, size_t* bytes);
int srad_pixel_pro(const float* scores, const uint8_t* masks, int n_img, int H, int W, double fpr_limit, uint64_t* counts_out,
                   double* aupro_out, double* curve_fpr, double* curve_pro, int64_t curve_cap, void* workspace,
                   size_t workspace_bytes, void* stream);
/* The value of ascending rank k (0-based) of `n` DEVICE float32 scores, 1 <= n < 2^31, 0 <= k < n: an exact radix select over
 * the order-preserving key of a float (-0.0 == +0.0, and a zero is returned as +0.0; NaN sorts last).  Three histogram passes
 * over the scores (11 / 11 / 10 key bits, each restricted to the prefix chosen so far); nothing is sorted or moved and the
 * workspace does not grow with n.  The result is always one of the scores.
 *   *value_out (DEVICE float) = the score of rank k (NaN when rank k falls among the NaN);
 *   counts_out (DEVICE, 3 x u64) = {n_nan, n_below, n_equal}: scores below and equal to the value, so that
 *   n_above = n - n_nan - n_below - n_equal (n_equal = 0 when the value is NaN).
 * Integer counts only: the same bits on every call.  Stream-ordered, no host sync, no allocation; workspace >=
 * srad_select_kth_workspace_bytes (about 25 KB whatever n). */
int srad_select_kth_workspace_bytes(int64_t n, size_t* bytes);
int srad_select_kth(const float* scores, int64_t n, int64_t k, float* value_out, uint64_t* counts_out, void* workspace,
                    size_t workspace_bytes, void* stream);
/* The operating point of DEVICE float32 scores [n_img, H, W] at `threshold` (DESIGN.md "Operating point"): a pixel is predicted
 * defective iff score > threshold, strictly (never for a NaN score); with min_area > 1 every 8-connected component of an
 * image's predicted set (the connectivity of srad_mask_regions) of fewer than min_area pixels is then removed.  masks: DEVICE
 * u8 of the same shape (nonzero = defect), or NULL = no defect anywhere.
 *   pred_out (DEVICE u8 [n_img, H, W]) = 1 where a predicted pixel survives, else 0;
 *   img_pred_out (DEVICE u32 [n_img]) = surviving predicted pixels of each image;
 *   counts_out (DEVICE, 8 x u64) = {tp, fp, fn, tn, n_nan, n_regions, pro_hi, pro_lo}: the pixel confusion counts (a pixel with
 *   a NaN score is in n_nan and in no other count), the regions of the masks (0 without masks), and the 128-bit fixed-point
 *   numerator pro_hi * 2^64 + pro_lo = sum over predicted defect pixels of floor(2^64 / |region of the pixel|), the same sum
 *   srad_pixel_pro carries: pro = numerator / 2^64 / n_regions.
 * A NaN threshold and min_area < 1 are refused; +-infinity and min_area > H x W are valid.  Launches: threshold; (min_area > 1)
 * srad_mask_regions on the prediction, drop small components; (masks) srad_mask_regions on the masks; count per block; final
 * reduce.  Integer sums only.  Stream-ordered, no host sync, no allocation; workspace >= srad_operating_point_workspace_bytes
 * (about 8 bytes per pixel). */
int srad_operating_point_workspace_bytes(int n_img, int H, int W, size_t* bytes);
int srad_operating_point(const float* scores, const uint8_t* masks, int n_img, int H, int W, float threshold, int min_area,
                         uint8_t* pred_out, uint32_t* img_pred_out, uint64_t* counts_out, void* workspace, size_t workspace_bytes,
                         void* stream);
/* One record of srad_region_table (56 bytes). */
typedef struct {
  int32_t image;              /* index into the stack */
  int32_t area;               /* pixels of the region */
  int32_t y0, x0, y1, x1;     /* bounding box, inclusive */
  uint64_t sum_y, sum_x;      /* sums of the member pixels' coordinates: centroid = sum / area */
  int32_t overlap;            /* member pixels with other != 0 (0 without `other`) */
  float peak;                 /* with scores: the region's largest score (-0.0 as +0.0); NaN without scores */
  int32_t peak_y, peak_x;     /* where: of equal maxima the first in raster order; -1 without scores */
} srad_region_record;
/* The table of regions of DEVICE u8 masks [n_img, H, W] (nonzero = member), n_img x H x W in [1, 2^31): one record per
 * 8-connected component of each image's mask, with the labelling of srad_mask_regions itself (DESIGN.md "Defect regions").
 * Records are ordered by image and, within an image, by the region's first pixel in raster order - the order of
 * scipy.ndimage.label(mask, ones((3, 3))).  scores: DEVICE float32 of the same shape, or NULL; other: DEVICE u8 of the same
 * shape, or NULL.
 *   records_out (DEVICE, cap x srad_region_record; may be NULL when cap == 0) receives the first min(R, cap) records;
 *   counts_out (DEVICE, 3 x u64) = {R = regions over all images (exact whatever cap), NaN scores inside regions, records
 *   written = min(R, cap)}.
 * A NaN score inside a region is counted and never the peak (a region of NaN scores only has peak NaN at (-1, -1)); outside the
 * regions the scores are not read.  cap < 0 is refused.  Launches: the labelling (3), a copy, the rank of the roots (3), one
 * accumulation pass, the peak decode.  Integer sums, minima and maxima only: the same bits on every call.  Stream-ordered, no
 * host sync, no allocation; workspace >= srad_region_table_workspace_bytes (about 12 bytes per pixel). */
int srad_region_table_workspace_bytes(int n_img, int H, int W, size_t* bytes);
int srad_region_table(const uint8_t* masks, const float* scores, const uint8_t* other, int n_img, int H, int W,
                      srad_region_record* records_out, int64_t cap, uint64_t* counts_out, void* workspace, size_t workspace_bytes,
                      void* stream);
/* Gaussian smoothing of DEVICE float32 maps [n_img, H, W] (n_img x H x W < 2^31) with a symmetric separable filter of radius
 * `radius` in [0, 128], radius <= min(H, W) (one half-sample reflection, d c b a | a b c d, at every edge).  weights_host: HOST
 * array of radius + 1 doubles, w[0] the centre and w[j] the weight at offsets +-j.  Given scipy's weights the result equals
 * scipy.ndimage.gaussian_filter(maps, (0, s, s), mode='reflect') bit for bit: the pass along H first, its output rounded to
 * fp32, then the pass along W; in each, acc = x[i] * w[0], then acc = acc + (x[i-j] + x[i+j]) * w[j] for j = radius down to 1 in
 * fp64 without fused multiply-adds, cast to fp32.  radius 0 copies the maps.  out (DEVICE float32 [n_img, H, W]) must not
 * overlap maps.  img_max_out (DEVICE float32 [n_img], may be NULL) receives max(out[i]) per image, NaN if any pixel of image i is
 * NaN.  Stream-ordered and asynchronous: no host sync, no allocation; workspace >= srad_smooth_maps_workspace_bytes (4 bytes
 * per image). */
int srad_smooth_maps_workspace_bytes(int n_img, int H, int W, int radius, size_t* bytes);
int srad_smooth_maps(const float* maps, int n_img, int H, int W, const double* weights_host, int radius, float* out,
                     float* img_max_out, void* workspace, size_t workspace_bytes, void* stream);
/* The per-pixel baseline of anomaly maps (DESIGN.md "Baseline").  maps: DEVICE float32 [n_img, H, W], n_img x H x W in
 * [1, 2^31).  Every operation named below is one IEEE operation, no fused multiply-adds.
 *   srad_map_stats_accumulate: per pixel s1 = s1 + (double)m_i and s2 = s2 + (double)m_i * (double)m_i for i = 0 .. n_img - 1 in
 *     that order, on DEVICE double planes [H, W] the caller has set (zeros for a new fit): a stack split over consecutive calls
 *     gives the bits of one call.  A NaN pixel makes that pixel's sums NaN.  maps, s1 and s2 must not overlap.
 *   srad_map_normalize: out = fl32(fl32(m - mu) * inv_sd) with DEVICE float32 planes mu, inv_sd [H, W]; signed, NaN propagates.
 *   srad_map_normalize_loo: the z-score of a map that is part of sums over n_total >= 3 maps against the other n_total - 1,
 *     in double: x = m, a = s1 - x, q = s2 - x * x, mean = a / (n_total - 1), var = max(q - a * a / (n_total - 1), 0) /
 *     (n_total - 2), sd = max(sqrt(var), floor) with a finite floor > 0 (both maxima keep a NaN), out = (float)((x - mean) / sd).
 * out (DEVICE float32 [n_img, H, W]) may be maps itself (in place); any other overlap is refused.  img_max_out (DEVICE float32
 * [n_img], may be NULL) receives max(out[i]) per image, NaN if any pixel of image i is NaN; it needs workspace >=
 * srad_map_normalize_workspace_bytes (1 KiB per image), which may be NULL otherwise.  Four pixels per thread with 16-byte
 * accesses where H x W is a multiple of 4 and every pointer sits on 16 bytes, one pixel per thread otherwise: the same bits.
 * Stream-ordered and asynchronous: no host sync, no allocation. */
int srad_map_stats_accumulate(const float* maps, int n_img, int H, int W, double* s1, double* s2, void* stream);
int srad_map_normalize_workspace_bytes(int n_img, size_t* bytes);
int srad_map_normalize(const float* maps, int n_img, int H, int W, const float* mu, const float* inv_sd, float* out,
                       float* img_max_out, void* workspace, size_t workspace_bytes, void* stream);
int srad_map_normalize_loo(const float* maps, int n_img, int H, int W, const double* s1, const double* s2, int n_total,
                           double floor, float* out, float* img_max_out, void* workspace, size_t workspace_bytes, void* stream);

/* mean |a-b| (nn.L1Loss, src/loss.py:84) -> *out (device double); workspace >= srad_l1_workspace_bytes */
int srad_l1_workspace_bytes(size_t* bytes);
int srad_l1_loss(const float* a, const float* b, int64_t n, double* out, void* workspace, void* stream);

/* The loss types of the reference's loss factory `Loss(opt, ckp)` (src/loss.py:72-121; the CLI only ever builds '1*L1'):
 *   SRAD_LOSS_L1   nn.L1Loss(reduction='mean')                     (src/loss.py:84)
 *   SRAD_LOSS_MSE  nn.MSELoss()                                    (src/loss.py:82)
 *   SRAD_LOSS_PSNR PSNRLoss: -10 log10(255^2 / (mse + 1e-8))       (src/loss.py:63-70)
 *   SRAD_LOSS_SSIM SSIMLoss / calc_ssim: sum(1 - ssim_map) / batch_size with the 10-px shave, zero-padded 11x11 mean
 *                  filter and the 255^2-scaled constants           (src/loss.py:9-61)
 *   SRAD_LOSS_GMS / SRAD_LOSS_MSGMS (not in the reference) the gradient-magnitude similarity over L = 1 / 4 levels, in fp32:
 *                  x = clamp(t / rgb_range, 0, 1) averaged over the channels, levels by 2x2 averages, reflect padding by
 *                  one pixel, Prewitt tap-pair differences summed then divided by 3, M = gx^2 + gy^2,
 *                  d = (sqrt(Ma) - sqrt(Mb))^2 / (Ma + Mb + 0.0026), loss = (1 / L) sum_l mean_{B, h_l, w_l} d_l (a plain
 *                  mean; batch_size is ignored).  d sqrt(M) / d gx is 0 where M == 0.  sr and hr of one size; MSGMS needs
 *                  H and W multiples of 8 and at least 16 (srad_loss_workspace_bytes refuses other sizes).  On u8-valued
 *                  inputs the loss is the mean of srad_gms_maps.  The backward reads the workspace the forward filled
 *                  and gathers (no atomics): gradients are bit-reproducible.
 * sr [B,C,sH,sW] and hr [B,C,H,W] fp32 NCHW (sH, sW may exceed H, W only for SSIM, which crops sr like the reference).
 * forward: out2[0] = loss, out2[1] = state for the backward (device doubles).  backward: dsr (+)= weight * gscale_dev[0]
 * * dLoss/dsr (gscale_dev may be NULL = 1); SSIM's backward reads the workspace its forward filled. */
#define SRAD_LOSS_L1 0
#define SRAD_LOSS_MSE 1
#define SRAD_LOSS_PSNR 2
#define SRAD_LOSS_SSIM 3
#define SRAD_LOSS_GMS 4
#define SRAD_LOSS_MSGMS 5
int srad_loss_workspace_bytes(int kind, int B, int C, int H, int W, size_t* bytes);
int srad_loss_forward(int kind, const float* sr, const float* hr, int B, int C, int sH, int sW, int H, int W, float rgb_range,
                      int batch_size, double* out2, void* workspace, size_t workspace_bytes, void* stream);
int srad_loss_backward(int kind, const float* sr, const float* hr, int B, int C, int sH, int sW, int H, int W, float rgb_range,
                       int batch_size, const double* fwd_out2, const float* gscale_dev, float weight, float* dsr, int accumulate,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ single operators
 * NHWC / token-major fp32 activations [rows][ld]; channel counts and row strides multiples of 4 floats. */
/* Linear / 1x1 conv / 3x3 conv (pad 1, stride 1|2) with fused prologue + epilogue:
 *   y = act(LN?(x) . w^T + bias) * alpha + r ;  w in PyTorch layout [N][Cin][taps] (packed into scratch)
 *   act: 0 none, 1 GELU(erf), 2 LeakyReLU(slope), 3 ReLU; ps = 2 -> PixelShuffle(2) scatter of the output
 *   nn.Linear (src/drct.py:178-181,262-264), nn.Conv2d (src/drct.py:782,837,844-847; src/drn.py:29-33,95-112) */
size_t srad_op_gemm_scratch_bytes(int precision, int N, int Cin, int ntaps);
int srad_op_gemm(int precision, const float* x, int ldx, int B, int Hi, int Wi, int Cin, const float* w, int N,
                 int ntaps, int stride, const float* bias, const float* ln_g, const float* ln_b, int act, float slope,
                 float alpha, const float* r, int ldr, float* y, int ldy, int yoff, int ps, void* scratch,
                 size_t scratch_bytes, void* stream);
/* Which kernel srad_op_gemm runs for these arguments, decided on the host from shape, precision and pointers alone; launches
 * nothing and needs no GPU (the pointers are compared with NULL and tested for alignment, never dereferenced).  Fails, with the
 * launch's own status and message, for a problem srad_op_gemm refuses.
 *   family : SRAD_GEMM_TILED the row-gather MFMA GEMM; SRAD_GEMM_CONV80 the weight-resident 80 -> 80 channel 3x3 kernel;
 *            SRAD_GEMM_CONV80X4 an 80 -> 320 conv + PixelShuffle(2) as four launches of it; SRAD_GEMM_THIN / SRAD_GEMM_TAIL the
 *            direct kernels for very few input / output channels
 *   TILED  : BM x BN output tile per workgroup, CPS 32-wide K chunks per stage, the LayerNorm / conv-gather / special-epilogue
 *            (PixelShuffle) template variant, and the launch grid (grid_x column tiles x grid_y row tiles)
 *   CONV80 / CONV80X4 : BM x BN = 128 x 80 (four 32-pixel tiles x all channels per step); THIN / TAIL leave the tile fields 0.
 *            Those kernels size their own grids: grid_x = grid_y = 0. */
#define SRAD_GEMM_TILED 0
#define SRAD_GEMM_CONV80 1
#define SRAD_GEMM_CONV80X4 2
#define SRAD_GEMM_THIN 3
#define SRAD_GEMM_TAIL 4
typedef struct {
  int32_t family;            /* SRAD_GEMM_* */
  int32_t BM, BN, CPS;
  int32_t LN, CONV, SPECIAL; /* 0 | 1 */
  int32_t grid_x, grid_y;
  int32_t launches;          /* kernel launches behind the call (the weight pack not counted) */
} srad_gemm_plan;
int srad_op_gemm_plan(int precision, const float* x, int ldx, int B, int Hi, int Wi, int Cin, const float* w, int N,
                      int ntaps, int stride, const float* bias, const float* ln_g, const float* ln_b, int act, float slope,
                      float alpha, const float* r, int ldr, float* y, int ldy, int yoff, int ps, void* scratch,
                      size_t scratch_bytes, void* stream, srad_gemm_plan* plan);
/* WindowAttention core + cyclic shift + window partition/reverse (src/drct.py:271-302,472-506):
 * qkv [B*H*W][3][heads][hdp] (each head slice padded to hdp floats, hdp % 4 == 0) -> out [B*H*W][d] */
int srad_op_window_attn(int precision, const float* qkv, float* out, const float* table, int B, int H, int W, int ws,
                        int shift, int d, int heads, int hdp, void* stream);
/* nn.LayerNorm over the last dimension, eps 1e-5 (src/drct.py:798,833) */
int srad_op_layernorm(const float* x, int ldx, float* y, int ldy, int rows, int C, const float* g, const float* b,
                      void* stream);

/* The two fused launches a Swin block becomes in bf16 and split-bf16 mode with 8 x 8 windows (BASELINE configs C2 / C4; what
 * bench.py times).  precision = SRAD_PRECISION_BF16 | SRAD_PRECISION_BF16X3; in split-bf16 mode the hand-off between the two
 * (out of the first, attn of the second) is fp32 and out_bf16 must be 0.  Weights in PyTorch layout (device fp32), packed into `scratch` (>= srad_op_swin_scratch_bytes, 256-byte aligned).
 *   srad_op_qkv_attn : norm1 -> attn.qkv -> cyclic shift + window partition -> softmax(q k^T * scale + relative position
 *                      bias + 0/-100 shift mask) v -> window reverse + shift back
 *                      (SwinTransformerBlock.forward src/drct.py:477-504 up to attn.proj; WindowAttention.forward 271-299)
 *                      x [B*H*W][ldx] (columns [0,d)) , w_qkv [3d][d], b_qkv [3d], table [225][heads] -> out [B*H*W][d],
 *                      fp32, or bf16 with out_bf16 = 1 (the form the engines hand to the second half)
 *   srad_op_mlp_block: x1 = shortcut + attn.proj(attn); x2 = x1 + mlp(norm2(x1)) (src/drct.py:300, 509-510, 184-190), then
 *                      the RDG's 1x1 adjust conv: y[:, yoff:yoff+no] = act(adjust(x2) + b) * alpha (+ r) (src/drct.py:389-396)
 *                      fm = token rows per workgroup (16 | 32 | 64, 0 = the engine's choice for M); attn is a bf16 [M][d]
 *                      array: the first half's output in the form the MFMA takes it */
size_t srad_op_swin_scratch_bytes(int d, int heads, int m, int no);
int srad_op_qkv_attn(int precision, const float* x, int ldx, int B, int H, int W, int shift, int d, int heads, const float* ln_g,
                     const float* ln_b, const float* w_qkv, const float* b_qkv, const float* table, void* out, int out_bf16,
                     void* scratch, size_t scratch_bytes, void* stream);
/* srad_op_qkv_attn (bf16) with the saves the training backward reads, as the training forward leaves them: out bf16, LN1(x)
 * as fp32 (save_xn) and / or bf16 (save_xn_h) [B*H*W][d], q | k | v as fp32 [B*H*W][3][heads][hdp] (q unscaled; save_qkv)
 * or as bf16 [B*H*W][3][heads][hp_h] exactly as the attention used them (save_qkv_h); null saves are skipped.  no_qsplit = 1
 * launches the plain (windows, heads) grid where the query split would be chosen (A/B of the two paths).
 * srad_qkv_attn_grid: the grid (x, y) srad_op_qkv_attn / the engines launch for this shape on the current device. */
int srad_op_qkv_attn_train(const float* x, int ldx, int B, int H, int W, int shift, int d, int heads, const float* ln_g,
                           const float* ln_b, const float* w_qkv, const float* b_qkv, const float* table, void* out_h,
                           float* save_xn, void* save_xn_h, float* save_qkv, int hdp, void* save_qkv_h, int hp_h, int no_qsplit,
                           void* scratch, size_t scratch_bytes, void* stream);
int srad_qkv_attn_grid(int precision, int B, int H, int W, int d, int heads, int no_qsplit, int* grid_xy);
int srad_op_mlp_block(int precision, int M, int d, int m, int no, int fm, const void* attn, const float* shortcut, int ld_short,
                      const float* w_proj, const float* b_proj, const float* ln_g, const float* ln_b, const float* w_fc1,
                      const float* b_fc1, const float* w_fc2, const float* b_fc2, const float* w_adj, const float* b_adj, int act,
                      float slope, float alpha, const float* r, int ldr, float* y, int ldy, int yoff, void* scratch,
                      size_t scratch_bytes, void* stream);
/* A whole Swin block + the adjust conv as ONE launch (kernels_fused_block.hip): srad_op_qkv_attn followed by srad_op_mlp_block
 * on 16-row tiles, a quarter window per workgroup, the attention output never leaving the CU.  bf16, 8 x 8 windows, inference,
 * B * (H / 8) * (W / 8) * 4 <= the device's CU count; anything else is an error (srad_swin_block_supported tells).  x is
 * LayerNorm1's input and the shortcut; scratch as for the pair (srad_op_swin_scratch_bytes(d, heads, m, no)). */
int srad_swin_block_supported(int precision, int ws, int B, int H, int W, int d, int heads, int m, int no);
int srad_op_swin_block(int precision, const float* x, int ldx, int B, int H, int W, int shift, int d, int heads, int m, int no,
                       const float* ln1_g, const float* ln1_b, const float* w_qkv, const float* b_qkv, const float* table,
                       const float* w_proj, const float* b_proj, const float* ln2_g, const float* ln2_b, const float* w_fc1,
                       const float* b_fc1, const float* w_fc2, const float* b_fc2, const float* w_adj, const float* b_adj, int act,
                       float slope, float alpha, const float* r, int ldr, float* y, int ldy, int yoff, void* scratch,
                       size_t scratch_bytes, void* stream);
/* The folded second half of a Swin block (inference).  Nothing non-linear sits between mlp.fc2 and the RDG's
 * adjust conv, so adjust(x1 + fc2(h) + b2) = [A | A W2] [x1 | h] + (A b2 + b_a): one GEMM with `no` output columns.
 * srad_op_mlp_fold_compose builds, in caller scratch (>= srad_op_mlp_fold_scratch_bytes(d, m, no), 256-byte aligned) and from
 * the fp32 tensors in PyTorch layout, Wf = [A zero-padded to 32 ceil(d / 32) columns | A W2 zero-padded to 32 ceil(m / 32)]
 * as fp32 [no][*kf], its bf16 fragment pack and bf = A b2 + b_a [no]; products accumulate in fp64 and are rounded to fp32 once.
 * The three results lie at the byte offsets it reports.  srad_op_swin_block_folded is srad_op_swin_block with that second
 * half (proj | fc1 | adjF, no fc2 phase); its scratch holds srad_op_swin_scratch_bytes(d, heads, m, no) followed by
 * srad_op_mlp_fold_scratch_bytes(d, m, no).  srad_swin_block_fold_supported: the shapes of srad_swin_block_supported whose
 * adjust width the folded stage takes (no <= 32 or no > 128). */
size_t srad_op_mlp_fold_scratch_bytes(int d, int m, int no);
/* the scratch region's layout, no device needed: off[8] = byte offsets of the copies of w_fc2, b_fc2, w_adj, b_adj, of Wf, the
 * pack and bf, and the region's size */
int srad_op_mlp_fold_layout(int d, int m, int no, size_t* off, int* kf);
int srad_op_mlp_fold_compose(int d, int m, int no, const float* w_fc2, const float* b_fc2, const float* w_adj, const float* b_adj,
                             void* scratch, size_t scratch_bytes, size_t* wf_off, size_t* pack_off, size_t* bias_off, int* kf,
                             void* stream);
int srad_swin_block_fold_supported(int precision, int ws, int B, int H, int W, int d, int heads, int m, int no);
int srad_op_swin_block_folded(int precision, const float* x, int ldx, int B, int H, int W, int shift, int d, int heads, int m, int no,
                              const float* ln1_g, const float* ln1_b, const float* w_qkv, const float* b_qkv, const float* table,
                              const float* w_proj, const float* b_proj, const float* ln2_g, const float* ln2_b, const float* w_fc1,
                              const float* b_fc1, const float* w_fc2, const float* b_fc2, const float* w_adj, const float* b_adj,
                              int act, float slope, float alpha, const float* r, int ldr, float* y, int ldy, int yoff, void* scratch,
                              size_t scratch_bytes, void* stream);
/* The same fold in the two-launch form: srad_op_mlp_block_folded is srad_op_mlp_block (bf16) with the second
 * half proj | fc1 | adjF; its scratch holds srad_op_swin_scratch_bytes(d, 1, m, no) followed by
 * srad_op_mlp_fold_scratch_bytes(d, m, no).  srad_mlp_block_fold_supported: bf16, a shape of the fused second half, an adjust
 * width the folded stage takes (no <= 32 or no > 128) and, at the tile height the launch picks for T rows, a folded tile
 * that fits the LDS (64-row tiles at d = 244 do not).  The DRCT engine folds the launches on 16-row tiles (T < 8192). */
int srad_mlp_block_fold_supported(int precision, int T, int d, int m, int no);
/* weight stages of the second half's chain and of its folded form (0: the adjust width has none) at a block shape of the table */
int srad_mlp_block_stage_counts(int d, int m, int no, int* chain, int* folded);
int srad_op_mlp_block_folded(int precision, int M, int d, int m, int no, int fm, const void* attn, const float* shortcut, int ld_short,
                             const float* w_proj, const float* b_proj, const float* ln_g, const float* ln_b, const float* w_fc1,
                             const float* b_fc1, const float* w_fc2, const float* b_fc2, const float* w_adj, const float* b_adj, int act,
                             float slope, float alpha, const float* r, int ldr, float* y, int ldy, int yoff, void* scratch,
                             size_t scratch_bytes, void* stream);

/* DRCT's output end folded into one launch.  Everything after conv_before_upsample's LeakyReLU - the Upsample
 * convolutions with their PixelShuffles, conv_last, then / img_range + mean (src/drct.py:694-713, 842-847, 894-897) - is linear:
 * the s x s HR pixels of an LR pixel are one 5 x 5 convolution of c2, whose weights and bias depend on whether the pixel lies in
 * the first, an interior or the last row / column (nine classes; the inner convolutions pad their own, finer inputs).
 *   srad_op_tail_fold_layout: byte offsets, in a fold's region, of the fp32 fold wf [9][N][25][F] (N = s s C, output
 *       (c s + py) s + px, tap (dy + 2) 5 + dx + 2), of its bf16 pack [9][NT][25][F / 32][64][8] (NT = ceil(N / 16); lane 16 fq + fr
 *       holds row 16 nt + fr, channels 32 j + 8 fq .. + 7; rows >= N zero) and of the fp32 bias table [9][16 NT], and the region's size
 *   srad_op_tail_fold_build : builds a fold in `scratch` (256-byte aligned, >= that size) from upsample.0 (w_up0 [4F][F][3][3],
 *       b_up0), upsample.2 (w_up1, b_up1; scale 4 only, else NULL) and conv_last (w_last [C][F][3][3], b_last), device fp32
 *   srad_op_tail_fold       : y [B][C][sH][sW] = fold(c2) / img_range + mean_c from c2 [B*H*W][64] fp32 (rounded to bf16 once, fp32
 *       accumulation); F = 64, scale 2 | 4, C 1 | 3, H, W >= 2 */
int srad_op_tail_fold_layout(int F, int C, int scale, size_t* wf_off, size_t* pack_off, size_t* bias_off, size_t* bytes);
int srad_op_tail_fold_build(int F, int C, int scale, const float* w_up0, const float* b_up0, const float* w_up1, const float* b_up1,
                            const float* w_last, const float* b_last, void* scratch, size_t scratch_bytes, void* stream);
int srad_op_tail_fold(const float* c2, int B, int H, int W, int C, int scale, const void* fold, float img_range, float mean0, float mean1,
                      float mean2, float* y, void* stream);

/* The end of the DRCT bf16 inference forward's body as one launch, 16 pixels of an LR row per workgroup.
 * E % 4 == 0, E <= 192, F = 64; rows and vectors 16-byte aligned, scratch 256-byte aligned.
 *   srad_drct_ends_supported     does a bf16 inference forward of this shape take it: the limits above, C 1 | 3 and
 *                                B * H * ceil(W / 16) <= the device's CU count (one round of tiles); _cus: the same on a given count
 *   srad_op_drct_ends_scratch_bytes  scratch the op needs (the two fragment packs it builds from the fp32 weights)
 *   srad_op_drct_body_end        c2 [B*H*W][F] = LeakyReLU_0.01(conv_before_upsample(conv_after_body(LayerNorm(x[:, :E])) + feat0))
 *                                (drct.py:881, 893-894) from x [B*H*W][ldx], w1 [E][E][3][3], w2 [F][E][3][3]; bf16 MFMA operands at
 *                                the chain's rounding points (LayerNorm output, c1), fp32 accumulation */
int srad_drct_ends_supported(int precision, int E, int F, int C, int B, int H, int W);
int srad_drct_ends_supported_cus(int precision, int E, int F, int C, int B, int H, int W, int cus);
size_t srad_op_drct_ends_scratch_bytes(int E, int F);
int srad_op_drct_body_end(const float* x, int ldx, int B, int H, int W, int E, int F, const float* ln_g, const float* ln_b, const float* w1,
                          const float* b1, const float* feat0, const float* w2, const float* b2, float* c2, void* scratch,
                          size_t scratch_bytes, void* stream);

/* The two kernels of BASELINE config C5's attention (bf16, 64 x 64 windows = 4096-token windows; src/main.py:286), each on its own:
 *   srad_op_ln_qkv              norm1 + attn.qkv (src/drct.py:477, 278) -> qkv_h [M][3][heads][hdp] bf16, the attention's MFMA
 *                               operands: q times qscale (= head_dim^-0.5 log2 e, srad_op_window_attn_qscale), padding columns 0,
 *                               column head_dim of every v slice 1 (P.V then also yields the softmax denominator); M % 64 == 0
 *   srad_op_window_attn_bf16_in WindowAttention.forward on those operands (src/drct.py:281-299 and the roll / partition / reverse
 *                               around it, 482-504): online softmax over 64-key chunks = rows of the window, relative position
 *                               bias rows sliding through an LDS ring, 0 / -100 shift mask; out [B*H*W][d] fp32 */
float srad_op_window_attn_qscale(int ws, int shift, int d, int heads);
size_t srad_op_ln_qkv_scratch_bytes(int d, int heads);
int srad_op_ln_qkv(const float* x, int ldx, int M, int d, int heads, const float* ln_g, const float* ln_b, const float* w_qkv,
                   const float* b_qkv, void* qkv_h, int hdp, float qscale, void* scratch, size_t scratch_bytes, void* stream);
int srad_op_window_attn_bf16_in(const void* qkv_h, float* out, const float* table, int B, int H, int W, int ws, int shift, int d,
                                int heads, int hdp, void* stream);

/* Backward operators (autograd of the rows above).
 * Weight/bias gradient of Linear / conv: dw[N][Cin][taps] += alpha * dy^T A(x), db[N] += alpha * colsum(dy);
 * dy [B*Ho*Wo][ldy], x [B*Hi*Wi][ldx]; N, Cin multiples of 4; row_scale optional per-sample factor [B].
 * Split-K partials are summed in a fixed order by a second kernel: results are bit-reproducible. */
int srad_op_wgrad(int precision, const float* dy, int ldy, const float* x, int ldx, int B, int Hi, int Wi, int N,
                  int Cin, int ntaps, int stride, const float* row_scale, float alpha, float* dw, float* db,
                  void* workspace, void* stream);
/* srad_op_wgrad with the extents and layout the engines give their layers: dY's columns start at ycol0 of its rows; dw is
 * [n_real][cin_real][taps] and db [n_real] with n_real <= N, cin_real <= Cin (the stored channel counts, multiples of 4, pad
 * columns never written); grp_pad > 0: x's channels are cin_real / grp_real groups of grp_pad stored channels holding grp_real
 * real ones each.  row_scale [B] is per Ho*Wo output rows; a Linear layer (ntaps 1, stride 1) is B samples of Hi*Wi rows. */
int srad_op_wgrad_ex(int precision, const float* dy, int ldy, int ycol0, const float* x, int ldx, int B, int Hi, int Wi, int N,
                     int Cin, int n_real, int cin_real, int grp_real, int grp_pad, int ntaps, int stride, const float* row_scale,
                     float alpha, float* dw, float* db, void* workspace, void* stream);
/* Which weight-gradient kernel a call runs, decided on the host by the functions the launch itself uses; launches nothing and
 * needs no GPU (pointers are compared with NULL and tested for alignment, never dereferenced).  Fails with the launch's own
 * status and message for a problem the launch refuses.
 *   per launch (launches <= 2): family SRAD_WGRAD_FAM_*, FULL (the mask-free body of a shared bf16 launch), grid (workgroups)
 *   per layer (count <= SRAD_WGRAD_PLAN_LAYERS): launch (which one it rides in), ksplit row splits of rows_per rows, tn x tc
 *       64-wide tiles (1 x 1 for the square-tile families), XH / YH operand storage, nblk workgroups from block blk0 of its launch
 *   CONV: the row-gather variant (3x3 or strided);  conv9: NT 16-channel sub-tiles, nchunks 4 x 32 pixel chunks, cpw per
 *       workgroup (ksplit = workgroups, rows_per = cpw * 128);  reduce_tiles: reduce tiles the call queues (0: direct stores)
 *   srad_op_wgrad_plan          : srad_op_wgrad_ex's arguments; dy_bf16 / x_bf16 as srad_op_wgrad_conv9_h stores its operands
 *   srad_op_wgrad_deferred_plan : the SRAD_WQ_WGRAD_DEFERRED steps of a script (below), sent by one srad_wgrad_launch_deferred at
 *       the end - a layer that finds five waiting sends them first, so six layers are two launches */
#define SRAD_WGRAD_FAM_TILE64 0
#define SRAD_WGRAD_FAM_W80 1
#define SRAD_WGRAD_FAM_CONV9 2
#define SRAD_WGRAD_FAM_MULTI 3
#define SRAD_WGRAD_FAM_MULTI_HH 4
#define SRAD_WGRAD_PLAN_LAYERS 6
typedef struct {
  int32_t count, launches, reduce_tiles;
  int32_t precision;         /* 0 fp32 MFMA, 1 bf16 MFMA */
  int32_t family[2], FULL[2], grid[2];
  int32_t CONV, NT, cpw, nchunks;
  int32_t launch[SRAD_WGRAD_PLAN_LAYERS], ksplit[SRAD_WGRAD_PLAN_LAYERS], rows_per[SRAD_WGRAD_PLAN_LAYERS];
  int32_t tn[SRAD_WGRAD_PLAN_LAYERS], tc[SRAD_WGRAD_PLAN_LAYERS], XH[SRAD_WGRAD_PLAN_LAYERS], YH[SRAD_WGRAD_PLAN_LAYERS];
  int32_t blk0[SRAD_WGRAD_PLAN_LAYERS], nblk[SRAD_WGRAD_PLAN_LAYERS];
} srad_wgrad_plan;
int srad_op_wgrad_plan(int precision, const void* dy, int ldy, int ycol0, int dy_bf16, const void* x, int ldx, int x_bf16, int B,
                       int Hi, int Wi, int N, int Cin, int n_real, int cin_real, int grp_real, int grp_pad, int ntaps, int stride,
                       const float* row_scale, srad_wgrad_plan* plan);
/* The 80 -> 80 channel 3x3 convolution (src/drn.py:143-158, RCAB) with bf16 operands, as DRN's bf16 chains issue it in the
 * forward and as the data gradient of the backward: x_h [B*H*W][80] bf16; w [80][80][3][3] fp32; output bf16 (y_h) or fp32 (y);
 * residual operand bf16 (r_h) or fp32 (r) or neither; rmode 0 = add, 2 = multiply by (r > 0 ? 1 : slope) (backward through
 * ReLU / LeakyReLU); pool_part (optional): [B*H*W/128][80] column sums per 128-pixel tile.  H % 4 == 0, W % 32 == 0,
 * B*H*W >= 8192; scratch >= srad_op_gemm_scratch_bytes(SRAD_PRECISION_BF16, 80, 80, 9).  Bit 16 of rmode (tools/c80_stamps.py):
 * the kernel's phase-stamp build, no residual; synchronous, per-phase medians to stderr. */
int srad_op_conv80_h(const void* x_h, const float* w, const float* bias, int act, float slope, const void* r_h, const float* r,
                     int rmode, int B, int H, int W, void* y_h, float* y, float* pool_part, void* scratch, size_t scratch_bytes,
                     void* stream);
/* Its weight / bias gradient from a bf16 dY and a bf16 (x_bf16 = 1) or fp32 X: dw [80][80][3][3], db [80] accumulated;
 * workspace as for srad_op_wgrad.  W % 32 == 0, B*H*W >= 8192. */
int srad_op_wgrad_conv9_h(const void* dy_h, const void* x, int x_bf16, int B, int H, int W, float* dw, float* db, void* workspace,
                          void* stream);
/* The same for a Linear layer, issued as the training step issues it (queued, one deferred launch, reduce).  x_bf16 /
 * dy_bf16 = 1: that operand is a bf16 array (ld in elements; a bf16 dY is taken as already multiplied by its per-sample
 * factor, so row_scale must be null with it, and it needs a bf16 X).  precision SRAD_PREC_BF16 for bf16 operands. */
int srad_op_wgrad_deferred(int precision, const void* dy, int ldy, int dy_bf16, const void* x, int ldx, int x_bf16, int M, int N,
                           int Cin, const float* row_scale, int rps, float alpha, float* dw, float* db, void* workspace,
                           void* stream);
/* split-K workspace of srad_op_wgrad (256-byte aligned scratch, contents irrelevant, reusable by later calls on the
 * same stream) */
size_t srad_op_wgrad_workspace_bytes(void);
/* The split-K queue under a script (tests): `nsteps` steps through ONE queue whose workspace is the first budget_floats floats
 * of `workspace` (budget_floats * 4 <= workspace_bytes), then the deferred launch and a flush.  A step is one of the calls a
 * backward pass makes; its integers and pointers, in order:
 *   SRAD_WQ_WGRAD            i: ldy ldx B Hi Wi N Cin ntaps stride       p: dy x dw db row_scale    (as srad_op_wgrad)
 *   SRAD_WQ_WGRAD_DEFERRED   i: ldy dy_bf16 ldx x_bf16 M N Cin rps       p: dy x dw db row_scale    (as srad_op_wgrad_deferred, not launched)
 *   SRAD_WQ_LAUNCH_DEFERRED  the queued Linear layers as one launch
 *   SRAD_WQ_LN_BWD           i: ldx accumulate rows C                    p: dxn x gamma dres out dgamma dbeta
 *   SRAD_WQ_ATTN_BWD         i: B H W ws shift d heads hdp               p: qkv dout dqkv table dtable  (as srad_op_window_attn_bwd)
 *   SRAD_WQ_FLUSH            reduce what is queued
 * Reports the reduce launches made, counted on the host: *n_reduce, and why[i] (i < why_cap) = the reason of launch i.  The
 * queue flushes itself when a reservation finds the batch (12 items) or the budget full; a reservation that cannot fit even
 * then is an error that names the call that made it, returned at once. */
enum { SRAD_WQ_WGRAD = 1, SRAD_WQ_WGRAD_DEFERRED = 2, SRAD_WQ_LAUNCH_DEFERRED = 3, SRAD_WQ_LN_BWD = 4, SRAD_WQ_ATTN_BWD = 5, SRAD_WQ_FLUSH = 6 };
enum { SRAD_WQ_FLUSH_EXPLICIT = 0, SRAD_WQ_FLUSH_BATCH = 1, SRAD_WQ_FLUSH_WS = 2 };
typedef struct {
  int32_t kind;
  int32_t i[9];
  float alpha;
  const void* p[7];
} srad_wq_step;
int srad_op_wgrad_queue_script(int precision, const srad_wq_step* steps, int nsteps, size_t budget_floats, void* workspace,
                               size_t workspace_bytes, int* n_reduce, int* why, int why_cap, void* stream);
/* srad_wgrad_plan (above) of a script of 1 to SRAD_WGRAD_PLAN_LAYERS SRAD_WQ_WGRAD_DEFERRED steps */
int srad_op_wgrad_deferred_plan(int precision, const srad_wq_step* steps, int nsteps, srad_wgrad_plan* plan);
/* Data gradient dx = (dy . w) * alpha * row_scale (* gelu'(r) if rmode 1, * lrelu'(r) if rmode 2), stride 1:
 * the forward GEMM on the transposed pack of w [N][Cin][taps]; scratch >= srad_op_gemm_scratch_bytes(p, Cin, N, taps) */
int srad_op_dgrad(int precision, const float* dy, int ldy, int B, int H, int W, int N, const float* w, int Cin,
                  int ntaps, const float* r, int ldr, int rmode, float slope, float alpha, const float* row_scale,
                  float* dx, int ldx, void* scratch, size_t scratch_bytes, void* stream);
/* LayerNorm backward: out (+)= dLN(dxn; x, gamma) + dres; dgamma / dbeta accumulated; workspace as for srad_op_wgrad */
int srad_op_layernorm_bwd(const float* dxn, const float* x, int ldx, const float* gamma, const float* dres, float* out,
                          int accumulate, float* dgamma, float* dbeta, int rows, int C, void* workspace, void* stream);
/* Window attention backward (window sizes 1 .. 16, 32 and 64; any other is an error): qkv head-padded as for
 * srad_op_window_attn, dout [T][d], dqkv [T][3d] compact, dtable accumulated; workspace as for srad_op_wgrad.  Windows of 32
 * and 64 take the tiled kernel (fp32 MFMAs in every precision; one partial row of (2 ws - 1)^2 heads floats per window in
 * the workspace, so B (H / ws) (W / ws) such rows must fit in it) */
int srad_op_window_attn_bwd(int precision, const float* qkv, const float* dout, float* dqkv, const float* table,
                            float* dtable, int B, int H, int W, int ws, int shift, int d, int heads, int hdp,
                            void* workspace, void* stream);
/* The all-bf16 form of the same backward, for head dims <= 128 (what the DRCT training step runs): qkv_h [T][3][heads][hp]
 * bf16 with q ALREADY multiplied by head_dim^-0.5 (the forward's MFMA operand), dout_h [T][heads][hp] bf16 (columns at
 * or beyond the head dim are ignored), dqkv_h [T][3 d] bf16 out; hp % 8 == 0; table / dtable fp32. */
int srad_op_window_attn_bwd_h(const void* qkv_h, const void* dout_h, void* dqkv_h, const float* table, float* dtable,
                              int B, int H, int W, int ws, int shift, int d, int heads, int hp, void* workspace, void* stream);
/* Fused backward of the MLP branch of a Swin block (bf16 MFMA; src/drct.py:510, 184-190, 389-396, 300):
 *   [KA > 0] dx2 = aalpha * (dA (.) lrelu'(y_act)) . w_adj          (written; dA (.) lrelu' -> dA_out if given)
 *   dh  = (dx2 . w_fc2) * rs2 * gelu'(hpre);  dx1 = dx2 + LayerNorm'(dh . w_fc1; x1, gamma);  dgamma / dbeta accumulated
 *   [w_proj] dO = (dx1 . w_proj) * rs1
 * Weights in PyTorch layout: w_fc1 [m][d], w_fc2 [d][m], w_adj [KA][d], w_proj [d][d]; rs1 / rs2 per sample (rps rows
 * each) or NULL.  scratch >= srad_op_mlp_bwd_scratch_bytes (256-byte aligned), workspace as for srad_op_wgrad. */
size_t srad_op_mlp_bwd_scratch_bytes(int d, int m, int KA);
int srad_op_mlp_bwd(int M, int d, int m, float* dx2, const float* hpre, const float* x1, const float* gamma,
                    const float* w_fc1, const float* w_fc2, const float* rs2, int rps, float* dh, float* dx1, float* dgamma,
                    float* dbeta, int KA, const float* dA, int ld_dA, const float* y_act, int ld_y, float slope,
                    float aalpha, const float* w_adj, float* dA_out, const float* w_proj, const float* rs1, float* dO,
                    void* scratch, size_t scratch_bytes, void* workspace, void* stream);
/* Data gradient of a Linear + backward of the LayerNorm that fed it (bf16 MFMA): out (+)= dres + LayerNorm'(dY . w; x,
 * gamma), w [K][d] in PyTorch layout, dY [M][K]; dgamma / dbeta accumulated */
size_t srad_op_lin_ln_bwd_scratch_bytes(int K, int d);
int srad_op_lin_ln_bwd(int M, int K, int d, const float* dY, const float* w, const float* x, int ldx, const float* gamma,
                       const float* dres, float* out, int ld_out, int accumulate, float* dgamma, float* dbeta, void* scratch,
                       size_t scratch_bytes, void* workspace, void* stream);

/* DRN's own kernels (csrc/kernels_drn.hip), one entry each, launched through the function the engines call: grid, slices per image,
 * items held in registers (NI) and storage instance are the engines' own.  NHWC fp32 rows unless a *_bf16 flag says the array
 * holds bf16.  The channel-attention entries take C % 4 == 0 in 16 .. 512 (Cr = C / 16 hidden units, w1 [Cr][C], w2 [C][Cr])
 * and nchunk in 1 .. 256 partial rows per image; anything else is an error before any launch.
 *   srad_drn_ca_plan          host only: the slices per image and NI (0 = loop, 5, 10) the two streaming CA kernels get for (hw, C)
 *   srad_op_drn_bicubic       x [B][C][H][W] -> bicubic x scale (align_corners = False, A = -0.75) -> raw [T][4] (optional),
 *                             then sub_mean (mw [C][C], mb [C]) -> y [T][4]; C = 1 | 3, column 3 is 0    (src/drn.py:243-246)
 *   srad_op_drn_affine_to_nchw add_mean: x [B*HW][ldx] -> y [B][C][HW] = mw x + mb                      (src/drn.py:257,266)
 *   srad_op_drn_pool_dot      part[b][k][c] = sum over chunk k's pixels of r (* g if given); r [B*hw][C] fp32 | bf16
 *   srad_op_drn_ca_scale_add  y = r * sigmoid(w2 relu(w1 mean + b1) + b2) + x, mean = (sum of part's rows) / hw; storage r / x / y:
 *                             all fp32, or r bf16 with x and y each fp32 | bf16; x rows ldx elements apart; gate_out, pool_out
 *                             [B][C] optional                                                            (src/drn.py:123-158)
 *   srad_op_drn_ca_apply_bwd  dr = g * gate + d(mean path): part = pool_dot(g, r) rows, pool / gate as the forward left them;
 *                             dr fp32 | bf16
 *   srad_op_drn_ca_bwd        the CA weight / bias gradients ACCUMULATED into dw1, db1, dw2, db2, and dpool [B][C];
 *                             C * C/16 <= 4096
 *   srad_op_drn_affine_bwd    MeanShift backward: dy as NCHW or as [T][4] rows (exactly one), t [T][ldt]; dt [T][4] optional;
 *                             dw [C][C], db [C] ACCUMULATED
 *   srad_op_drn_zero_upsample z [B][2 Ho][2 Wo][C] = dy at the even pixels, 0 elsewhere
 *   srad_op_drn_add_cols      dst[m][0..C) += src[m][0..C)
 *   srad_op_conv_pool         one C -> C 3x3 conv + bias as the forward's second RCAB conv, x, y [B*H*W][C] fp32, w [C][C][3][3];
 *                             *rows = partial rows per image the conv's epilogue wrote to pool_part [B][*rows][C], or 0 when the
 *                             shape does not take that epilogue (pool_part untouched).  x = w = y = NULL: only *rows is answered.
 *                             scratch >= srad_op_gemm_scratch_bytes(precision, C, C, 9), 256-byte aligned */
int srad_drn_ca_plan(int hw, int C, int* slices, int* ni);
int srad_op_drn_bicubic(const float* x, int B, int C, int H, int W, int scale, const float* mw, const float* mb, float* y, float* raw,
                        void* stream);
int srad_op_drn_affine_to_nchw(const float* x, int ldx, int B, int C, int HW, const float* mw, const float* mb, float* y, void* stream);
int srad_op_drn_pool_dot(const float* g, const void* r, int r_bf16, int B, int hw, int C, int nchunk, float* part, void* stream);
int srad_op_drn_ca_scale_add(const float* part, int nchunk, int B, int hw, int C, const float* w1, const float* b1, const float* w2,
                             const float* b2, const void* r, int r_bf16, const void* x, int x_bf16, int ldx, void* y, int y_bf16,
                             float* gate_out, float* pool_out, void* stream);
int srad_op_drn_ca_apply_bwd(const float* g, const float* gate, const float* part, int nchunk, const float* pool, int B, int hw, int C,
                             const float* w1, const float* b1, const float* w2, void* dr, int dr_bf16, void* stream);
int srad_op_drn_ca_bwd(const float* part, int nchunk, const float* pool, const float* gate, int B, int hw, int C, const float* w1,
                       const float* b1, const float* w2, float* dw1, float* db1, float* dw2, float* db2, float* dpool, void* stream);
int srad_op_drn_affine_bwd(const float* dy_nchw, const float* dy_rows, const float* t, int ldt, float* dt, int B, int C, int HW,
                           const float* w, float* dw, float* db, void* stream);
int srad_op_drn_zero_upsample(const float* dy, float* z, int B, int Ho, int Wo, int C, void* stream);
int srad_op_drn_add_cols(const float* src, int ld_src, float* dst, int ld_dst, int64_t rows, int C, void* stream);
int srad_op_conv_pool(int precision, const float* x, const float* w, const float* bias, int B, int H, int W, int C, float* y,
                      float* pool_part, int* rows, void* scratch, size_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------ diagnostics
 * Reference paths for tests.  The library picks kernel paths from shape and precision alone; these process-wide overrides
 * (all off at load) force the path a test compares the default one against:
 *   SRAD_PATH_UNFUSED_BLOCKS    DRCT Swin blocks as separate launches instead of the fused block kernels (the forward reads
 *                               it at srad_drct_create, the backward at every srad_drct_backward)
 *   SRAD_PATH_QKV_VIA_GEMM      64 x 64 windows: LayerNorm1 + qkv through the tiled GEMM's epilogue instead of one launch
 *   SRAD_PATH_ATTN_F32_IN       64 x 64 windows: the attention stages fp32 q | k | v itself
 *   SRAD_PATH_UPCONV_ONE_GEMM   DRN's Upsampler conv as one tiled GEMM instead of four 80-channel convolutions
 * srad_set_path_override returns 0, or non-zero for an unknown path; srad_get_path_override returns 0 / 1, or -1 for an
 * unknown path. */
enum { SRAD_PATH_UNFUSED_BLOCKS = 0, SRAD_PATH_QKV_VIA_GEMM = 1, SRAD_PATH_ATTN_F32_IN = 2, SRAD_PATH_UPCONV_ONE_GEMM = 3,
       SRAD_PATH_COUNT = 4 };
/* Launch-plan overrides: the same two calls, ids from SRAD_PATH_PLAN_FIRST (the ids between SRAD_PATH_COUNT and it stay unknown).
 *   SRAD_PATH_BLOCK_TWO_LAUNCHES  DRCT forward: a Swin block as the qkv_attn + mlp_block pair where the one-launch
 *                                 swin_block kernel would be chosen (read at every forward that records launches)
 *   SRAD_PATH_TAIL_CHAIN          DRCT bf16 forward: the Upsample convolutions, conv_last and the layout change as their own
 *                                 launches where the folded output end (srad_op_tail_fold) would run (read at every forward) */
enum { SRAD_PATH_PLAN_FIRST = 16, SRAD_PATH_BLOCK_TWO_LAUNCHES = 16, SRAD_PATH_TAIL_CHAIN = 17, SRAD_PATH_END = 18 };
/* ... continued in a second range, so that the ids above and their end stay what callers know (18 .. 31 stay unknown):
 *   SRAD_PATH_ENDS_CHAIN          DRCT bf16 forward: the final LayerNorm, conv_after_body and conv_before_upsample as their
 *                                 own launches where the body-end launch (srad_op_drct_body_end) would run (read at every
 *                                 forward) */
enum { SRAD_PATH_PLAN2_FIRST = 32, SRAD_PATH_ENDS_CHAIN = 32, SRAD_PATH_PLAN2_END = 33 };
/* ... and in a third range (33 .. 47 stay unknown):
 *   SRAD_PATH_FC2_CHAIN           DRCT bf16 inference forward: a Swin block's fc2 and the adjust conv as the two GEMMs of the
 *                                 chain where the folded second half (srad_op_swin_block_folded, srad_op_mlp_block_folded)
 *                                 would run (read at every forward) */
enum { SRAD_PATH_PLAN3_FIRST = 48, SRAD_PATH_FC2_CHAIN = 48, SRAD_PATH_PLAN3_END = 49 };
int srad_set_path_override(int path, int on);
int srad_get_path_override(int path);
/* Per-kernel-class device timing with HIP events on the launch stream (bench.py's roofline numbers). */
int srad_prof_enable(int on);
int srad_prof_num_classes(void);
const char* srad_prof_class_name(int cls);
int srad_prof_collect(int64_t* launches, double* ms, double* flops, double* bytes);
/* Back-to-back launches of one kernel, average microseconds per launch (tools/gemm_bench.py). */
int srad_bench_gemm(int precision, const float* x, int ldx, int B, int Hi, int Wi, int Cin, const float* w, int N,
                    int ntaps, int stride, const float* bias, const float* ln_g, const float* ln_b, int act,
                    const float* r, int ldr, float* y, int ldy, int hsplit_hd, int hsplit_hdp, void* scratch,
                    size_t scratch_bytes, int iters, float* us_out, void* stream);
int srad_bench_mlp_block(int M, int d, int m, int no, const void* attn /* bf16 [M][320] */, const float* shortcut, float* y,
                         const float* w_fp32, void* scratch, size_t scratch_bytes, int dbg, int iters, float* us_out,
                         void* stream);
int srad_bench_window_attn(int precision, const float* qkv, float* out, const float* table, int B, int H, int W, int ws,
                           int shift, int d, int heads, int hdp, int iters, float* us_out, void* stream);
int srad_bench_qkv_attn(const float* x, int ldx, int B, int H, int W, int shift, int d, int heads, const float* w_fp32,
                        void* out /* written as bf16 [B*H*W][d] */, void* scratch, size_t scratch_bytes, int iters, float* us_out,
                        void* stream);
/* tools/swin_block_bench.py: the one-launch Swin block on synthetic operands (x, y: [B*H*W][320] fp32; y also takes the
 * output: columns [d, d + no), or [0, no) where those do not fit), microseconds per launch, back-to-back launches.  Bit 17 of
 * `shift` selects the folded second half. */
int srad_bench_swin_block(const float* x, int B, int H, int W, int shift, int d, int heads, int m, int no, const float* w_fp32,
                          float* y, void* scratch, size_t scratch_bytes, int iters, float* us_out, void* stream);
/* tools/wgrad_bench.py: one Swin block's five weight gradients as the training step issues them (one deferred launch +
 * the reduce), `iters` times; storage bit 0 / 1: the X / dY operands are bf16. */
int srad_bench_wgrad_block(int M, int d, int hidden, int KA, int storage, const void* xbuf, const void* ybuf, float* dw,
                           void* workspace, int iters, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SRAD_H */
