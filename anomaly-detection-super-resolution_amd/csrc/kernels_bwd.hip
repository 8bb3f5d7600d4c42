// kernels_bwd.hip - backward kernels of the training step on gfx950 (reference src/trainer.py:152-222:
// loss.backward() through src/drct.py / src/drn.py; the arithmetic is PyTorch autograd's for Linear,
// conv2d, LayerNorm, GELU / LeakyReLU and PixelShuffle; the attention backward is kernels_attn_bwd.hip).
//
//   ln_bwd_kernel           dx, dgamma, dbeta    one wave per row, statistics recomputed; dgamma / dbeta partial rows go
//                                                to the split-K queue (srad_wgrad_queue_ln_partials)
//   dact_kernel, unshuffle_kernel, copy_cols_kernel   activation backward, pixel un-shuffle, column copies
//   l1_grad_kernel          the L1 loss's gradient seed
//   adam_kernel, adam_dev_kernel, set4_kernel         torch.optim.Adam on flat buffers, its per-step scalars
//   adam_ema_kernel, adam_ema_dev_kernel              the same step, also keeping the weights' exponential moving average
//   sumsq_partials_kernel, grad_guard_finalize_kernel the gradient's global L2 norm in fp64 and the apply / clip / skip decision
//   adam_guarded_kernel, adam_ema_guarded_kernel      the two device-scalar steps behind that decision
//
// The weight gradients and the split-K queue's launches are kernels_wgrad.hip.  Data gradients (dX = dY W) are not here
// either: they are the forward GEMM of kernels_gemm.hip run on the transposed packed weight (srad_launch_pack_weight_transposed).
#include "srad_common.h"
#include <type_traits>
#include <algorithm>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

namespace {

static inline int grid_for(size_t total) {
  size_t b = (total + 255) / 256;
  return (int)(b > 4096 ? 4096 : (b < 1 ? 1 : b));
}

constexpr int LNB_RPW = 16;                  // LayerNorm backward: rows per workgroup
constexpr int LNB_CP = SRAD_LNB_CP;          // columns of a dgamma | dbeta partial row (channel counts <= 320)

// ------------------------------------------------------------------------------------------
// LayerNorm backward, one wave per row, RPW rows per 16-wave workgroup (two rows per wave, four waves per SIMD
// to cover the load latency).  Mean / rstd are recomputed exactly as the forward kernel does; dgamma / dbeta
// partials live in registers across the wave's rows, are summed over the waves in LDS and left in the split-K
// workspace for wgrad_reduce_kernel.
// ------------------------------------------------------------------------------------------

// HAS_RES / ACC are template flags: a load behind a run-time test is waited for before the next one issues.
// One wave per row, 32 rows per 4-wave workgroup.
// Lane l owns channels [4 l, 4 l + 4) and [256 + 4 l, 256 + 4 l + 4): 16-byte loads, two per tensor per row.
template <bool HAS_RES, bool ACC, int J4>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const LnBwdParams p, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float red[4][2][512];      // per wave: dgamma | dbeta partial rows
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const f32x4 z4 = f32x4{0.f, 0.f, 0.f, 0.f};
  int cofs[J4];
  bool cok[J4];
  f32x4 gam[J4], dg[J4], db[J4];
#pragma unroll
  for (int j = 0; j < J4; ++j) {
    const int c = 4 * lane + 256 * j;
    cok[j] = c < p.C;                          // C % 4 == 0: a float4 is all in or all out
    cofs[j] = min(c, p.C - 4);
    gam[j] = *reinterpret_cast<const f32x4*>(p.gamma + cofs[j]);
    dg[j] = z4; db[j] = z4;
  }
  const float invC = 1.0f / (float)p.C;
  const int r_end = min(p.rows, (int)(blockIdx.x + 1) * LNB_RPW);
  // two rows per wave and trip: their loads are in flight together and the four reduction chains interleave
  for (int row0 = blockIdx.x * LNB_RPW + wave; row0 < r_end; row0 += 8) {
    f32x4 xv[2][J4], dy[2][J4], rv[2][J4], ov[2][J4];
    int rows_[2];
    bool rok[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      rok[u] = row0 + 4 * u < r_end;
      rows_[u] = rok[u] ? row0 + 4 * u : row0;
#pragma unroll
      for (int j = 0; j < J4; ++j) {
        xv[u][j] = *reinterpret_cast<const f32x4*>(p.x + (size_t)rows_[u] * p.ldx + cofs[j]);
        dy[u][j] = *reinterpret_cast<const f32x4*>(p.dxn + (size_t)rows_[u] * p.ld_dxn + cofs[j]);
        rv[u][j] = z4; ov[u][j] = z4;
        if constexpr (HAS_RES) rv[u][j] = *reinterpret_cast<const f32x4*>(p.dres + (size_t)rows_[u] * p.ld_dres + cofs[j]);
        if constexpr (ACC) ov[u][j] = *reinterpret_cast<const f32x4*>(p.out + (size_t)rows_[u] * p.ld_out + cofs[j]);
      }
    }
    float s[2], v[2], s1[2], s2[2], rstd[2];
    f32x4 xh[2][J4], gy[2][J4];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      s[u] = 0.f;
#pragma unroll
      for (int j = 0; j < J4; ++j) {
        xv[u][j] = cok[j] ? xv[u][j] : z4;
        dy[u][j] = cok[j] && rok[u] ? dy[u][j] : z4;
        s[u] += (xv[u][j][0] + xv[u][j][1]) + (xv[u][j][2] + xv[u][j][3]);
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) s[u] = srad_wave_sum(s[u]) * invC;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      v[u] = 0.f;
#pragma unroll
      for (int j = 0; j < J4; ++j) {
        xh[u][j] = cok[j] ? xv[u][j] - s[u] : z4;
        v[u] += (xh[u][j][0] * xh[u][j][0] + xh[u][j][1] * xh[u][j][1]) + (xh[u][j][2] * xh[u][j][2] + xh[u][j][3] * xh[u][j][3]);
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) { v[u] = srad_wave_sum(v[u]); rstd[u] = rsqrtf(v[u] * invC + p.eps); }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      s1[u] = 0.f; s2[u] = 0.f;
#pragma unroll
      for (int j = 0; j < J4; ++j) {
        xh[u][j] = xh[u][j] * rstd[u];
        gy[u][j] = dy[u][j] * gam[j];
        const f32x4 t = gy[u][j] * xh[u][j];
        s1[u] += (gy[u][j][0] + gy[u][j][1]) + (gy[u][j][2] + gy[u][j][3]);
        s2[u] += (t[0] + t[1]) + (t[2] + t[3]);
        dg[j] += dy[u][j] * xh[u][j];
        db[j] += dy[u][j];
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) { s1[u] = srad_wave_sum(s1[u]) * invC; s2[u] = srad_wave_sum(s2[u]) * invC; }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
#pragma unroll
      for (int j = 0; j < J4; ++j) {
        const f32x4 o4 = (gy[u][j] - s1[u] - xh[u][j] * s2[u]) * rstd[u] + rv[u][j] + ov[u][j];
        if (cok[j] && rok[u]) *reinterpret_cast<f32x4*>(p.out + (size_t)rows_[u] * p.ld_out + 4 * lane + 256 * j) = o4;
      }
    }
  }
#pragma unroll
  for (int j = J4; j < 2; ++j) {
    *reinterpret_cast<f32x4*>(&red[wave][0][4 * lane + 256 * j]) = z4;
    *reinterpret_cast<f32x4*>(&red[wave][1][4 * lane + 256 * j]) = z4;
  }
  // LDS float atomics cost ~13 us here (measured); plain 16-byte stores per wave, then a 4-way sum
#pragma unroll
  for (int j = 0; j < J4; ++j) {
    *reinterpret_cast<f32x4*>(&red[wave][0][4 * lane + 256 * j]) = dg[j];
    *reinterpret_cast<f32x4*>(&red[wave][1][4 * lane + 256 * j]) = db[j];
  }
  __syncthreads();
  // per-workgroup column sums -> workspace row [dgamma LNB_CP | dbeta LNB_CP]; wgrad_reduce_kernel adds them up
  float* row = part + (size_t)blockIdx.x * (2 * LNB_CP);
  for (int i = tid; i < 2 * LNB_CP; i += 256) {
    const int which = i >= LNB_CP ? 1 : 0, c = i - which * LNB_CP;
    row[i] = (red[0][which][c] + red[1][which][c]) + (red[2][which][c] + red[3][which][c]);
  }
}

// ------------------------------------------------------------------------------------------ elementwise
__global__ void dact_kernel(const float* __restrict__ dy, int ld_dy, const float* __restrict__ y, int ld_y,
                            float* __restrict__ out, int ld_out, int rows, int C, float slope) {
  const size_t total = (size_t)rows * C;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t m = i / C;
    const int c = (int)(i - m * C);
    out[m * ld_out + c] = dy[m * ld_dy + c] * (y[m * ld_y + c] > 0.f ? 1.f : slope);
  }
}

__global__ void unshuffle_kernel(const float* __restrict__ src, float* __restrict__ dst, int B, int H, int W, int F) {
  const size_t total = (size_t)B * H * W * 4 * F;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    // iterate in SOURCE order (coalesced reads): i = ((b*2H + y2)*2W + x2)*F + c
    const int c = (int)(i % F);
    size_t pix = i / F;
    const int x2 = (int)(pix % (2 * W)); pix /= 2 * W;
    const int y2 = (int)(pix % (2 * H));
    const int b = (int)(pix / (2 * H));
    const int n = c * 4 + (y2 & 1) * 2 + (x2 & 1);
    dst[(((size_t)b * H + (y2 >> 1)) * W + (x2 >> 1)) * 4 * F + n] = src[i];
  }
}

__global__ void copy_cols_kernel(const float* __restrict__ src, int ld_src, float* __restrict__ dst, int ld_dst, int rows, int C) {
  const size_t total = (size_t)rows * ld_dst;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t m = i / ld_dst;
    const int c = (int)(i - m * ld_dst);
    dst[i] = c < C ? src[m * ld_src + c] : 0.f;
  }
}

__global__ void l1_grad_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, size_t n, float scale) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float d = a[i] - b[i];
    out[i] = d > 0.f ? scale : (d < 0.f ? -scale : 0.f);
  }
}

// torch.optim.Adam single-tensor arithmetic (torch/optim/adam.py _single_tensor_adam, amsgrad off, maximize off)
// EMA: the same pass also keeps the exponential moving average of the weights, ema = fl(fl(d * ema) + fl(omd * p')) with p' the
// parameter just stored - three separately rounded fp32 operations (no contraction into an fma), so the average is defined
// bit for bit by its previous value and the new parameter (BasicSR's ema.mul_(decay).add_(p, alpha=1 - decay)).
// HIP's __fmul_rn / __fadd_rn are plain * and + that the compiler may still contract; the pragma is what keeps them apart.
__device__ __forceinline__ float ema_update(float d, float e, float omd, float pn) {
#pragma clang fp contract(off)
  const float a = d * e;
  const float b = omd * pn;
  return a + b;
}
template <bool EMA>
__device__ __forceinline__ void adam_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                          float* __restrict__ v, size_t n, float lr, float b1, float b2, float eps, float wd,
                                          float bc1, float bc2_sqrt, float gs, float* __restrict__ ema = nullptr, float d = 0.f,
                                          float omd = 0.f) {
  const float step_size = lr / bc1;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    float grad = g[i] * gs;
    const float w = p[i];
    if (wd != 0.f) grad = grad + wd * w;
    const float mi = m[i] + (grad - m[i]) * (1.f - b1);          // exp_avg.lerp_(grad, 1 - beta1)
    const float vi = v[i] * b2 + (1.f - b2) * grad * grad;       // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
    m[i] = mi; v[i] = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    p[i] = w - step_size * (mi / denom);
    if constexpr (EMA) ema[i] = ema_update(d, ema[i], omd, p[i]);     // p[i]: the value just stored
  }
}
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                            size_t n, float lr, float b1, float b2, float eps, float wd, float bc1, float bc2_sqrt, float gs) {
  adam_body<false>(p, g, m, v, n, lr, b1, b2, eps, wd, bc1, bc2_sqrt, gs);
}
__global__ void adam_ema_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                float* __restrict__ ema, size_t n, float lr, float b1, float b2, float eps, float wd, float bc1,
                                float bc2_sqrt, float gs, float d, float omd) {
  adam_body<true>(p, g, m, v, n, lr, b1, b2, eps, wd, bc1, bc2_sqrt, gs, ema, d, omd);
}
// the same step with the per-step scalars [lr, 1 - beta1^t, sqrt(1 - beta2^t), grad_scale] read from device memory, so
// that a captured hipGraph of a whole training step can be replayed with a new step count / learning rate
__global__ void adam_dev_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                size_t n, float b1, float b2, float eps, float wd, const float* __restrict__ hyper) {
  adam_body<false>(p, g, m, v, n, hyper[0], b1, b2, eps, wd, hyper[1], hyper[2], hyper[3]);
}
__global__ void adam_ema_dev_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                    float* __restrict__ v, float* __restrict__ ema, size_t n, float b1, float b2, float eps,
                                    float wd, const float* __restrict__ hyper, float d, float omd) {
  adam_body<true>(p, g, m, v, n, hyper[0], b1, b2, eps, wd, hyper[1], hyper[2], hyper[3], ema, d, omd);
}

// ------------------------------------------------------------------------------------------
// Guarded step (DESIGN.md "Guarded step"): the gradient's global L2 norm, one device-side decision (apply, scale or skip),
// and the Adam step that obeys it.  Three launches, no atomics, no host read: the whole thing replays inside a hipGraph.
// ------------------------------------------------------------------------------------------

// all 64 lanes' values summed in a fixed tree; lane 0 holds the result
__device__ __forceinline__ double wave_sum_f64(double s) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  return s;
}
// the workgroup's four wave sums added in wave order; thread 0 holds the result
__device__ __forceinline__ double block_sum_f64(double s, double* red) {
  s = wave_sum_f64(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}
__device__ __forceinline__ double sq4_f64(const f32x4 x, double a) {
  a = fma((double)x[0], (double)x[0], a);      // the fp64 square of an fp32 value is exact: no overflow, one rounding per add
  a = fma((double)x[1], (double)x[1], a);
  a = fma((double)x[2], (double)x[2], a);
  return fma((double)x[3], (double)x[3], a);
}

// part[blockIdx.x] = this workgroup's share of sum g[i]^2, squares and sums in fp64.  g needs only float alignment: the up
// to three floats in front of the first 16-byte boundary and the up to three behind the last whole float4 are read one by
// one, everything between as 16-byte loads, four in flight per thread.  Which thread adds which element in which order
// depends on n, the grid (a function of n) and g's offset from a 16-byte boundary alone, so the sum's bits repeat.
__global__ __launch_bounds__(256) void sumsq_partials_kernel(const float* __restrict__ g, size_t n, double* __restrict__ part) {
  __shared__ double red[4];
  const size_t tid = blockIdx.x * (size_t)256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
  size_t head = ((16 - ((uintptr_t)g & 15)) & 15) >> 2;
  if (head > n) head = n;
  const f32x4* __restrict__ g4 = reinterpret_cast<const f32x4*>(g + head);
  const size_t nvec = (n - head) >> 2, tail0 = head + 4 * nvec;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  size_t i = tid;
  for (; i + 3 * stride < nvec; i += 4 * stride) {
    const f32x4 x0 = g4[i], x1 = g4[i + stride], x2 = g4[i + 2 * stride], x3 = g4[i + 3 * stride];
    a0 = sq4_f64(x0, a0); a1 = sq4_f64(x1, a1); a2 = sq4_f64(x2, a2); a3 = sq4_f64(x3, a3);
  }
  for (; i < nvec; i += stride) a0 = sq4_f64(g4[i], a0);
  if (tid < head) { const double x = (double)g[tid]; a1 = fma(x, x, a1); }
  if (tid < n - tail0) { const double x = (double)g[tail0 + tid]; a2 = fma(x, x, a2); }
  const double s = block_sum_f64((a0 + a1) + (a2 + a3), red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__device__ __forceinline__ double ipow_f64(double b, long long e) {      // b^e by squaring, e >= 0
  double r = 1.0;
  for (; e; e >>= 1, b *= b)
    if (e & 1) r *= b;
  return r;
}

// One workgroup: thread t adds the slots [t c, (t + 1) c), c = ceil(n_slots / 256), in index order, the 256 sums go through
// the same fixed tree as above; thread 0 then decides and writes the state and the record Adam reads.
__global__ __launch_bounds__(256) void grad_guard_finalize_kernel(const double* __restrict__ part, int n_slots,
                                                                  SradGuardState* __restrict__ st, SradGuardRecord* __restrict__ rec,
                                                                  const float* __restrict__ hyper_in, float b1, float b2,
                                                                  double max_norm) {
  __shared__ double red[4];
  const int c = (n_slots + 255) / 256, lo = min((int)threadIdx.x * c, n_slots), hi = min(lo + c, n_slots);
  double s = 0.0;
  for (int j = lo; j < hi; ++j) s += part[j];
  s = block_sum_f64(s, red);
  if (threadIdx.x != 0) return;
  const float lr = hyper_in[0];
  const double gs = (double)hyper_in[3];
  const double norm = gs * sqrt(s);                       // non-finite exactly when some gradient element is
  st->last_norm = norm;
  if (!isfinite(norm)) {
    st->skipped += 1;
    rec->hyper[0] = lr; rec->hyper[1] = 1.f; rec->hyper[2] = 1.f; rec->hyper[3] = 0.f;
    rec->apply = 0;
    return;
  }
  const double coef = fmin(1.0, max_norm / (norm + 1e-6));     // clip_grad_norm_; max_norm = +inf gives exactly 1
  if (coef < 1.0) st->clipped += 1;
  const long long t = st->applied + 1;                    // bias correction counts the steps that were applied
  st->applied = t;
  rec->hyper[0] = lr;
  rec->hyper[1] = (float)(1.0 - ipow_f64((double)b1, t));
  rec->hyper[2] = (float)sqrt(1.0 - ipow_f64((double)b2, t));
  rec->hyper[3] = (float)(gs * coef);
  rec->apply = 1;
}

// adam_dev_kernel / adam_ema_dev_kernel behind the guard's record: a skipped step returns before any access to the five
// buffers; an applied one is the same adam_body on the record's four scalars
__global__ void adam_guarded_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                    size_t n, float b1, float b2, float eps, float wd, const SradGuardRecord* __restrict__ rec) {
  if (rec->apply == 0) return;
  adam_body<false>(p, g, m, v, n, rec->hyper[0], b1, b2, eps, wd, rec->hyper[1], rec->hyper[2], rec->hyper[3]);
}
__global__ void adam_ema_guarded_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                        float* __restrict__ v, float* __restrict__ ema, size_t n, float b1, float b2, float eps,
                                        float wd, const SradGuardRecord* __restrict__ rec, float d, float omd) {
  if (rec->apply == 0) return;
  adam_body<true>(p, g, m, v, n, rec->hyper[0], b1, b2, eps, wd, rec->hyper[1], rec->hyper[2], rec->hyper[3], ema, d, omd);
}

}  // namespace


int srad_launch_ln_bwd(const LnBwdParams& p, WgradQueue& q, hipStream_t stream) {
  SRAD_REQUIRE(p.rows > 0 && p.C >= 4 && p.C <= LNB_CP && (p.C & 3) == 0, "ln_bwd: channel count %d unsupported (4..%d, multiple of 4)", p.C, LNB_CP);
  SRAD_REQUIRE(((p.ldx | p.ld_dxn | p.ld_out | (p.dres ? p.ld_dres : 0)) & 3) == 0 &&
                   (((uintptr_t)p.x | (uintptr_t)p.dxn | (uintptr_t)p.out | (uintptr_t)p.dres | (uintptr_t)p.gamma) & 15) == 0,
               "ln_bwd: rows must be 16-byte aligned (strides multiples of 4 floats)");
  SRAD_REQUIRE(p.dxn && p.x && p.gamma && p.out, "ln_bwd: null argument");
  const int nwg = (p.rows + LNB_RPW - 1) / LNB_RPW;
  float* part = nullptr;
  SRAD_TRY(srad_wgrad_queue_ln_partials(q, p.dgamma, p.dbeta, p.C, nwg, stream, &part));
  SradProfScope prof(stream, SRAD_K_LN_BWD, 16.0 * p.rows * p.C, 4.0 * p.rows * p.C * (3 + (p.dres ? 1 : 0) + (p.accumulate ? 1 : 0)));
  auto go = [&](auto j4) {
    constexpr int J = decltype(j4)::value;
    if (p.dres && p.accumulate) hipLaunchKernelGGL((ln_bwd_kernel<true, true, J>), dim3(nwg), dim3(256), 0, stream, p, part);
    else if (p.dres) hipLaunchKernelGGL((ln_bwd_kernel<true, false, J>), dim3(nwg), dim3(256), 0, stream, p, part);
    else if (p.accumulate) hipLaunchKernelGGL((ln_bwd_kernel<false, true, J>), dim3(nwg), dim3(256), 0, stream, p, part);
    else hipLaunchKernelGGL((ln_bwd_kernel<false, false, J>), dim3(nwg), dim3(256), 0, stream, p, part);
  };
  if (p.C <= 256) go(std::integral_constant<int, 1>{});
  else go(std::integral_constant<int, 2>{});
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

int srad_launch_dact(const float* dy, int ld_dy, const float* y, int ld_y, float* out, int ld_out, int rows, int C,
                     float slope, hipStream_t stream) {
  const size_t total = (size_t)rows * C;
  SradProfScope prof(stream, SRAD_K_MISC, 1.0 * total, 12.0 * total);
  hipLaunchKernelGGL(dact_kernel, dim3(grid_for(total)), dim3(256), 0, stream, dy, ld_dy, y, ld_y, out, ld_out, rows, C, slope);
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

int srad_launch_unshuffle(const float* src, float* dst, int B, int H, int W, int F, hipStream_t stream) {
  const size_t total = (size_t)B * H * W * 4 * F;
  SradProfScope prof(stream, SRAD_K_LAYOUT, 0.0, 8.0 * total);
  hipLaunchKernelGGL(unshuffle_kernel, dim3(grid_for(total)), dim3(256), 0, stream, src, dst, B, H, W, F);
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

int srad_launch_copy_cols(const float* src, int ld_src, float* dst, int ld_dst, int rows, int C, hipStream_t stream) {
  const size_t total = (size_t)rows * ld_dst;
  SradProfScope prof(stream, SRAD_K_LAYOUT, 0.0, 4.0 * total + 4.0 * rows * C);
  hipLaunchKernelGGL(copy_cols_kernel, dim3(grid_for(total)), dim3(256), 0, stream, src, ld_src, dst, ld_dst, rows, C);
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

int srad_launch_l1_grad(const float* a, const float* b, float* out, size_t n, float scale, hipStream_t stream) {
  SradProfScope prof(stream, SRAD_K_OPTIM, 2.0 * n, 12.0 * n);
  hipLaunchKernelGGL(l1_grad_kernel, dim3(grid_for(n)), dim3(256), 0, stream, a, b, out, n, scale);
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

int srad_launch_adam(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2,
                     float eps, float weight_decay, int step, float grad_scale, hipStream_t stream) {
  SRAD_REQUIRE(step >= 1, "adam: step counts from 1 (got %d)", step);
  const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
  SradProfScope prof(stream, SRAD_K_OPTIM, 12.0 * n, 28.0 * n);
  hipLaunchKernelGGL(adam_kernel, dim3(grid_for(n)), dim3(256), 0, stream, p, g, m, v, n, lr, beta1, beta2, eps,
                     weight_decay, (float)bc1, (float)sqrt(bc2), grad_scale);
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

int srad_launch_adam_dev(float* p, const float* g, float* m, float* v, size_t n, float beta1, float beta2, float eps,
                         float weight_decay, const float* hyper, hipStream_t stream) {
  SradProfScope prof(stream, SRAD_K_OPTIM, 12.0 * n, 28.0 * n);
  hipLaunchKernelGGL(adam_dev_kernel, dim3(grid_for(n)), dim3(256), 0, stream, p, g, m, v, n, beta1, beta2, eps, weight_decay, hyper);
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

// what both EMA launches refuse before anything is enqueued; *omd = (float)(1 - (double)decay), the weight of the new parameter
static int adam_ema_check(const char* what, const float* p, const float* g, const float* m, const float* v, const float* ema,
                          size_t n, float decay, float* omd) {
  SRAD_REQUIRE(ema, "%s: null ema", what);
  SRAD_REQUIRE(decay >= 0.f && decay < 1.f, "%s: ema_decay must be in [0, 1) (got %g)", what, (double)decay);     // NaN too
  SRAD_REQUIRE(!srad_ranges_overlap(ema, n, p, n) && !srad_ranges_overlap(ema, n, g, n) && !srad_ranges_overlap(ema, n, m, n) &&
                   !srad_ranges_overlap(ema, n, v, n),
               "%s: ema overlaps another buffer", what);
  *omd = (float)(1.0 - (double)decay);
  return SRAD_OK;
}

int srad_launch_adam_ema(float* p, const float* g, float* m, float* v, float* ema, size_t n, float lr, float beta1, float beta2,
                         float eps, float weight_decay, int step, float grad_scale, float ema_decay, hipStream_t stream) {
  SRAD_REQUIRE(step >= 1, "adam_ema_step: step counts from 1 (got %d)", step);
  float omd;
  SRAD_TRY(adam_ema_check("adam_ema_step", p, g, m, v, ema, n, ema_decay, &omd));
  const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
  SradProfScope prof(stream, SRAD_K_OPTIM, 15.0 * n, 36.0 * n);
  hipLaunchKernelGGL(adam_ema_kernel, dim3(grid_for(n)), dim3(256), 0, stream, p, g, m, v, ema, n, lr, beta1, beta2, eps,
                     weight_decay, (float)bc1, (float)sqrt(bc2), grad_scale, ema_decay, omd);
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

int srad_launch_adam_ema_dev(float* p, const float* g, float* m, float* v, float* ema, size_t n, float beta1, float beta2,
                             float eps, float weight_decay, float ema_decay, const float* hyper, hipStream_t stream) {
  float omd;
  SRAD_TRY(adam_ema_check("adam_ema_step_dev", p, g, m, v, ema, n, ema_decay, &omd));
  SradProfScope prof(stream, SRAD_K_OPTIM, 15.0 * n, 36.0 * n);
  hipLaunchKernelGGL(adam_ema_dev_kernel, dim3(grid_for(n)), dim3(256), 0, stream, p, g, m, v, ema, n, beta1, beta2, eps,
                     weight_decay, hyper, ema_decay, omd);
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

// ------------------------------------------------------------------------------------------
// Guarded step: workspace = [SradGuardState | SradGuardRecord | fp64 partial slots]
// ------------------------------------------------------------------------------------------
int srad_guard_slots_for(size_t n) { return grid_for(n); }

static inline double* guard_partials(void* ws) { return reinterpret_cast<double*>((char*)ws + SRAD_GUARD_HEADER_BYTES); }
static inline SradGuardRecord* guard_record(const void* ws) {
  return reinterpret_cast<SradGuardRecord*>((char*)const_cast<void*>(ws) + sizeof(SradGuardState));
}
// does the byte range [ws, ws + bytes) touch q[0..nq)?
static inline bool guard_overlaps(const void* ws, size_t bytes, const float* q, size_t nq) {
  const uintptr_t a = (uintptr_t)ws, b = (uintptr_t)q;
  return a < b + nq * sizeof(float) && b < a + bytes;
}

int srad_launch_grad_guard_partials(const float* g, size_t n, void* ws, size_t ws_bytes, int first_slot, hipStream_t stream) {
  SRAD_REQUIRE(((uintptr_t)ws & 15) == 0 && ((uintptr_t)g & 3) == 0, "grad_guard_partials: the workspace must be 16-byte aligned, the gradients float aligned");
  SRAD_REQUIRE(first_slot >= 0, "grad_guard_partials: first_slot %d is negative", first_slot);
  const int slots = grid_for(n);
  const size_t need = SRAD_GUARD_HEADER_BYTES + ((size_t)first_slot + slots) * sizeof(double);
  SRAD_REQUIRE(ws_bytes >= need, "grad_guard_partials: workspace too small (%zu bytes, slots %d..%d need %zu)", ws_bytes, first_slot,
               first_slot + slots - 1, need);
  SRAD_REQUIRE(!guard_overlaps(ws, ws_bytes, g, n), "grad_guard_partials: the workspace overlaps the gradients");
  SradProfScope prof(stream, SRAD_K_OPTIM, 2.0 * n, 4.0 * n);
  hipLaunchKernelGGL(sumsq_partials_kernel, dim3(slots), dim3(256), 0, stream, g, n, guard_partials(ws) + first_slot);
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

int srad_launch_grad_guard_finalize(void* ws, size_t ws_bytes, int n_slots, const float* hyper, float beta1, float beta2,
                                    double max_norm, hipStream_t stream) {
  SRAD_REQUIRE(((uintptr_t)ws & 15) == 0, "grad_guard_finalize: the workspace must be 16-byte aligned");
  SRAD_REQUIRE(n_slots >= 1, "grad_guard_finalize: n_slots must be positive (got %d)", n_slots);
  SRAD_REQUIRE(max_norm > 0.0, "grad_guard_finalize: max_norm must be > 0 (got %g; +inf = no clipping)", max_norm);     // NaN too
  const size_t need = SRAD_GUARD_HEADER_BYTES + (size_t)n_slots * sizeof(double);
  SRAD_REQUIRE(ws_bytes >= need, "grad_guard_finalize: workspace too small (%zu bytes, %d slots need %zu)", ws_bytes, n_slots, need);
  SRAD_REQUIRE(!guard_overlaps(ws, ws_bytes, hyper, 4), "grad_guard_finalize: the workspace overlaps dev_hyper");
  hipLaunchKernelGGL(grad_guard_finalize_kernel, dim3(1), dim3(256), 0, stream, guard_partials(ws), n_slots,
                     reinterpret_cast<SradGuardState*>(ws), guard_record(ws), hyper, beta1, beta2, max_norm);
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

// the guard's state and record may not share a byte with a buffer the step reads or writes
static int adam_guarded_check(const char* what, const float* p, const float* g, const float* m, const float* v, const float* ema,
                              size_t n, const void* ws) {
  SRAD_REQUIRE(((uintptr_t)ws & 15) == 0, "%s: the workspace must be 16-byte aligned", what);
  const size_t hb = SRAD_GUARD_HEADER_BYTES;
  SRAD_REQUIRE(!guard_overlaps(ws, hb, p, n) && !guard_overlaps(ws, hb, g, n) && !guard_overlaps(ws, hb, m, n) &&
                   !guard_overlaps(ws, hb, v, n) && !(ema && guard_overlaps(ws, hb, ema, n)),
               "%s: the guard state overlaps another buffer", what);
  return SRAD_OK;
}

int srad_launch_adam_guarded(float* p, const float* g, float* m, float* v, size_t n, float beta1, float beta2, float eps,
                             float weight_decay, const void* ws, hipStream_t stream) {
  SRAD_TRY(adam_guarded_check("adam_guarded_step", p, g, m, v, nullptr, n, ws));
  SradProfScope prof(stream, SRAD_K_OPTIM, 12.0 * n, 28.0 * n);
  hipLaunchKernelGGL(adam_guarded_kernel, dim3(grid_for(n)), dim3(256), 0, stream, p, g, m, v, n, beta1, beta2, eps, weight_decay,
                     guard_record(ws));
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

int srad_launch_adam_ema_guarded(float* p, const float* g, float* m, float* v, float* ema, size_t n, float beta1, float beta2,
                                 float eps, float weight_decay, float ema_decay, const void* ws, hipStream_t stream) {
  float omd;
  SRAD_TRY(adam_ema_check("adam_ema_guarded_step", p, g, m, v, ema, n, ema_decay, &omd));
  SRAD_TRY(adam_guarded_check("adam_ema_guarded_step", p, g, m, v, ema, n, ws));
  SradProfScope prof(stream, SRAD_K_OPTIM, 15.0 * n, 36.0 * n);
  hipLaunchKernelGGL(adam_ema_guarded_kernel, dim3(grid_for(n)), dim3(256), 0, stream, p, g, m, v, ema, n, beta1, beta2, eps,
                     weight_decay, guard_record(ws), ema_decay, omd);
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}


namespace {
__global__ void set4_kernel(float* __restrict__ dst, float a, float b, float c, float d) {
  if (threadIdx.x == 0) { dst[0] = a; dst[1] = b; dst[2] = c; dst[3] = d; }
}
}  // namespace
int srad_launch_set4(float* dst, float a, float b, float c, float d, hipStream_t stream) {
  hipLaunchKernelGGL(set4_kernel, dim3(1), dim3(64), 0, stream, dst, a, b, c, d);
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}
