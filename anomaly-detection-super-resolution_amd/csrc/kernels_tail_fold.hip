// kernels_tail_fold.hip - DRCT's output end as one launch: everything after conv_before_upsample's LeakyReLU is
// linear (the Upsample convolutions, their PixelShuffles, conv_last; reference src/drct.py:694-713, 842-847, 894-895), so the
// s x s HR pixels of an LR pixel are one 5 x 5 convolution of c2 (tail_fold.h has the algebra and the nine position classes).
//   build : the fold from the fp32 sources, in fp32, in two steps (head = conv_last o up_1, then head o up_0), the bf16 pack
//           in the kernel's fragment order and the bias table.  Runs once per weight load, never inside a captured graph.
//   kernel: one workgroup per 16 pixels of an LR row, five waves, wave k owns row k of the 5 x 5 window (5 taps x 2 chunks
//           of 32 channels); both MFMA operands straight from global memory (c2 rounded to bf16 once, the pack as it lies),
//           fp32 accumulation, the five partial sums added through LDS in a fixed order, then bias, / img_range + mean and the
//           NCHW store.  The class in y is uniform per tile; a tile that holds column 0 or W - 1 accumulates with that
//           class's weights too and every pixel picks its own sum.
#include "srad_common.h"
#include "tail_fold.h"

namespace {

struct FoldGeom { int F, C, scale, N; };

// head[cls][oc][uy][ux][h] = sum over (t1, t2) per axis landing on (uy, ux) of sum_g conv_last[c][g][t1] up_1[4 g + i2][h][t2]
// (scale 2: conv_last[c][h][t1] itself); zero where no path lands, i.e. also where the position is outside its map
__global__ __launch_bounds__(256) void tail_fold_head_kernel(FoldGeom g, const float* __restrict__ w_last, const float* __restrict__ w_up1,
                                                             float* __restrict__ head) {
  const int F = g.F, s = g.scale, n2 = tf_head_taps(s);
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)TF_CLASSES * g.N * TF_U * TF_U * F) return;
  const int h = (int)(idx % F), ux = (int)(idx / F % TF_U), uy = (int)(idx / ((size_t)F * TF_U) % TF_U);
  const int oc = (int)(idx / ((size_t)F * TF_U * TF_U) % g.N), cls = (int)(idx / ((size_t)F * TF_U * TF_U * g.N));
  const int cy = cls / 3, cx = cls % 3, px = oc % s, py = (oc / s) % s, c = oc / (s * s);
  float acc = 0.f;
  for (int t1y = 0; t1y < 3; ++t1y)
    for (int t2y = 0; t2y < n2; ++t2y) {
      int u, i2y;
      if (!tf_head(s, cy, py, t1y, t2y, &u, &i2y) || u != uy) continue;
      for (int t1x = 0; t1x < 3; ++t1x)
        for (int t2x = 0; t2x < n2; ++t2x) {
          int v, i2x;
          if (!tf_head(s, cx, px, t1x, t2x, &v, &i2x) || v != ux) continue;
          if (s == 4) {
            const float* const wl = w_last + (size_t)c * F * 9 + t1y * 3 + t1x;
            const float* const w1 = w_up1 + ((size_t)(i2y * 2 + i2x) * F + h) * 9 + t2y * 3 + t2x;
            for (int q = 0; q < F; ++q) acc += wl[(size_t)q * 9] * w1[(size_t)q * 4 * F * 9];
          } else {
            acc += w_last[((size_t)c * F + h) * 9 + t1y * 3 + t1x];
          }
        }
    }
  head[idx] = acc;
}

// wf[cls][oc][dy][dx][f] = sum over (u, t3) per axis landing on (dy, dx) of sum_h head[..][uy][ux][h] up_0[4 h + i1][f][t3];
// taps outside the image are stored as zeros
__global__ __launch_bounds__(256) void tail_fold_compose_kernel(FoldGeom g, const float* __restrict__ head, const float* __restrict__ w_up0,
                                                                float* __restrict__ wf) {
  const int F = g.F;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)TF_CLASSES * g.N * TF_TAPS * F) return;
  const int f = (int)(idx % F), tap = (int)(idx / F % TF_TAPS);
  const size_t co = idx / ((size_t)F * TF_TAPS);            // cls * N + oc
  const int cls = (int)(co / g.N), dy = tap / TF_K - TF_RADIUS, dx = tap % TF_K - TF_RADIUS;
  float acc = 0.f;
  if (tf_tap_in_image(cls / 3, dy) && tf_tap_in_image(cls % 3, dx))
    for (int uy = 0; uy < TF_U; ++uy) {
      int i1y, t3y;
      if (!tf_tail(uy, dy, &i1y, &t3y)) continue;
      for (int ux = 0; ux < TF_U; ++ux) {
        int i1x, t3x;
        if (!tf_tail(ux, dx, &i1x, &t3x)) continue;
        const float* const hd = head + ((co * TF_U + uy) * TF_U + ux) * F;
        const float* const w0 = w_up0 + ((size_t)(i1y * 2 + i1x) * F + f) * 9 + t3y * 3 + t3x;
        for (int h = 0; h < F; ++h) acc += hd[h] * w0[(size_t)h * 4 * F * 9];
      }
    }
  wf[idx] = acc;
}

// bias[cls][16 NT] (columns >= N zero): conv_last's bias, up_1's through every conv_last tap that stays inside its map, up_0's
// through every head position that does
__global__ __launch_bounds__(256) void tail_fold_bias_kernel(FoldGeom g, int npad, const float* __restrict__ head, const float* __restrict__ w_last,
                                                             const float* __restrict__ b_last, const float* __restrict__ b_up1,
                                                             const float* __restrict__ b_up0, float* __restrict__ bias) {
  const int F = g.F, s = g.scale;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= TF_CLASSES * npad) return;
  const int oc = idx % npad, cls = idx / npad;
  if (oc >= g.N) { bias[idx] = 0.f; return; }
  const int cy = cls / 3, cx = cls % 3, px = oc % s, py = (oc / s) % s, c = oc / (s * s);
  float acc = b_last[c];
  if (s == 4)
    for (int t1y = 0; t1y < 3; ++t1y)
      for (int t1x = 0; t1x < 3; ++t1x) {
        const int ry = py + t1y - 1, rx = px + t1x - 1;
        if (!tf_inside(cy, ry, s) || !tf_inside(cx, rx, s)) continue;
        const float* const wl = w_last + (size_t)c * F * 9 + t1y * 3 + t1x;
        const float* const b1 = b_up1 + (ry & 1) * 2 + (rx & 1);
        for (int q = 0; q < F; ++q) acc += wl[(size_t)q * 9] * b1[4 * q];
      }
  for (int uy = 0; uy < TF_U; ++uy)
    for (int ux = 0; ux < TF_U; ++ux) {
      const float* const hd = head + ((((size_t)cls * g.N + oc) * TF_U + uy) * TF_U + ux) * F;
      const float* const b0 = b_up0 + (uy & 1) * 2 + (ux & 1);
      for (int h = 0; h < F; ++h) acc += hd[h] * b0[4 * h];
    }
  bias[idx] = acc;
}

// pack[cls][nt][tap][j][lane][8]: lane = 16 fq + fr holds bf16(wf[cls][16 nt + fr][tap][32 j + 8 fq .. + 7]) - the A operand of
// v_mfma_f32_16x16x32_bf16 as one 16-byte load per lane; rows >= N are zeros
__global__ __launch_bounds__(256) void tail_fold_pack_kernel(FoldGeom g, int NT, const float* __restrict__ wf, __bf16* __restrict__ pack) {
  const int F = g.F, J = F / 32;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)TF_CLASSES * NT * TF_TAPS * J * 512) return;
  const int e = (int)(idx & 7), lane = (int)(idx >> 3 & 63), fr = lane & 15, fq = lane >> 4;
  const int j = (int)(idx / 512 % J), tap = (int)(idx / ((size_t)512 * J) % TF_TAPS);
  const int nt = (int)(idx / ((size_t)512 * J * TF_TAPS) % NT), cls = (int)(idx / ((size_t)512 * J * TF_TAPS * NT));
  const int oc = 16 * nt + fr;
  pack[idx] = oc < g.N ? (__bf16)wf[(((size_t)cls * g.N + oc) * TF_TAPS + tap) * F + 32 * j + 8 * fq + e] : (__bf16)0.f;
}

struct TailFoldParams {
  const float* X;            // c2 [B*H*W][64]
  const __bf16* pack;
  const float* bias;         // [9][16 NT]
  float* Y;                  // [B][C][S H][S W]
  int B, H, W, C, tpr;       // tpr: 16-pixel tiles per LR row
  float inv_range, mean0, mean1, mean2;
};

template <int S, int NT>
__global__ __launch_bounds__(320) void tail_fold_kernel(const TailFoldParams p) {
  constexpr int F = 64, J = 2;
  __shared__ f32x4 red[TF_K][NT][64];
  const int lane = threadIdx.x & 63, fr = lane & 15, fq = lane >> 4, ky = threadIdx.x >> 6;
  const int H = p.H, W = p.W;
  const int row = blockIdx.x / p.tpr, x0 = (blockIdx.x - row * p.tpr) << 4;
  const int b = row / H, y = row - b * H;
  const int x = x0 + fr, xc = min(x, W - 1);                      // lanes beyond the row compute on its last pixel and store nothing
  const int cy = tf_class(y, H), cxp = tf_class(xc, W);
  const int yy = y + ky - TF_RADIUS;
  const bool first = x0 == 0, last = x0 + 16 >= W;                // uniform: does the tile hold column 0 / W - 1
  const f32x4 z4 = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 a0[NT], a1[NT], a2[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) { a0[nt] = z4; a1[nt] = z4; a2[nt] = z4; }
  if (yy >= 0 && yy < H) {                                         // (uniform per wave: a window row outside the image adds nothing)
    const float* const xrow = p.X + (size_t)(b * H + yy) * W * F + 8 * fq;
    const __bf16* const wrow = p.pack + ((size_t)(cy * 3) * NT * TF_TAPS + ky * TF_K) * (J * 512) + lane * 8;
    constexpr size_t CLS = (size_t)NT * TF_TAPS * J * 512, NTS = (size_t)TF_TAPS * J * 512;
#pragma unroll
    for (int kx = 0; kx < TF_K; ++kx) {
      const int xx = xc + kx - TF_RADIUS;
      const bool in = xx >= 0 && xx < W;
      const float* const src = xrow + (size_t)min(max(xx, 0), W - 1) * F;      // clamped: no load behind a branch
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const f32x4 lo = *reinterpret_cast<const f32x4*>(src + 32 * j), hi = *reinterpret_cast<const f32x4*>(src + 32 * j + 4);
        bf16x8 a;
#pragma unroll
        for (int e = 0; e < 4; ++e) { a[e] = (__bf16)lo[e]; a[4 + e] = (__bf16)hi[e]; }
        u32x4 au = __builtin_bit_cast(u32x4, a);
#pragma unroll
        for (int e = 0; e < 4; ++e) au[e] = in ? au[e] : 0u;
        a = __builtin_bit_cast(bf16x8, au);
        const __bf16* const wt = wrow + (size_t)(kx * J + j) * 512;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          a1[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(wt + CLS + nt * NTS), a, a1[nt], 0, 0, 0);
          if (first) a0[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(wt + nt * NTS), a, a0[nt], 0, 0, 0);
          if (last) a2[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(wt + 2 * CLS + nt * NTS), a, a2[nt], 0, 0, 0);
        }
      }
    }
  }
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) red[ky][nt][lane] = cxp == TF_FIRST ? a0[nt] : (cxp == TF_LAST ? a2[nt] : a1[nt]);
  __syncthreads();
  if (ky >= NT) return;
  const int nt = ky;                                               // wave nt finishes column tile nt
  f32x4 v = red[0][nt][lane];
#pragma unroll
  for (int k = 1; k < TF_K; ++k) v += red[k][nt][lane];
  v += *reinterpret_cast<const f32x4*>(p.bias + (cy * 3 + cxp) * (16 * NT) + 16 * nt + 4 * fq);
  // lane (fr, fq) holds outputs 16 nt + 4 fq .. + 3 of pixel x
  if constexpr (S == 4) {                                          // a column tile is a channel, fq the HR row, the four values its HR columns
    const int c = nt;
    const float mean = c == 0 ? p.mean0 : (c == 1 ? p.mean1 : p.mean2);
    v = v * p.inv_range + mean;
    if (x < W) *reinterpret_cast<f32x4*>(p.Y + ((size_t)(b * p.C + c) * 4 * H + 4 * y + fq) * 4 * W + 4 * x) = v;
  } else {                                                         // fq is the channel, the four values its 2 x 2 HR pixels
    const int c = fq;
    const float mean = c == 0 ? p.mean0 : (c == 1 ? p.mean1 : p.mean2);
    v = v * p.inv_range + mean;
    if (x < W && c < p.C) {
      float* const dst = p.Y + ((size_t)(b * p.C + c) * 2 * H + 2 * y) * 2 * W + 2 * x;
      dst[0] = v[0]; dst[1] = v[1];
      dst[2 * W] = v[2]; dst[2 * W + 1] = v[3];
    }
  }
}

}  // namespace

bool srad_tail_fold_supported(int prec, int F, int C, int scale) {
  return prec == SRAD_PREC_BF16 && F == 64 && (scale == 2 || scale == 4) && (C == 1 || C == 3);
}

int srad_launch_tail_fold_build(const TailFoldLayout& l, char* base, hipStream_t s) {
  SRAD_REQUIRE(base && ((uintptr_t)base & 255) == 0, "tail_fold_build: the fold's region must be 256-byte aligned");
  SRAD_REQUIRE(l.F % 32 == 0 && (l.scale == 2 || l.scale == 4) && l.C >= 1, "tail_fold_build: unsupported geometry");
  const FoldGeom g{l.F, l.C, l.scale, l.N};
  auto f = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
  auto blocks = [](size_t n) { return dim3((unsigned)((n + 255) / 256)); };
  SradProfScope prof(s, SRAD_K_PACK, 0.0, (double)l.bytes);
  hipLaunchKernelGGL(tail_fold_head_kernel, blocks((size_t)TF_CLASSES * l.N * TF_U * TF_U * l.F), dim3(256), 0, s, g, f(l.w_last), f(l.w_up1), f(l.head));
  hipLaunchKernelGGL(tail_fold_compose_kernel, blocks((size_t)TF_CLASSES * l.N * TF_TAPS * l.F), dim3(256), 0, s, g, f(l.head), f(l.w_up0), f(l.wf));
  hipLaunchKernelGGL(tail_fold_bias_kernel, blocks((size_t)TF_CLASSES * l.NT * 16), dim3(256), 0, s, g, l.NT * 16, f(l.head), f(l.w_last), f(l.b_last),
                     f(l.b_up1), f(l.b_up0), f(l.bias));
  hipLaunchKernelGGL(tail_fold_pack_kernel, blocks((size_t)TF_CLASSES * l.NT * TF_TAPS * (l.F / 32) * 512), dim3(256), 0, s, g, l.NT, f(l.wf),
                     reinterpret_cast<__bf16*>(base + l.pack));
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

int srad_launch_tail_fold(const TailFoldLayout& l, const char* base, const float* X, int B, int H, int W, float* Y, float inv_range,
                          const float mean3[3], hipStream_t s) {
  SRAD_REQUIRE(l.F == 64 && (l.scale == 2 || l.scale == 4) && (l.C == 1 || l.C == 3), "tail_fold: unsupported geometry");
  SRAD_REQUIRE(B > 0 && H >= 2 && W >= 2, "tail_fold: the map must be at least 2 x 2 (got %d x %d x %d)", B, H, W);
  SRAD_REQUIRE(((uintptr_t)X & 15) == 0 && ((uintptr_t)Y & 15) == 0, "tail_fold: input and output must be 16-byte aligned");
  TailFoldParams p{};
  p.X = X; p.pack = reinterpret_cast<const __bf16*>(base + l.pack); p.bias = reinterpret_cast<const float*>(base + l.bias); p.Y = Y;
  p.B = B; p.H = H; p.W = W; p.C = l.C; p.tpr = (W + 15) / 16;
  p.inv_range = inv_range; p.mean0 = mean3[0]; p.mean1 = mean3[1]; p.mean2 = mean3[2];
  SRAD_REQUIRE((int64_t)B * H * p.tpr < (1LL << 31), "tail_fold: too many tiles");
  const dim3 grid((unsigned)(B * H * p.tpr));
  const double T = (double)B * H * W;
  SradProfScope prof(s, SRAD_K_TAIL_FOLD, 2.0 * T * l.N * TF_TAPS * 64, 4.0 * T * (64 + l.N));
  if (l.scale == 2) hipLaunchKernelGGL((tail_fold_kernel<2, 1>), grid, dim3(320), 0, s, p);
  else if (l.C == 1) hipLaunchKernelGGL((tail_fold_kernel<4, 1>), grid, dim3(320), 0, s, p);
  else hipLaunchKernelGGL((tail_fold_kernel<4, 3>), grid, dim3(320), 0, s, p);
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

extern "C" {

int srad_op_tail_fold_layout(int F, int C, int scale, size_t* wf_off, size_t* pack_off, size_t* bias_off, size_t* bytes) {
  SRAD_REQUIRE(F > 0 && F % 32 == 0 && (scale == 2 || scale == 4) && C >= 1 && C <= 3, "op_tail_fold_layout: unsupported geometry");
  const TailFoldLayout l = tf_layout(F, C, scale);
  if (wf_off) *wf_off = l.wf;
  if (pack_off) *pack_off = l.pack;
  if (bias_off) *bias_off = l.bias;
  if (bytes) *bytes = l.bytes;
  return SRAD_OK;
}

int srad_op_tail_fold_build(int F, int C, int scale, const float* w_up0, const float* b_up0, const float* w_up1, const float* b_up1,
                            const float* w_last, const float* b_last, void* scratch, size_t scratch_bytes, void* stream) {
  SRAD_REQUIRE(F > 0 && F % 32 == 0 && (scale == 2 || scale == 4) && C >= 1 && C <= 3, "op_tail_fold_build: unsupported geometry");
  SRAD_REQUIRE(w_up0 && b_up0 && w_last && b_last && scratch && (scale == 2 || (w_up1 && b_up1)), "op_tail_fold_build: null argument");
  const TailFoldLayout l = tf_layout(F, C, scale);
  SRAD_REQUIRE(scratch_bytes >= l.bytes, "op_tail_fold_build: scratch %zu bytes, %zu needed", scratch_bytes, l.bytes);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  char* const base = reinterpret_cast<char*>(scratch);
  auto put = [&](size_t off, const float* src, size_t n) { return hipMemcpyAsync(base + off, src, n * 4, hipMemcpyDeviceToDevice, s); };
  SRAD_CHECK_HIP(put(l.w_up0, w_up0, (size_t)4 * F * F * 9));
  SRAD_CHECK_HIP(put(l.b_up0, b_up0, (size_t)4 * F));
  if (scale == 4) {
    SRAD_CHECK_HIP(put(l.w_up1, w_up1, (size_t)4 * F * F * 9));
    SRAD_CHECK_HIP(put(l.b_up1, b_up1, (size_t)4 * F));
  }
  SRAD_CHECK_HIP(put(l.w_last, w_last, (size_t)C * F * 9));
  SRAD_CHECK_HIP(put(l.b_last, b_last, (size_t)C));
  return srad_launch_tail_fold_build(l, base, s);
}

int srad_op_tail_fold(const float* c2, int B, int H, int W, int C, int scale, const void* fold, float img_range, float mean0, float mean1,
                      float mean2, float* y, void* stream) {
  SRAD_REQUIRE(c2 && fold && y, "op_tail_fold: null argument");
  SRAD_REQUIRE(srad_tail_fold_supported(SRAD_PREC_BF16, 64, C, scale), "op_tail_fold: scale must be 2 or 4 and the image gray or RGB");
  SRAD_REQUIRE(img_range > 0.f, "op_tail_fold: img_range must be positive");
  const float mean3[3] = {mean0, mean1, mean2};
  return srad_launch_tail_fold(tf_layout(64, C, scale), reinterpret_cast<const char*>(fold), c2, B, H, W, y, 1.0f / img_range, mean3,
                               reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
