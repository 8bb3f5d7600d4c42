// kernels_loss.hip - the loss types of the reference's loss factory (src/loss.py:72-121) as device reductions with
// their gradients: L1 (nn.L1Loss), MSE (nn.MSELoss), PSNR (PSNRLoss, loss.py:63-70) and SSIM (calc_ssim, loss.py:9-52).
// Every CLI path of the reference hard-codes '1*L1' (main.py:453, evaluate.py:317); the other three exist for
// completeness of the `Loss(opt, ckp)` surface.  All are HBM-bound elementwise / small-stencil work: coalesced float
// loads, double partial sums per workgroup, a fixed-order finish (results are bit-reproducible).  The kinds GMS and MSGMS
// (not in the reference) enter through the same three entry points; their kernels are in kernels_gms.hip (gms_loss.h).
//
// SSIM loss, as written in the reference (quirks kept verbatim):
//   s = clamp(x / rgb_range, 0, 1); shave = scale + 6 with scale hard-wired to 4 (loss.py:61) -> crop 10 px when the
//   width exceeds 20, else 1 px; RGB -> luminance with (65.738, 129.057, 25.064) / 256; 11 x 11 mean filter with ZERO
//   padding; C1 = (0.01 * 255)^2 and C2 = (0.03 * 255)^2 although the data are in [0, 1]; loss = sum(1 - map) / batch_size
//   where batch_size is the option value, not the tensor's.
// Backward: with m1 = box(x), e11 = box(x^2), e12 = box(x y) the map is S(m1, e11, e12; y); the zero-padded box filter
// with a symmetric kernel is self-adjoint, so dL/dx = box(dL/dS * dS/dm1) + 2 x box(dL/dS * dS/de11) + y box(dL/dS * dS/de12),
// then the luminance weights, the clamp's indicator and 1 / rgb_range.
#include "../../include/srad.h"
#include "srad_common.h"
#include "gms_loss.h"
#include <algorithm>

namespace {

constexpr int LOSS_NB = 1024;     // partial sums per reduction

// kind 0: |a - b|, kind 1 / 2: (a - b)^2
template <int SQ>
__global__ __launch_bounds__(256) void diff_sum_kernel(const float* __restrict__ a, const float* __restrict__ b, size_t n,
                                                       double* __restrict__ partial) {
  __shared__ double red[256];
  double local = 0.0;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float d = a[i] - b[i];
    local += SQ ? (double)(d * d) : (double)fabsf(d);
  }
  const double s = srad_block_sum(local, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// *out = the loss value, *aux = what the backward needs (the mean squared error for PSNR); aux may be null except for PSNR
__global__ void finish_kernel(const double* __restrict__ partial, int nb, double inv_n, int kind, double* __restrict__ out,
                              double* __restrict__ aux) {
  if (threadIdx.x || blockIdx.x) return;
  double s = 0.0;
  for (int i = 0; i < nb; ++i) s += partial[i];
  if (kind == SRAD_LOSS_PSNR) {
    // nn.MSELoss in fp32, then 10 * log10(255^2 / (mse + 1e-8)) in fp32 (loss.py:67-70)
    const float mse = (float)(s * inv_n);
    *aux = (double)mse;
    *out = -(double)(10.0f * log10f((255.0f * 255.0f) / (mse + 1e-8f)));
  } else {
    *out = s * inv_n;
    if (aux) *aux = *out;
  }
}

// dy (+)= gscale * d loss / d a
__global__ void diff_grad_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ dy, size_t n,
                                 int kind, float inv_n, const double* __restrict__ fwd, const float* __restrict__ gscale,
                                 float weight, int accumulate) {
  float g = weight * (gscale ? gscale[0] : 1.0f);
  if (kind == SRAD_LOSS_MSE) g *= 2.0f * inv_n;
  else if (kind == SRAD_LOSS_PSNR) g *= (float)(10.0 / 2.302585092994046) / ((float)fwd[1] + 1e-8f) * 2.0f * inv_n;   // d(-10 log10(c / (m + e)))/dm = 10 / (ln 10 (m + e))
  else g *= inv_n;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float d = a[i] - b[i];
    const float v = kind == SRAD_LOSS_L1 ? (d > 0.f ? g : (d < 0.f ? -g : 0.f)) : g * d;
    dy[i] = accumulate ? dy[i] + v : v;
  }
}

// ---- SSIM loss ---------------------------------------------------------------------------------------------------
struct SsimGeo {
  int B, C, H, W;           // sr / hr tensors (hr may be the smaller one: sr is read through its own strides)
  int sH, sW;               // sr plane size
  int y0, x0, h2, w2;       // cropped region
  float inv_range;
};

__device__ __forceinline__ float lum_at(const float* __restrict__ t, size_t plane, int W, int C, int yy, int xx, float inv_range) {
  if (C == 1) return fminf(fmaxf(t[(size_t)yy * W + xx] * inv_range, 0.0f), 1.0f);
  const float cv[3] = {65.738f / 256.0f, 129.057f / 256.0f, 25.064f / 256.0f};
  float acc = 0.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) acc += fminf(fmaxf(t[c * plane + (size_t)yy * W + xx] * inv_range, 0.0f), 1.0f) * cv[c];
  return acc;
}

// luminance planes of the cropped region: lx, ly [B][h2][w2]
__global__ void ssim_lum_kernel(const float* __restrict__ sr, const float* __restrict__ hr, SsimGeo g, float* __restrict__ lx,
                                float* __restrict__ ly) {
  const size_t total = (size_t)g.B * g.h2 * g.w2;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int b = (int)(i / ((size_t)g.h2 * g.w2));
    const int p = (int)(i - (size_t)b * g.h2 * g.w2);
    const int yy = g.y0 + p / g.w2, xx = g.x0 + p % g.w2;
    lx[i] = lum_at(sr + (size_t)b * g.C * g.sH * g.sW, (size_t)g.sH * g.sW, g.sW, g.C, yy, xx, g.inv_range);
    ly[i] = lum_at(hr + (size_t)b * g.C * g.H * g.W, (size_t)g.H * g.W, g.W, g.C, yy, xx, g.inv_range);
  }
}

// per pixel: the five box means -> SSIM map value; optionally the three partial-derivative maps for the backward
template <bool GRAD>
__global__ __launch_bounds__(256) void ssim_map_kernel(const float* __restrict__ lx, const float* __restrict__ ly, SsimGeo g,
                                                       double* __restrict__ partial, float* __restrict__ dm1,
                                                       float* __restrict__ de11, float* __restrict__ de12) {
  __shared__ double red[256];
  const float C1 = (float)((0.01 * 255) * (0.01 * 255)), C2 = (float)((0.03 * 255) * (0.03 * 255));   // python doubles -> fp32 scalars
  const size_t total = (size_t)g.B * g.h2 * g.w2;
  double local = 0.0;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int b = (int)(i / ((size_t)g.h2 * g.w2));
    const int p = (int)(i - (size_t)b * g.h2 * g.w2);
    const int yy = p / g.w2, xx = p % g.w2;
    const float* X = lx + (size_t)b * g.h2 * g.w2;
    const float* Y = ly + (size_t)b * g.h2 * g.w2;
    float a1 = 0, a2 = 0, a11 = 0, a22 = 0, a12 = 0;
    for (int dy = -5; dy <= 5; ++dy) {
      const int y2 = yy + dy;
      if (y2 < 0 || y2 >= g.h2) continue;
      for (int dx = -5; dx <= 5; ++dx) {
        const int x2 = xx + dx;
        if (x2 < 0 || x2 >= g.w2) continue;
        const float u = X[(size_t)y2 * g.w2 + x2], v = Y[(size_t)y2 * g.w2 + x2];
        a1 += u; a2 += v; a11 += u * u; a22 += v * v; a12 += u * v;
      }
    }
    const float k = 1.0f / 121.0f;
    const float m1 = a1 * k, m2 = a2 * k;
    const float s1 = a11 * k - m1 * m1, s2 = a22 * k - m2 * m2, s12 = a12 * k - m1 * m2;
    const float A1 = 2 * m1 * m2 + C1, A2 = 2 * s12 + C2, B1 = m1 * m1 + m2 * m2 + C1, B2 = s1 + s2 + C2;
    const float S = (A1 * A2) / (B1 * B2);
    local += (double)(1.0f - S);
    if (GRAD) {
      const float den = B1 * B2;
      // m1 enters A1, A2 (through s12), B1 and B2 (through s1)
      const float dnum = 2 * m2 * A2 - 2 * m2 * A1;
      const float dden = 2 * m1 * B2 - 2 * m1 * B1;
      dm1[i] = (dnum * den - A1 * A2 * dden) / (den * den);
      de11[i] = -(A1 * A2) * B1 / (den * den);
      de12[i] = 2 * A1 / den;
    }
  }
  const double s = srad_block_sum(local, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// dsr (+)= gscale * weight * (-1 / batch_size) * [box(dm1) + 2 x box(de11) + y box(de12)] * lum weight * clamp' / range
__global__ void ssim_grad_kernel(const float* __restrict__ sr, const float* __restrict__ lx, const float* __restrict__ ly,
                                 const float* __restrict__ dm1, const float* __restrict__ de11, const float* __restrict__ de12,
                                 SsimGeo g, float coef, const float* __restrict__ gscale, float* __restrict__ dsr, int accumulate) {
  const float cf = coef * (gscale ? gscale[0] : 1.0f);
  const size_t plane = (size_t)g.sH * g.sW;
  const size_t total = (size_t)g.B * plane;
  const float cv[3] = {65.738f / 256.0f, 129.057f / 256.0f, 25.064f / 256.0f};
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int b = (int)(i / plane);
    const int p = (int)(i - (size_t)b * plane);
    const int yy = p / g.sW - g.y0, xx = p % g.sW - g.x0;
    float gy = 0.0f;
    if (yy >= 0 && yy < g.h2 && xx >= 0 && xx < g.w2) {
      const size_t o = (size_t)b * g.h2 * g.w2;
      float b1 = 0, b11 = 0, b12 = 0;
      for (int dy = -5; dy <= 5; ++dy) {
        const int y2 = yy + dy;
        if (y2 < 0 || y2 >= g.h2) continue;
        for (int dx = -5; dx <= 5; ++dx) {
          const int x2 = xx + dx;
          if (x2 < 0 || x2 >= g.w2) continue;
          const size_t q = o + (size_t)y2 * g.w2 + x2;
          b1 += dm1[q]; b11 += de11[q]; b12 += de12[q];
        }
      }
      const size_t q0 = o + (size_t)yy * g.w2 + xx;
      gy = (b1 + 2.0f * lx[q0] * b11 + ly[q0] * b12) * (1.0f / 121.0f) * cf;
    }
    for (int c = 0; c < g.C; ++c) {
      const size_t idx = ((size_t)b * g.C + c) * plane + p;
      const float s = sr[idx] * g.inv_range;
      const float v = (s >= 0.0f && s <= 1.0f) ? gy * (g.C == 1 ? 1.0f : cv[c]) * g.inv_range : 0.0f;   // torch.clamp passes the bounds
      dsr[idx] = accumulate ? dsr[idx] + v : v;
    }
  }
}

inline int grid_for(size_t n) { return (int)std::min<size_t>(LOSS_NB, std::max<size_t>(1, (n + 255) / 256)); }

int ssim_geo(int B, int C, int sH, int sW, int H, int W, float rgb_range, SsimGeo* g) {
  SRAD_REQUIRE(C == 1 || C == 3, "ssim loss: 1 or 3 channels (got %d)", C);
  SRAD_REQUIRE(sH >= H && sW >= W, "ssim loss: sr %dx%d is smaller than hr %dx%d", sH, sW, H, W);
  const int shave = 4 + 6;                               // scale is the literal 4 in SSIMLoss.forward (loss.py:61)
  const int cut = W > 2 * shave ? shave : 1;
  g->B = B; g->C = C; g->H = H; g->W = W; g->sH = sH; g->sW = sW;
  g->y0 = cut; g->x0 = cut; g->h2 = H - 2 * cut; g->w2 = W - 2 * cut;
  g->inv_range = 1.0f / rgb_range;
  SRAD_REQUIRE(g->h2 > 0 && g->w2 > 0, "ssim loss: image %dx%d is too small", H, W);
  return SRAD_OK;
}

}  // namespace

extern "C" {

int srad_l1_workspace_bytes(size_t* bytes) {
  SRAD_REQUIRE(bytes, "l1_workspace_bytes: null");
  *bytes = LOSS_NB * sizeof(double);
  return SRAD_OK;
}

// mean |a - b| -> *out (device double): the L1 loss forward without its second value.  workspace: >= srad_l1_workspace_bytes().
int srad_l1_loss(const float* a, const float* b, int64_t n, double* out, void* workspace, void* stream) {
  SRAD_REQUIRE(a && b && out && workspace && n > 0, "l1_loss: bad argument");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int nb = grid_for((size_t)n);
  double* partial = reinterpret_cast<double*>(workspace);
  hipLaunchKernelGGL(diff_sum_kernel<0>, dim3(nb), dim3(256), 0, s, a, b, (size_t)n, partial);
  hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(64), 0, s, partial, nb, 1.0 / (double)n, (int)SRAD_LOSS_L1, out, (double*)nullptr);
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

int srad_loss_workspace_bytes(int kind, int B, int C, int H, int W, size_t* bytes) {
  SRAD_REQUIRE(bytes && B > 0 && C > 0 && H > 0 && W > 0, "loss_workspace_bytes: bad argument");
  if (kind == SRAD_LOSS_GMS || kind == SRAD_LOSS_MSGMS) return srad_gms_loss_workspace_bytes("loss_workspace_bytes", kind, B, C, H, W, bytes);
  size_t n = LOSS_NB * sizeof(double);
  if (kind == SRAD_LOSS_SSIM) n += 5 * srad_align_up((size_t)B * H * W * sizeof(float), 256);   // lx, ly, dm1, de11, de12
  *bytes = n;
  return SRAD_OK;
}

int srad_loss_forward(int kind, const float* sr, const float* hr, int B, int C, int sH, int sW, int H, int W, float rgb_range,
                      int batch_size, double* out2, void* workspace, size_t workspace_bytes, void* stream) {
  SRAD_REQUIRE(sr && hr && out2 && workspace, "loss_forward: null argument");
  SRAD_REQUIRE(kind >= SRAD_LOSS_L1 && kind <= SRAD_LOSS_MSGMS, "loss_forward: unknown loss kind %d", kind);
  size_t need = 0;
  SRAD_TRY(srad_loss_workspace_bytes(kind, B, C, H, W, &need));
  SRAD_REQUIRE(workspace_bytes >= need, "loss_forward: workspace %zu bytes, %zu needed", workspace_bytes, need);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  double* partial = reinterpret_cast<double*>(workspace);
  if (kind == SRAD_LOSS_GMS || kind == SRAD_LOSS_MSGMS) {
    SRAD_REQUIRE(sH == H && sW == W, "loss_forward: sr and hr must have the same size");
    return srad_gms_loss_forward(kind, sr, hr, B, C, H, W, rgb_range, out2, workspace, stream);
  }
  if (kind != SRAD_LOSS_SSIM) {
    SRAD_REQUIRE(sH == H && sW == W, "loss_forward: sr and hr must have the same size");
    const size_t n = (size_t)B * C * H * W;
    const int nb = grid_for(n);
    if (kind == SRAD_LOSS_L1) hipLaunchKernelGGL(diff_sum_kernel<0>, dim3(nb), dim3(256), 0, s, sr, hr, n, partial);
    else hipLaunchKernelGGL(diff_sum_kernel<1>, dim3(nb), dim3(256), 0, s, sr, hr, n, partial);
    hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(64), 0, s, partial, nb, 1.0 / (double)n, kind, out2, out2 + 1);
    SRAD_CHECK_HIP(hipGetLastError());
    return SRAD_OK;
  }
  SRAD_REQUIRE(batch_size > 0, "ssim loss: batch_size must be positive");
  SsimGeo g;
  SRAD_TRY(ssim_geo(B, C, sH, sW, H, W, rgb_range, &g));
  const size_t slab = srad_align_up((size_t)B * H * W * sizeof(float), 256);
  char* base = reinterpret_cast<char*>(workspace) + LOSS_NB * sizeof(double);
  float* lx = reinterpret_cast<float*>(base);
  float* ly = reinterpret_cast<float*>(base + slab);
  float* dm1 = reinterpret_cast<float*>(base + 2 * slab);
  float* de11 = reinterpret_cast<float*>(base + 3 * slab);
  float* de12 = reinterpret_cast<float*>(base + 4 * slab);
  const size_t total = (size_t)B * g.h2 * g.w2;
  const int nb = grid_for(total);
  hipLaunchKernelGGL(ssim_lum_kernel, dim3(nb), dim3(256), 0, s, sr, hr, g, lx, ly);
  hipLaunchKernelGGL(ssim_map_kernel<true>, dim3(nb), dim3(256), 0, s, lx, ly, g, partial, dm1, de11, de12);
  hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(64), 0, s, partial, nb, 1.0 / (double)batch_size, kind, out2, out2 + 1);
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

int srad_loss_backward(int kind, const float* sr, const float* hr, int B, int C, int sH, int sW, int H, int W, float rgb_range,
                       int batch_size, const double* fwd_out2, const float* gscale_dev, float weight, float* dsr, int accumulate,
                       void* workspace, size_t workspace_bytes, void* stream) {
  SRAD_REQUIRE(sr && hr && dsr && fwd_out2 && workspace, "loss_backward: null argument");
  SRAD_REQUIRE(kind >= SRAD_LOSS_L1 && kind <= SRAD_LOSS_MSGMS, "loss_backward: unknown loss kind %d", kind);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (kind == SRAD_LOSS_GMS || kind == SRAD_LOSS_MSGMS) {
    SRAD_REQUIRE(sH == H && sW == W, "loss_backward: sr and hr must have the same size");
    size_t need = 0;
    SRAD_TRY(srad_loss_workspace_bytes(kind, B, C, H, W, &need));
    SRAD_REQUIRE(workspace_bytes >= need, "loss_backward: workspace %zu bytes, %zu needed (the one srad_loss_forward filled)", workspace_bytes, need);
    return srad_gms_loss_backward(kind, sr, B, C, H, W, rgb_range, gscale_dev, weight, dsr, accumulate, workspace, stream);
  }
  if (kind != SRAD_LOSS_SSIM) {
    SRAD_REQUIRE(sH == H && sW == W, "loss_backward: sr and hr must have the same size");
    const size_t n = (size_t)B * C * H * W;
    hipLaunchKernelGGL(diff_grad_kernel, dim3(grid_for(n) * 4), dim3(256), 0, s, sr, hr, dsr, n, kind, 1.0f / (float)n, fwd_out2,
                       gscale_dev, weight, accumulate);
    SRAD_CHECK_HIP(hipGetLastError());
    return SRAD_OK;
  }
  size_t need = 0;
  SRAD_TRY(srad_loss_workspace_bytes(kind, B, C, H, W, &need));
  SRAD_REQUIRE(workspace_bytes >= need, "loss_backward: workspace %zu bytes, %zu needed (the one srad_loss_forward filled)", workspace_bytes, need);
  SsimGeo g;
  SRAD_TRY(ssim_geo(B, C, sH, sW, H, W, rgb_range, &g));
  const size_t slab = srad_align_up((size_t)B * H * W * sizeof(float), 256);
  char* base = reinterpret_cast<char*>(workspace) + LOSS_NB * sizeof(double);
  const float* lx = reinterpret_cast<const float*>(base);
  const float* ly = reinterpret_cast<const float*>(base + slab);
  const float* dm1 = reinterpret_cast<const float*>(base + 2 * slab);
  const float* de11 = reinterpret_cast<const float*>(base + 3 * slab);
  const float* de12 = reinterpret_cast<const float*>(base + 4 * slab);
  const size_t total = (size_t)B * sH * sW;
  hipLaunchKernelGGL(ssim_grad_kernel, dim3(grid_for(total) * 4), dim3(256), 0, s, sr, lx, ly, dm1, de11, de12, g,
                     -weight / (float)batch_size, gscale_dev, dsr, accumulate);
  SRAD_CHECK_HIP(hipGetLastError());
  return SRAD_OK;
}

}  // extern "C"
