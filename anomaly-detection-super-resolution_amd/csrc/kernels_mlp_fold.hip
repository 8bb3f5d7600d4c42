// kernels_mlp_fold.hip - builds a Swin block's folded second-half weight (mlp_fold.h) from the fp32 sources in
// its region: Wf = [A | A W2] with both parts zero-padded to whole 32-wide k chunks, bf = A b2 + b_a, then Wf as the bf16
// fragment pack the block kernels stream.  Products accumulate in fp64 in index order (a product of two fp32 values is exact
// in fp64) and are rounded to fp32 once.  Three launches per block, once per weight load, never inside a capture.
#include "srad_common.h"
#include "mlp_fold.h"

namespace {

// one thread per element of Wf [no][kf]; consecutive threads read consecutive columns of W2
__global__ void mlp_fold_compose_kernel(const float* __restrict__ A, const float* __restrict__ W2, float* __restrict__ Wf, int d, int m, int no,
                                        int kc32, int kf) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= (size_t)no * kf) return;
  const int r = (int)(i / kf), c = (int)(i - (size_t)r * kf);
  float v = 0.f;
  if (c < kc32) {
    if (c < d) v = A[(size_t)r * d + c];
  } else if (c - kc32 < m) {
    const int j = c - kc32;
    double acc = 0.0;
    for (int k = 0; k < d; ++k) acc += (double)A[(size_t)r * d + k] * (double)W2[(size_t)k * m + j];
    v = (float)acc;
  }
  Wf[i] = v;
}

__global__ void mlp_fold_bias_kernel(const float* __restrict__ A, const float* __restrict__ b2, const float* __restrict__ ba,
                                     float* __restrict__ bf, int d, int no) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= no) return;
  double acc = 0.0;
  for (int k = 0; k < d; ++k) acc += (double)A[(size_t)r * d + k] * (double)b2[k];
  bf[r] = (float)(acc + (double)ba[r]);
}

}  // namespace

int srad_launch_mlp_fold_build(const MlpFoldLayout& l, char* base, hipStream_t s) {
  SRAD_REQUIRE(base && ((uintptr_t)base & 255) == 0, "mlp_fold_build: the fold's region must be 256-byte aligned");
  SRAD_REQUIRE(l.d > 0 && l.m > 0 && l.no > 0, "mlp_fold_build: empty geometry");
  auto f = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
  {
    SradProfScope prof(s, SRAD_K_PACK, 2.0 * l.no * (double)l.d * l.m, (double)l.bytes);
    const size_t n = (size_t)l.no * l.kf;
    hipLaunchKernelGGL(mlp_fold_compose_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, f(l.a), f(l.w2), f(l.wf), l.d, l.m, l.no, 32 * l.kc,
                       l.kf);
    hipLaunchKernelGGL(mlp_fold_bias_kernel, dim3((unsigned)((l.no + 63) / 64)), dim3(64), 0, s, f(l.a), f(l.b2), f(l.ba), f(l.bias), l.d, l.no);
    SRAD_CHECK_HIP(hipGetLastError());
  }
  return srad_launch_pack_weight_frag(f(l.wf), base + l.pack, l.no, l.kf, s);
}

// the sources into a block's region, then the build (the op entry points' form: the engine copies sources in set_param)
int srad_mlp_fold_from_sources(const MlpFoldLayout& l, char* base, const float* w_fc2, const float* b_fc2, const float* w_adj, const float* b_adj,
                               hipStream_t s) {
  auto put = [&](size_t off, const float* src, size_t n) { return hipMemcpyAsync(base + off, src, n * 4, hipMemcpyDeviceToDevice, s); };
  SRAD_CHECK_HIP(put(l.w2, w_fc2, (size_t)l.d * l.m));
  SRAD_CHECK_HIP(put(l.b2, b_fc2, (size_t)l.d));
  SRAD_CHECK_HIP(put(l.a, w_adj, (size_t)l.no * l.d));
  SRAD_CHECK_HIP(put(l.ba, b_adj, (size_t)l.no));
  return srad_launch_mlp_fold_build(l, base, s);
}

extern "C" {

size_t srad_op_mlp_fold_scratch_bytes(int d, int m, int no) { return mf_layout(d > 0 ? d : 4, m > 0 ? m : 4, no > 0 ? no : 4).bytes; }

// the region's layout (mlp_fold.h), host only: off[8] = w2, b2, a, ba, wf, pack, bias, bytes
int srad_op_mlp_fold_layout(int d, int m, int no, size_t* off, int* kf) {
  SRAD_REQUIRE(d > 0 && m > 0 && no > 0 && off, "op_mlp_fold_layout: bad argument");
  const MlpFoldLayout l = mf_layout(d, m, no);
  const size_t v[8] = {l.w2, l.b2, l.a, l.ba, l.wf, l.pack, l.bias, l.bytes};
  for (int i = 0; i < 8; ++i) off[i] = v[i];
  if (kf) *kf = l.kf;
  return SRAD_OK;
}

// Composes into caller scratch (>= srad_op_mlp_fold_scratch_bytes, 256-byte aligned) and reports where the results lie:
// Wf fp32 [no][*kf], the fragment pack, bf fp32 [no] (byte offsets into scratch).
int srad_op_mlp_fold_compose(int d, int m, int no, const float* w_fc2, const float* b_fc2, const float* w_adj, const float* b_adj, void* scratch,
                             size_t scratch_bytes, size_t* wf_off, size_t* pack_off, size_t* bias_off, int* kf, void* stream) {
  SRAD_REQUIRE(w_fc2 && b_fc2 && w_adj && b_adj && scratch, "op_mlp_fold_compose: null argument");
  SRAD_REQUIRE(d > 0 && m > 0 && no > 0, "op_mlp_fold_compose: empty geometry d=%d m=%d no=%d", d, m, no);
  const MlpFoldLayout l = mf_layout(d, m, no);
  SRAD_REQUIRE(scratch_bytes >= l.bytes && ((uintptr_t)scratch & 255) == 0, "op_mlp_fold_compose: scratch %zu bytes, %zu needed (256-byte aligned)",
               scratch_bytes, l.bytes);
  if (wf_off) *wf_off = l.wf;
  if (pack_off) *pack_off = l.pack;
  if (bias_off) *bias_off = l.bias;
  if (kf) *kf = l.kf;
  return srad_mlp_fold_from_sources(l, reinterpret_cast<char*>(scratch), w_fc2, b_fc2, w_adj, b_adj, reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
