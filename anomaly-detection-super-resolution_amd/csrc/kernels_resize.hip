// kernels_resize.hip - Pillow's 8-bit resize (LANCZOS / BICUBIC) on the device: two integer passes over u8 images
// [n, H, W, C], the horizontal one first with its result rounded to u8 in `tmp`, then the vertical one.  The tables come
// from resample_coeffs.h (host); both passes accumulate in int32 exactly as Pillow does, so every output byte equals
// PIL.Image.resize (DESIGN.md "Resize on the device").  HBM-bound: the source is read once, tmp is 1/scale of it.
// Below them Pillow's mode-F resize of float32 maps [n, H, W] (srad_resize_f32): the same two passes with the double taps of
// resample_coeffs_f.h, every output one sequential fp64 sum rounded to float32 (DESIGN.md "Maps and masks at source size").
#include "srad_common.h"
#include "resample_coeffs_f.h"
#include <vector>

// The float passes are defined by separate fp64 products and sums; hipcc would contract a * b + c into an fma.
#pragma clang fp contract(off)

namespace {

constexpr int kResizeRows = 4;                 // source rows per workgroup of the horizontal pass
constexpr int kResizeStageBytes = (65536 - 16) / kResizeRows;     // longest row (W * C bytes) the horizontal pass stages: 64 KB of LDS

__device__ __forceinline__ uint8_t resize_round(int acc) {
  acc >>= RESAMPLE_PRECISION_BITS;
  return (uint8_t)min(max(acc, 0), 255);
}

// Horizontal pass, src [rows_total, W*C] -> dst [rows_total, w*C].  One workgroup of 256 threads per kResizeRows consecutive
// rows, which are one contiguous byte range: STAGE copies it to LDS with 16-byte loads (bytewise up to the first aligned
// address and after the last whole chunk; the LDS copy starts at the same misalignment, so the chunks land aligned), then
// thread t owns output bytes t, t + 256, .. of all the rows: one coefficient load per tap, kResizeRows byte reads.  Adjacent
// lanes write adjacent bytes.  Without STAGE (rows above kResizeStageBytes) the taps are read from global memory.
template <bool STAGE>
__global__ __launch_bounds__(256) void resize_rows_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                          long long rows_total, int W, int w, int C,
                                                          const int32_t* __restrict__ bounds, const int32_t* __restrict__ coeffs,
                                                          int ksize) {
  extern __shared__ __attribute__((aligned(16))) uint8_t stage[];
  const size_t WC = (size_t)W * C, wC = (size_t)w * C;
  const long long r0 = (long long)blockIdx.x * kResizeRows;
  const int rows = (int)min((long long)kResizeRows, rows_total - r0);
  const uint8_t* g = src + (size_t)r0 * WC;
  const uint8_t* base = g;
  size_t pitch = WC;
  if (STAGE) {
    const unsigned nb = (unsigned)(rows * WC);                          // <= 4 * kResizeStageBytes
    const unsigned pad = (unsigned)((uintptr_t)g & 15);
    const unsigned head = min((16u - pad) & 15u, nb);
    for (unsigned i = threadIdx.x; i < head; i += 256) stage[pad + i] = g[i];
    const unsigned nvec = (nb - head) / 16;
    for (unsigned v = threadIdx.x; v < nvec; v += 256)
      *reinterpret_cast<u32x4*>(stage + pad + head + 16 * v) = *reinterpret_cast<const u32x4*>(g + head + 16 * v);
    for (unsigned i = head + 16 * nvec + threadIdx.x; i < nb; i += 256) stage[pad + i] = g[i];
    __syncthreads();
    base = stage + pad;
  }
  for (size_t j = threadIdx.x; j < wC; j += 256) {
    const int xx = (int)(j / C), c = (int)(j - (size_t)xx * C);
    const int xmin = bounds[2 * xx], xmax = bounds[2 * xx + 1];
    const int32_t* k = coeffs + (size_t)xx * ksize;
    const uint8_t* p = base + (size_t)xmin * C + c;
    int acc[kResizeRows];
#pragma unroll
    for (int r = 0; r < kResizeRows; ++r) acc[r] = 1 << (RESAMPLE_PRECISION_BITS - 1);
    for (int x = 0; x < xmax; ++x) {
      const int kv = k[x];
#pragma unroll
      for (int r = 0; r < kResizeRows; ++r)
        if (STAGE || r < rows) acc[r] += (int)p[r * pitch + (size_t)x * C] * kv;     // staged: rows past the last read LDS only
    }
#pragma unroll
    for (int r = 0; r < kResizeRows; ++r)
      if (r < rows) dst[(size_t)(r0 + r) * wC + j] = resize_round(acc[r]);
  }
}

// Vertical pass, src [n, H, wC] -> dst [n, h, wC]: one thread per output byte, lanes along wC, so a wave reads adjacent bytes
// of one source row per tap and the coefficient is the same for the whole wave wherever it stays inside one output row.
__global__ __launch_bounds__(256) void resize_cols_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int n,
                                                          int H, int h, size_t wC, const int32_t* __restrict__ bounds,
                                                          const int32_t* __restrict__ coeffs, int ksize) {
  const size_t total = (size_t)n * h * wC;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const size_t line = i / wC, j = i - line * wC;
  const int yy = (int)(line % h);
  const size_t img = line / h;
  const int ymin = bounds[2 * yy], ymax = bounds[2 * yy + 1];
  const int32_t* k = coeffs + (size_t)yy * ksize;
  const uint8_t* p = src + (img * H + ymin) * wC + j;
  int acc = 1 << (RESAMPLE_PRECISION_BITS - 1);
  for (int y = 0; y < ymax; ++y) acc += (int)p[(size_t)y * wC] * k[y];
  dst[i] = resize_round(acc);
}

// Table: srad_resample_table (resize_u8) or srad_resample_table_f (resize_f32); they differ in the type of the taps only
template <class Table>
int check_table(const char* who, const char* axis, const Table* t, int in_size, int out_size) {
  SRAD_REQUIRE(t, "%s: the %s table is missing (the %s sizes differ: %d -> %d)", who, axis, axis, in_size, out_size);
  SRAD_REQUIRE(t->bounds && t->dev_bounds && t->dev_coeffs, "%s: null pointer in the %s table", who, axis);
  SRAD_REQUIRE(t->in_size == in_size && t->out_size == out_size && t->ksize >= 1,
               "%s: the %s table is for %d -> %d with %d taps, the images need %d -> %d", who, axis, t->in_size, t->out_size,
               t->ksize, in_size, out_size);
  SRAD_REQUIRE(resample_bounds_ok(t->bounds, in_size, out_size, t->ksize), "%s: the %s table's bounds leave the source (%d) or its %d taps",
               who, axis, in_size, t->ksize);
  return SRAD_OK;
}

// One pass of the float32 resize, one thread per output value: src [lines, in_size, inner] -> dst [lines, out_size, inner]
// along the middle axis.  The taps go in index order into one fp64 accumulator, product and sum rounded separately
// (contraction is off in this file), and the sum is rounded to float32 once: Pillow's 32bpc passes.  The grid carries the
// indices, so no thread divides.  ALONG (horizontal; lines = n * H, inner = 1): blockIdx.x is the line and the lanes run
// along the outputs of it.  Otherwise (vertical; lines = n, inner = w): blockIdx.x is (line, output) and the lanes run along
// `inner`, so a wave reads adjacent floats of one source row per tap and its bounds and taps are uniform.
constexpr int kResizeFAlongThreads = 64, kResizeFThreads = 256;
template <bool ALONG>
__global__ __launch_bounds__(ALONG ? kResizeFAlongThreads : kResizeFThreads) void resize_f32_pass_kernel(
    const float* __restrict__ src, float* __restrict__ dst, int in_size, int out_size, size_t inner, const int32_t* __restrict__ bounds,
    const double* __restrict__ coeffs, int ksize) {
  const size_t t = (size_t)blockIdx.y * blockDim.x + threadIdx.x;
  if (t >= (ALONG ? (size_t)out_size : inner)) return;
  const size_t line = ALONG ? blockIdx.x : blockIdx.x / out_size, j = ALONG ? 0 : t;
  const int xx = ALONG ? (int)t : (int)(blockIdx.x - line * out_size);
  const int xmin = bounds[2 * xx], xmax = bounds[2 * xx + 1];
  const double* k = coeffs + (size_t)xx * ksize;
  const float* p = src + (line * in_size + xmin) * inner + j;
  double ss = 0.0;
  for (int x = 0; x < xmax; ++x) ss += (double)p[(size_t)x * inner] * k[x];
  dst[(line * out_size + xx) * inner + j] = (float)ss;
}

}  // namespace

extern "C" int srad_resample_ksize(int in_size, int out_size, int filter, int* ksize) {
  SRAD_REQUIRE(ksize, "resample_ksize: null argument");
  SRAD_REQUIRE(resample_filter_known(filter), "resample_ksize: unknown filter %d (0 = LANCZOS, 1 = BICUBIC)", filter);
  const int k = resample_ksize(in_size, out_size, filter);
  SRAD_REQUIRE(k > 0, "resample_ksize: sizes %d -> %d are not supported (1 .. %d each)", in_size, out_size, (int)RESAMPLE_MAX_SIZE);
  *ksize = k;
  return SRAD_OK;
}

extern "C" int srad_resample_coeffs(int in_size, int out_size, int filter, int32_t* bounds, int32_t* coeffs) {
  SRAD_REQUIRE(bounds && coeffs, "resample_coeffs: null argument");
  int ksize = 0;
  SRAD_TRY(srad_resample_ksize(in_size, out_size, filter, &ksize));
  std::vector<double> scratch((size_t)ksize);
  SRAD_REQUIRE(resample_coeffs(in_size, out_size, filter, bounds, coeffs, scratch.data()) == ksize, "resample_coeffs: refused");
  return SRAD_OK;
}

extern "C" int srad_resize_u8(const uint8_t* src, int n, int H, int W, int C, uint8_t* dst, int h, int w,
                              const srad_resample_table* x_table, const srad_resample_table* y_table, uint8_t* tmp, void* stream) {
  SRAD_REQUIRE(src && dst, "resize_u8: null argument");
  SRAD_REQUIRE(n >= 1 && H >= 1 && W >= 1 && h >= 1 && w >= 1, "resize_u8: sizes must be >= 1, got n=%d %dx%d -> %dx%d", n, H, W, h, w);
  SRAD_REQUIRE(C >= 1 && C <= 4, "resize_u8: %d channels, 1 to 4 are supported", C);
  const bool pass_x = W != w, pass_y = H != h;
  if (pass_x) SRAD_TRY(check_table("resize_u8", "x", x_table, W, w));
  if (pass_y) SRAD_TRY(check_table("resize_u8", "y", y_table, H, h));
  SRAD_REQUIRE(!(pass_x && pass_y) || tmp, "resize_u8: null argument (both passes run: tmp [n,H,w,C] is needed)");
  const size_t src_bytes = (size_t)n * H * W * C, dst_bytes = (size_t)n * h * w * C, tmp_bytes = (size_t)n * H * w * C;
  SRAD_REQUIRE(!srad_byte_ranges_overlap(src, src_bytes, dst, dst_bytes), "resize_u8: dst overlaps src");
  if (pass_x && pass_y)
    SRAD_REQUIRE(!srad_byte_ranges_overlap(src, src_bytes, tmp, tmp_bytes) && !srad_byte_ranges_overlap(dst, dst_bytes, tmp, tmp_bytes),
                 "resize_u8: tmp overlaps src or dst");
  const unsigned long long row_blocks = ((unsigned long long)n * H + kResizeRows - 1) / kResizeRows;
  const unsigned long long col_blocks = (dst_bytes + 255) / 256;
  SRAD_REQUIRE(row_blocks < (1ull << 31) && col_blocks < (1ull << 31), "resize_u8: n=%d %dx%dx%d -> %dx%d needs more than 2^31 workgroups", n, H, W,
               C, h, w);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  SradProfScope prof(s, SRAD_K_RESIZE, 0.0, (double)src_bytes + (double)dst_bytes + (pass_x && pass_y ? 2.0 * tmp_bytes : 0.0));
  if (!pass_x && !pass_y) {
    SRAD_CHECK_HIP(hipMemcpyAsync(dst, src, src_bytes, hipMemcpyDeviceToDevice, s));
    return SRAD_OK;
  }
  const uint8_t* mid = src;
  if (pass_x) {
    uint8_t* out = pass_y ? tmp : dst;
    const long long rows_total = (long long)n * H;
    const size_t WC = (size_t)W * C;
    if (WC <= (size_t)kResizeStageBytes)
      hipLaunchKernelGGL(resize_rows_kernel<true>, dim3((unsigned)row_blocks), dim3(256), kResizeRows * WC + 16, s, src, out, rows_total, W, w, C,
                         x_table->dev_bounds, x_table->dev_coeffs, x_table->ksize);
    else
      hipLaunchKernelGGL(resize_rows_kernel<false>, dim3((unsigned)row_blocks), dim3(256), 0, s, src, out, rows_total, W, w, C,
                         x_table->dev_bounds, x_table->dev_coeffs, x_table->ksize);
    SRAD_CHECK_HIP(hipGetLastError());
    mid = out;
  }
  if (pass_y) {
    hipLaunchKernelGGL(resize_cols_kernel, dim3((unsigned)col_blocks), dim3(256), 0, s, mid, dst, n, H, h, (size_t)w * C, y_table->dev_bounds,
                       y_table->dev_coeffs, y_table->ksize);
    SRAD_CHECK_HIP(hipGetLastError());
  }
  return SRAD_OK;
}

extern "C" int srad_resample_ksize_f64(int in_size, int out_size, int filter, int* ksize) {
  SRAD_REQUIRE(ksize, "resample_ksize_f64: null argument");
  SRAD_REQUIRE(resample_filter_known_f(filter), "resample_ksize_f64: unknown filter %d (0 = LANCZOS, 1 = BICUBIC, 2 = BILINEAR)", filter);
  const int k = resample_ksize_f(in_size, out_size, filter);
  SRAD_REQUIRE(k > 0, "resample_ksize_f64: sizes %d -> %d are not supported (1 .. %d each)", in_size, out_size, (int)RESAMPLE_MAX_SIZE);
  *ksize = k;
  return SRAD_OK;
}

extern "C" int srad_resample_coeffs_f64(int in_size, int out_size, int filter, int32_t* bounds, double* coeffs) {
  SRAD_REQUIRE(bounds && coeffs, "resample_coeffs_f64: null argument");
  int ksize = 0;
  SRAD_TRY(srad_resample_ksize_f64(in_size, out_size, filter, &ksize));
  SRAD_REQUIRE(resample_coeffs_f(in_size, out_size, filter, bounds, coeffs) == ksize, "resample_coeffs_f64: refused");
  return SRAD_OK;
}

extern "C" int srad_resize_f32(const float* src, int n, int H, int W, float* dst, int h, int w, const srad_resample_table_f* x_table,
                               const srad_resample_table_f* y_table, float* tmp, void* stream) {
  SRAD_REQUIRE(src && dst, "resize_f32: null argument");
  SRAD_REQUIRE(n >= 1 && H >= 1 && W >= 1 && h >= 1 && w >= 1, "resize_f32: sizes must be >= 1, got n=%d %dx%d -> %dx%d", n, H, W, h, w);
  const bool pass_x = W != w, pass_y = H != h;
  if (pass_x) SRAD_TRY(check_table("resize_f32", "x", x_table, W, w));
  if (pass_y) SRAD_TRY(check_table("resize_f32", "y", y_table, H, h));
  SRAD_REQUIRE(!(pass_x && pass_y) || tmp, "resize_f32: null argument (both passes run: tmp [n,H,w] is needed)");
  const size_t src_n = (size_t)n * H * W, dst_n = (size_t)n * h * w, tmp_n = (size_t)n * H * w;
  SRAD_REQUIRE(!srad_byte_ranges_overlap(src, 4 * src_n, dst, 4 * dst_n), "resize_f32: dst overlaps src");
  if (pass_x && pass_y)
    SRAD_REQUIRE(!srad_byte_ranges_overlap(src, 4 * src_n, tmp, 4 * tmp_n) && !srad_byte_ranges_overlap(dst, 4 * dst_n, tmp, 4 * tmp_n),
                 "resize_f32: tmp overlaps src or dst");
  // the grids: (lines, outputs / 64) threads of 64 and (lines * outputs, w / 256) threads of 256; x threads < 2^32, y <= 65535
  const unsigned long long x_lines = (unsigned long long)n * H, y_rows = (unsigned long long)n * h;
  const unsigned long long x_cols = ((unsigned long long)w + kResizeFAlongThreads - 1) / kResizeFAlongThreads;
  const unsigned long long y_cols = ((unsigned long long)w + kResizeFThreads - 1) / kResizeFThreads;
  SRAD_REQUIRE((!pass_x || (x_lines * kResizeFAlongThreads < (1ull << 32) && x_cols <= 65535)) &&
                   (!pass_y || (y_rows * kResizeFThreads < (1ull << 32) && y_cols <= 65535)),
               "resize_f32: n=%d %dx%d -> %dx%d is more than one launch takes (n * H < 2^26, n * h < 2^24, w < 2^22)", n, H, W, h, w);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  SradProfScope prof(s, SRAD_K_RESIZE, 0.0, 4.0 * ((double)src_n + (double)dst_n + (pass_x && pass_y ? 2.0 * tmp_n : 0.0)));
  if (!pass_x && !pass_y) {
    SRAD_CHECK_HIP(hipMemcpyAsync(dst, src, 4 * src_n, hipMemcpyDeviceToDevice, s));
    return SRAD_OK;
  }
  const float* mid = src;
  if (pass_x) {
    float* out = pass_y ? tmp : dst;
    hipLaunchKernelGGL(resize_f32_pass_kernel<true>, dim3((unsigned)x_lines, (unsigned)x_cols), dim3(kResizeFAlongThreads), 0, s, src, out, W, w,
                       (size_t)1, x_table->dev_bounds, x_table->dev_coeffs, x_table->ksize);
    SRAD_CHECK_HIP(hipGetLastError());
    mid = out;
  }
  if (pass_y) {
    hipLaunchKernelGGL(resize_f32_pass_kernel<false>, dim3((unsigned)y_rows, (unsigned)y_cols), dim3(kResizeFThreads), 0, s, mid, dst, H, h,
                       (size_t)w, y_table->dev_bounds, y_table->dev_coeffs, y_table->ksize);
    SRAD_CHECK_HIP(hipGetLastError());
  }
  return SRAD_OK;
}
