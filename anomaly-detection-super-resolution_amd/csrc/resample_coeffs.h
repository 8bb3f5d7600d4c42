// resample_coeffs.h - the fixed-point coefficient tables of an 8-bit image resize: plain host arithmetic, no HIP.
//
// Pillow resamples 8-bit images in fixed point (src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc and the
// 8bpc passes).  This header restates the table half of that for one axis: (in_size, out_size, filter) -> ksize, the first
// source index and the tap count of every output index (bounds[out][2] = xmin, xmax) and the taps as int32 with 22 fractional
// bits (coeffs[out][ksize], zero from xmax on).  All of it in double and in Pillow's order of operations, so the tables - and
// with them every pixel of the passes in kernels_resize.hip - equal Pillow's.  One pass along an axis is
//     acc = (1 << 21) + sum_{x < xmax} src[xmin + x] * k[x]      (int32)
//     out = clamp(acc >> 22, 0, 255)                              (arithmetic shift)
// (resample_pass_pixel below, shared with the check program).  The horizontal pass comes first and is rounded to u8.
// It compiles with any C++17 compiler: tests/host/resample_check.cpp includes only this header and runs under sanitizers.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__clang__)
#pragma STDC FP_CONTRACT OFF   // a fused multiply-add would round differently from Pillow's build
#endif

enum { RESAMPLE_LANCZOS = 0, RESAMPLE_BICUBIC = 1, RESAMPLE_FILTERS = 2 };
enum { RESAMPLE_PRECISION_BITS = 32 - 8 - 2 };

static inline double resample_sinc(double x) {
  if (x == 0.0) return 1.0;
  x = x * 3.14159265358979323846;
  return sin(x) / x;
}

static inline double resample_lanczos(double x) {
  if (-3.0 <= x && x < 3.0) return resample_sinc(x) * resample_sinc(x / 3);
  return 0.0;
}

static inline double resample_bicubic(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

static inline bool resample_filter_known(int filter) { return filter >= 0 && filter < RESAMPLE_FILTERS; }
static inline double resample_filter_support(int filter) { return filter == RESAMPLE_BICUBIC ? 2.0 : 3.0; }
static inline double resample_filter(int filter, double x) { return filter == RESAMPLE_BICUBIC ? resample_bicubic(x) : resample_lanczos(x); }

// in_size / out_size limit: the tables are indexed with int, and out_size * ksize (about 6 * in_size or 7 * out_size at most)
// stays far below 2^31
enum { RESAMPLE_MAX_SIZE = 1 << 20 };

// taps per output index; 0 for arguments resample_coeffs refuses
static inline int resample_ksize(int in_size, int out_size, int filter) {
  if (in_size < 1 || out_size < 1 || in_size > RESAMPLE_MAX_SIZE || out_size > RESAMPLE_MAX_SIZE || !resample_filter_known(filter)) return 0;
  double filterscale = (double)in_size / out_size;
  if (filterscale < 1.0) filterscale = 1.0;
  const double support = resample_filter_support(filter) * filterscale;
  return (int)ceil(support) * 2 + 1;
}

// Fills bounds[out_size][2] and coeffs[out_size][ksize]; `scratch` holds ksize doubles.  Returns ksize, 0 for refused arguments.
static inline int resample_coeffs(int in_size, int out_size, int filter, int32_t* bounds, int32_t* coeffs, double* scratch) {
  const int ksize = resample_ksize(in_size, out_size, filter);
  if (!ksize || !bounds || !coeffs || !scratch) return 0;
  const double scale = (double)in_size / out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = resample_filter_support(filter) * filterscale;
  const double ss = 1.0 / filterscale;
  for (int xx = 0; xx < out_size; ++xx) {
    const double center = (xx + 0.5) * scale;
    double ww = 0.0;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    for (int x = 0; x < xmax; ++x) {
      const double w = resample_filter(filter, (x + xmin - center + 0.5) * ss);
      scratch[x] = w;
      ww += w;
    }
    int32_t* k = coeffs + (size_t)xx * ksize;
    for (int x = 0; x < ksize; ++x) {
      double w = 0.0;
      if (x < xmax) w = ww != 0.0 ? scratch[x] / ww : scratch[x];
      k[x] = w < 0 ? (int32_t)(-0.5 + w * (1 << RESAMPLE_PRECISION_BITS)) : (int32_t)(0.5 + w * (1 << RESAMPLE_PRECISION_BITS));
    }
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = xmax;
  }
  return ksize;
}

// Does every output index read inside [0, in_size) and inside its ksize taps?  (what srad_resize_u8 checks before it launches)
static inline bool resample_bounds_ok(const int32_t* bounds, int in_size, int out_size, int ksize) {
  for (int xx = 0; xx < out_size; ++xx) {
    const int64_t xmin = bounds[2 * xx], xmax = bounds[2 * xx + 1];
    if (xmin < 0 || xmax < 0 || xmax > ksize || xmin + xmax > in_size) return false;
  }
  return true;
}

// One output value of a pass: `src` points at the first source value of this output's line, `stride` apart along the axis.
static inline uint8_t resample_pass_pixel(const uint8_t* src, size_t stride, const int32_t* bound, const int32_t* k) {
  int32_t acc = 1 << (RESAMPLE_PRECISION_BITS - 1);
  for (int x = 0; x < bound[1]; ++x) acc += (int32_t)src[(size_t)(bound[0] + x) * stride] * k[x];
  acc >>= RESAMPLE_PRECISION_BITS;
  return (uint8_t)(acc < 0 ? 0 : (acc > 255 ? 255 : acc));
}
