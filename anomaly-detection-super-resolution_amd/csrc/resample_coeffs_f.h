// resample_coeffs_f.h - the double coefficient tables of a float32 image resize: plain host arithmetic, no HIP.
//
// Pillow resamples mode-F (float32) images with the taps of precompute_coeffs as they are, in double: they are divided by their
// sum and NOT brought to fixed point (src/libImaging/Resample.c: precompute_coeffs and the 32bpc passes).  This header restates
// the table half of that for one axis: (in_size, out_size, filter) -> ksize, bounds[out][2] = (xmin, xmax) as in
// resample_coeffs.h, and the taps as double (coeffs[out][ksize], zero from xmax on), in Pillow's order of operations.  One pass
// along an axis is
//     ss = 0.0;  for x < xmax:  ss += (double)src[xmin + x] * k[x];      (one product, one sum, no fused multiply-add)
//     out = (float)ss
// (resample_pass_value_f below, shared with the check program).  The horizontal pass comes first and is rounded to float32.
// The filters are those of resample_coeffs.h plus BILINEAR (id 2), which only the functions here accept: the 8-bit functions
// keep refusing it.  It compiles with any C++17 compiler: tests/host/resample_f_check.cpp includes only this header and runs
// under sanitizers.
#pragma once
#include "resample_coeffs.h"

enum { RESAMPLE_BILINEAR = 2, RESAMPLE_FILTERS_F = 3 };

static inline double resample_bilinear(double x) {
  if (x < 0.0) x = -x;
  if (x < 1.0) return 1.0 - x;
  return 0.0;
}

static inline bool resample_filter_known_f(int filter) { return filter >= 0 && filter < RESAMPLE_FILTERS_F; }
static inline double resample_filter_support_f(int filter) { return filter == RESAMPLE_BILINEAR ? 1.0 : resample_filter_support(filter); }
static inline double resample_filter_f(int filter, double x) { return filter == RESAMPLE_BILINEAR ? resample_bilinear(x) : resample_filter(filter, x); }

// taps per output index; 0 for arguments resample_coeffs_f refuses
static inline int resample_ksize_f(int in_size, int out_size, int filter) {
  if (in_size < 1 || out_size < 1 || in_size > RESAMPLE_MAX_SIZE || out_size > RESAMPLE_MAX_SIZE || !resample_filter_known_f(filter)) return 0;
  double filterscale = (double)in_size / out_size;
  if (filterscale < 1.0) filterscale = 1.0;
  const double support = resample_filter_support_f(filter) * filterscale;
  return (int)ceil(support) * 2 + 1;
}

// Fills bounds[out_size][2] and coeffs[out_size][ksize].  Returns ksize, 0 for refused arguments (nothing is written then).
static inline int resample_coeffs_f(int in_size, int out_size, int filter, int32_t* bounds, double* coeffs) {
  const int ksize = resample_ksize_f(in_size, out_size, filter);
  if (!ksize || !bounds || !coeffs) return 0;
  const double scale = (double)in_size / out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = resample_filter_support_f(filter) * filterscale;
  const double ss = 1.0 / filterscale;
  for (int xx = 0; xx < out_size; ++xx) {
    const double center = (xx + 0.5) * scale;
    double ww = 0.0;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    double* k = coeffs + (size_t)xx * ksize;
    for (int x = 0; x < xmax; ++x) {
      const double w = resample_filter_f(filter, (x + xmin - center + 0.5) * ss);
      k[x] = w;
      ww += w;
    }
    for (int x = 0; x < xmax; ++x)
      if (ww != 0.0) k[x] /= ww;
    for (int x = xmax; x < ksize; ++x) k[x] = 0.0;
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = xmax;
  }
  return ksize;
}

// One output value of a pass: `src` points at the first source value of this output's line, `stride` apart along the axis.
static inline float resample_pass_value_f(const float* src, size_t stride, const int32_t* bound, const double* k) {
  double ss = 0.0;
  for (int x = 0; x < bound[1]; ++x) ss += (double)src[(size_t)(bound[0] + x) * stride] * k[x];
  return (float)ss;
}
