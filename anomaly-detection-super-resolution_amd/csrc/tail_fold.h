// tail_fold.h - the index algebra of DRCT's folded output end.  Host-only core: no HIP include, so a plain C++
// program can use it (tests/host/tail_fold_check.cpp); the device builder (kernels_tail_fold.hip) calls the same functions.
//
// Everything after conv_before_upsample's LeakyReLU is linear (reference src/drct.py:694-713, 842-847, 894-895):
//     y = conv_last( PixelShuffle(2)( up_1( PixelShuffle(2)( up_0(c2) ) ) ) )           (scale 4; scale 2 has up_0 only)
// so the s x s HR pixels of an LR pixel are one 5 x 5 convolution of c2 with num_feat inputs and N = s s in_chans outputs,
// output oc = (c s + py) s + px.  Zero padding is the one complication: conv_last and up_1 pad their own, finer inputs, and a
// product whose intermediate position lies outside its map must be dropped.  That happens only for LR pixels of the first or
// last row / column, and per axis on its own, so the folded weights and bias depend on a position class per axis
// (first / interior / last): nine classes.  Maps need H, W >= 2 (a pixel that is first and last has no class).
//
// Per axis, with t1 the conv_last tap, t2 the up_1 tap, t3 the up_0 tap (0..2 each, offset t - 1) and p the sub-pixel:
//     r2 = p + t1 - 1                    position at HR, relative to s y          dropped when outside [0, s H)
//     i2 = r2 & 1, q2 = r2 >> 1          PixelShuffle phase / position of up_1's output at 2 H
//     r1 = q2 + t2 - 1                   position in up_1's input, relative to 2 y dropped when outside [0, 2 H)
//     u  = r1 + 2 in 0..5                ("head": everything up to here is independent of up_0)
//     i1 = u & 1, q1 = (u - 2) >> 1      PixelShuffle phase / LR pixel of up_0's output, relative to y
//     d  = q1 + t3 - 1 in -2..2          the folded tap (outside the image: ordinary zero padding of the folded convolution)
// The conv channel a PixelShuffle reads for output channel g at phases (iy, ix) is 4 g + 2 iy + ix.  At scale 2 the head is
// r1 = p + t1 - 1 alone.  The fold is composed in two steps: head[cls][oc][uy][ux][h] (conv_last o up_1 at up_0's output), then
// wf[cls][oc][dy][dx][f] = sum over (u, t3) landing on d of head . up_0.
#pragma once
#include <stddef.h>

#if defined(__HIPCC__)
#define TF_HD __host__ __device__
#else
#define TF_HD
#endif

enum { TF_FIRST = 0, TF_INTERIOR = 1, TF_LAST = 2 };
enum { TF_RADIUS = 2, TF_K = 5, TF_TAPS = 25, TF_U = 6, TF_CLASSES = 9 };

TF_HD inline int tf_class(int pos, int size) { return pos == 0 ? TF_FIRST : (pos == size - 1 ? TF_LAST : TF_INTERIOR); }
// is the position `rel` (relative to r * y, at r times the LR resolution) inside its map for an LR pixel of class cls?
TF_HD inline bool tf_inside(int cls, int rel, int r) { return !(cls == TF_FIRST && rel < 0) && !(cls == TF_LAST && rel >= r); }
// is the folded tap d inside the LR image?  (the weights of the others are stored as zeros; the kernel zeroes their input)
TF_HD inline bool tf_tap_in_image(int cls, int d) { return !(cls == TF_FIRST && d < 0) && !(cls == TF_LAST && d > 0); }
TF_HD inline int tf_head_taps(int scale) { return scale == 4 ? 3 : 1; }      // values t2 runs over
// Head of a path: sub-pixel p, conv_last tap t1, up_1 tap t2 (0 at scale 2) -> position u at up_0's output and the phase i2
// of the PixelShuffle between up_1 and conv_last (-1 at scale 2).  false: an intermediate position is outside its map.
TF_HD inline bool tf_head(int scale, int cls, int p, int t1, int t2, int* u, int* i2) {
  const int r2 = p + t1 - 1;
  if (!tf_inside(cls, r2, scale)) return false;
  if (scale == 2) { *u = r2 + 2; *i2 = -1; return true; }
  const int r1 = (r2 >> 1) + t2 - 1;
  if (!tf_inside(cls, r1, 2)) return false;
  *u = r1 + 2; *i2 = r2 & 1;
  return true;
}
// Tail of a path: from position u to the folded tap d -> PixelShuffle phase i1 and up_0 tap t3.  false: no tap lands there.
TF_HD inline bool tf_tail(int u, int d, int* i1, int* t3) {
  const int t = d - ((u - 2) >> 1) + 1;
  *i1 = u & 1; *t3 = t;
  return t >= 0 && t <= 2;
}

// Device / arena layout of a fold (byte offsets from a 256-byte aligned base): the fp32 sources in PyTorch layout, the head
// (scratch of the build), the fp32 fold wf [9][N][25][F], the bf16 pack in the kernel's fragment order
// [9][NT][25][F / 32][64 lanes][8] (lane = 16 fq + fr holds outputs row 16 nt + fr, channels 32 j + 8 fq .. + 7; rows >= N zero)
// and the fp32 bias table [9][16 NT].
struct TailFoldLayout {
  int F, C, scale, N, NT;
  size_t w_up0, b_up0, w_up1, b_up1, w_last, b_last, head, wf, pack, bias, bytes;
};
inline TailFoldLayout tf_layout(int F, int C, int scale) {
  TailFoldLayout l{};
  l.F = F; l.C = C; l.scale = scale; l.N = scale * scale * C; l.NT = (l.N + 15) / 16;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
  l.w_up0 = take((size_t)4 * F * F * 9 * 4); l.b_up0 = take((size_t)4 * F * 4);
  l.w_up1 = take(scale == 4 ? (size_t)4 * F * F * 9 * 4 : 0); l.b_up1 = take(scale == 4 ? (size_t)4 * F * 4 : 0);
  l.w_last = take((size_t)C * F * 9 * 4); l.b_last = take((size_t)C * 4);
  l.head = take((size_t)TF_CLASSES * l.N * TF_U * TF_U * F * 4);
  l.wf = take((size_t)TF_CLASSES * l.N * TF_TAPS * F * 4);
  l.pack = take((size_t)TF_CLASSES * l.NT * 16 * TF_TAPS * F * 2);
  l.bias = take((size_t)TF_CLASSES * l.NT * 16 * 4);
  l.bytes = off;
  return l;
}

// ---- the fold on the host, in T (the tests use double): the literal sum over every path, no intermediate ----
template <class T>
struct TfWeights {
  int F, C, scale;
  const T *w_up0, *b_up0;      // upsample.0 [4F][F][3][3], [4F]
  const T *w_up1, *b_up1;      // upsample.2, scale 4 only
  const T *w_last, *b_last;    // conv_last [C][F][3][3], [C]
};

// wf [9][N][25][F]: class cy * 3 + cx, output (c s + py) s + px, tap (dy + 2) * 5 + dx + 2
template <class T>
void tf_fold_weights(const TfWeights<T>& w, T* wf) {
  const int F = w.F, s = w.scale, N = s * s * w.C, n2 = tf_head_taps(s);
  for (size_t i = 0; i < (size_t)TF_CLASSES * N * TF_TAPS * F; ++i) wf[i] = T(0);
  for (int cls = 0; cls < TF_CLASSES; ++cls)
    for (int oc = 0; oc < N; ++oc) {
      const int cy = cls / 3, cx = cls % 3, px = oc % s, py = (oc / s) % s, c = oc / (s * s);
      for (int t1y = 0; t1y < 3; ++t1y) for (int t2y = 0; t2y < n2; ++t2y) for (int t1x = 0; t1x < 3; ++t1x) for (int t2x = 0; t2x < n2; ++t2x) {
        int uy, ux, i2y, i2x;
        if (!tf_head(s, cy, py, t1y, t2y, &uy, &i2y) || !tf_head(s, cx, px, t1x, t2x, &ux, &i2x)) continue;
        for (int dy = -TF_RADIUS; dy <= TF_RADIUS; ++dy) for (int dx = -TF_RADIUS; dx <= TF_RADIUS; ++dx) {
          int i1y, i1x, t3y, t3x;
          if (!tf_tail(uy, dy, &i1y, &t3y) || !tf_tail(ux, dx, &i1x, &t3x)) continue;
          if (!tf_tap_in_image(cy, dy) || !tf_tap_in_image(cx, dx)) continue;
          T* const out = wf + (((size_t)cls * N + oc) * TF_TAPS + (dy + 2) * TF_K + dx + 2) * F;
          for (int h = 0; h < F; ++h) {
            T head;
            if (s == 4) {
              head = T(0);
              for (int g = 0; g < F; ++g)
                head += w.w_last[(c * F + g) * 9 + t1y * 3 + t1x] * w.w_up1[((size_t)(g * 4 + i2y * 2 + i2x) * F + h) * 9 + t2y * 3 + t2x];
            } else {
              head = w.w_last[(c * F + h) * 9 + t1y * 3 + t1x];
            }
            const T* const w0 = w.w_up0 + ((size_t)(h * 4 + i1y * 2 + i1x) * F) * 9 + t3y * 3 + t3x;
            for (int f = 0; f < F; ++f) out[f] += head * w0[(size_t)f * 9];
          }
        }
      }
    }
}

// bias [9][N]: conv_last's bias, up_1's through every conv_last tap that stays inside, up_0's through every head that does
template <class T>
void tf_fold_bias(const TfWeights<T>& w, T* bias) {
  const int F = w.F, s = w.scale, N = s * s * w.C, n2 = tf_head_taps(s);
  for (int cls = 0; cls < TF_CLASSES; ++cls)
    for (int oc = 0; oc < N; ++oc) {
      const int cy = cls / 3, cx = cls % 3, px = oc % s, py = (oc / s) % s, c = oc / (s * s);
      T acc = w.b_last[c];
      for (int t1y = 0; t1y < 3; ++t1y) for (int t1x = 0; t1x < 3; ++t1x) {
        const int r2y = py + t1y - 1, r2x = px + t1x - 1;
        if (!tf_inside(cy, r2y, s) || !tf_inside(cx, r2x, s)) continue;
        if (s == 4)
          for (int g = 0; g < F; ++g) acc += w.w_last[(c * F + g) * 9 + t1y * 3 + t1x] * w.b_up1[g * 4 + (r2y & 1) * 2 + (r2x & 1)];
        for (int t2y = 0; t2y < n2; ++t2y) for (int t2x = 0; t2x < n2; ++t2x) {
          int uy, ux, i2y, i2x;
          if (!tf_head(s, cy, py, t1y, t2y, &uy, &i2y) || !tf_head(s, cx, px, t1x, t2x, &ux, &i2x)) continue;
          for (int h = 0; h < F; ++h) {
            T head;
            if (s == 4) {
              head = T(0);
              for (int g = 0; g < F; ++g)
                head += w.w_last[(c * F + g) * 9 + t1y * 3 + t1x] * w.w_up1[((size_t)(g * 4 + i2y * 2 + i2x) * F + h) * 9 + t2y * 3 + t2x];
            } else {
              head = w.w_last[(c * F + h) * 9 + t1y * 3 + t1x];
            }
            acc += head * w.b_up0[h * 4 + (uy & 1) * 2 + (ux & 1)];
          }
        }
      }
      bias[cls * N + oc] = acc;
    }
}

// Applies a fold to c2 [H][W][F] by class: out [C][s H][s W].  cls_override >= 0 forces that class everywhere (the tests show
// that a wrong class is detected).
template <class T>
void tf_apply(const T* wf, const T* bias, int F, int C, int s, const T* c2, int H, int W, T* out, int cls_override = -1) {
  const int N = s * s * C;
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const int cls = cls_override >= 0 ? cls_override : tf_class(y, H) * 3 + tf_class(x, W);
      for (int oc = 0; oc < N; ++oc) {
        const int px = oc % s, py = (oc / s) % s, c = oc / (s * s);
        T acc = bias[cls * N + oc];
        for (int dy = -TF_RADIUS; dy <= TF_RADIUS; ++dy) for (int dx = -TF_RADIUS; dx <= TF_RADIUS; ++dx) {
          const int yy = y + dy, xx = x + dx;
          if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
          const T* const wr = wf + (((size_t)cls * N + oc) * TF_TAPS + (dy + 2) * TF_K + dx + 2) * F;
          const T* const in = c2 + ((size_t)yy * W + xx) * F;
          for (int f = 0; f < F; ++f) acc += wr[f] * in[f];
        }
        out[((size_t)c * s * H + s * y + py) * s * W + s * x + px] = acc;
      }
    }
}
