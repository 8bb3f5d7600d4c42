// mlp_fold.h - the layout of a Swin block's folded second half.  Host-only: no HIP include.
//
// In eval mode nothing non-linear sits between mlp.fc2 and the RDG's 1 x 1 adjust conv (reference src/drct.py:184-190, 388-396,
// 509-510), and the block's output x2 is read by that conv alone:
//     adjust(x1 + fc2(h) + b2) = A x1 + (A W2) h + (A b2 + b_a)        x1 = x + proj(attn), h = GELU(fc1(LayerNorm2(x1)))
// so for inference fc2 and adjust are ONE GEMM over k = [x1 | h] with `no` output columns:
//     Wf = [ A, zero-padded to 32 KC columns | A W2, zero-padded to 32 KCM columns ]   (no rows),   bf = A b2 + b_a
// KC = ceil(d / 32), KCM = ceil(hidden / 32): both parts start on a 32-wide k chunk, so the kernels read chunks [0, KC) from
// their bf16(x1) tile and chunks [KC, KC + KCM) from the hidden tile.  The products accumulate in fp64 in index order and are
// rounded to fp32 once (kernels_mlp_fold.hip); Wf is then packed like every other Linear weight (srad_launch_pack_weight_frag:
// its k extent is a multiple of 32 by construction).
#pragma once
#include <stddef.h>

// Region of one block's fold (byte offsets from a 256-byte aligned base): the fp32 sources in PyTorch layout, the composed
// fp32 matrix Wf [no][32 (KC + KCM)], its bf16 fragment pack [ceil128(no) / 16][KC + KCM][16 x 32] and the fp32 bias [no].
struct MlpFoldLayout {
  int d, m, no, kc, kcm, kf;     // block dim, hidden, adjust outputs; k chunks of d / of hidden; columns of Wf = 32 (kc + kcm)
  size_t w2, b2, a, ba;          // mlp.fc2.weight [d][m], mlp.fc2.bias [d], adjust.weight [no][d], adjust.bias [no]
  size_t wf, pack, bias, bytes;
};
inline MlpFoldLayout mf_layout(int d, int m, int no) {
  MlpFoldLayout l{};
  l.d = d; l.m = m; l.no = no; l.kc = (d + 31) / 32; l.kcm = (m + 31) / 32; l.kf = 32 * (l.kc + l.kcm);
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
  l.w2 = take((size_t)d * m * 4); l.b2 = take((size_t)d * 4);
  l.a = take((size_t)no * d * 4); l.ba = take((size_t)no * 4);
  l.wf = take((size_t)no * l.kf * 4);
  l.pack = take((size_t)((no + 127) / 128 * 128) * l.kf * 2);
  l.bias = take((size_t)no * 4);
  l.bytes = off;
  return l;
}
// column of Wf that multiplies x1[i] / h[j]
inline int mf_col_x1(const MlpFoldLayout&, int i) { return i; }
inline int mf_col_h(const MlpFoldLayout& l, int j) { return 32 * l.kc + j; }
