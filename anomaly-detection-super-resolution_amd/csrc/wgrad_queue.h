// wgrad_queue.h - the split-K gradient queue's bookkeeping: plain structs and host arithmetic, no HIP.
//
// Every weight gradient, LayerNorm dgamma / dbeta and attention bias-table gradient of a backward pass writes partial sums
// into one caller-owned workspace and queues a reduce item; wgrad_reduce_kernel (kernels_wgrad.hip) sums a batch of items
// with one launch.  This header holds the structs those kernels receive and EVERY decision the queue makes - where a region
// goes, when a batch is reduced and which of its items, what a refusal is - as inline host functions that launch nothing:
// "reduce this batch now" is a callable the caller passes (kernels_wgrad.hip passes the launch, tests/host/wgrad_queue_check.cpp
// a recorder).  It compiles with any C++17 compiler, so the offsets and counts are tested on the CPU under sanitizers.
// Nothing outside this header and kernels_wgrad.hip writes a WgradQueue field.
//
// The rules ("The split-K queue's flush rules"):
//  * A reservation (wgrad_queue_reserve) takes `need` floats and room for `nitems` batch entries.  It bumps `used`; when the
//    batch or the workspace is full it flushes first (reason BATCH resp. WS; both at once counts as BATCH).
//  * A deferred layer's item is PENDING from the moment it is queued until wgrad_queue_deferred_launched: its partials are
//    not written yet.  A flush reduces only the items that are not pending; the pending ones stay, with their regions.
//  * After such a flush `used` is the end of the highest pending region, and what the reduced items held below it is handed
//    out again first-fit from the low end ([hole_lo, hole_end) minus the pending regions; the cursor only moves up).  The holes
//    are forgotten once the deferred launch has gone out.  A flush with nothing pending restarts at 0.
#pragma once
#include <stddef.h>

typedef struct ihipStream_t* hipStream_t;   // as hip_runtime_api.h declares it: the queue only stores one

#if defined(__HIPCC__)
#define SRAD_WGRAD_HD __host__ __device__ __attribute__((always_inline))
#else
#define SRAD_WGRAD_HD
#endif

// Weight gradient of a Linear / conv layer, accumulated (+=) into the PyTorch-layout fp32 tensor:
//   dW[n][c][tap] += alpha * sum_m rs(m) * dY[m][ycol0 + n] * A(m, tap, c),   db[n] += alpha * sum_m rs(m) * dY[m][ycol0 + n]
// with A the forward's row gather (identity for Linear, the 3x3 / strided window for convs).
struct WgradParams {
  const float* dY; int ldy, ycol0;
  const float* X; int ldx;
  int M, N, Cin, ntaps;        // N, Cin: padded to multiples of 4 as stored in dY / X
  int n_real, cin_real;        // extents of dW (columns/rows beyond are padding and never written)
  int grp_real, grp_pad;       // grp_pad > 0: X's channels are groups of grp_pad holding grp_real real ones each (DRN x8 level 0)
  int Hi, Wi, Ho, Wo, stride;  // conv geometry (M = B*Ho*Wo); ignored for ntaps == 1 && stride == 1
  const float* row_scale; int rps;
  float alpha;
  float* dW;                   // [n_real][cin_real][ntaps]
  float* db;                   // [n_real] or null
  int x_bf16, dy_bf16;         // operand storage: 1 = the pointer is a __bf16 array (ld in elements); Linear layers on the
                               // mask-free (FULL) bf16 path only.  A bf16 dY is already multiplied by its DropPath factor.
};

#define SRAD_WGRAD_BATCH 12
struct WgradReduceItem {
  float* dW; float* db; const float* part;
  int n_real, cin_real, ntaps, tn, tc, ksplit;
  int tile0;                     // first reduce tile of the item in its launch: set when the batch to launch is assembled
  int grp_real, grp_pad;         // as WgradParams
  float alpha;
  int wc;                        // C > 0: one C x C partial tile per tap (wgrad80_kernel, wgrad_conv9_kernel), row-major + C bias sums;
                                 // then tn = reduce tiles per tap, tc = float4 per reduce workgroup
};
struct WgradReduceBatch { WgradReduceItem it[SRAD_WGRAD_BATCH]; int count; };   // what wgrad_reduce_kernel receives
#define SRAD_WGRAD_MULTI 5
struct WgradMulti {                            // Linear layers whose weight-gradient kernels go out as one launch
  WgradParams p[SRAD_WGRAD_MULTI];
  float* part[SRAD_WGRAD_MULTI];
  int ksplit[SRAD_WGRAD_MULTI], tn[SRAD_WGRAD_MULTI], tc[SRAD_WGRAD_MULTI], blk0[SRAD_WGRAD_MULTI], nblk[SRAD_WGRAD_MULTI];
  int count;
};
// why a reduce launch happened (include/srad.h SRAD_WQ_FLUSH_*): asked for, or made by a reservation that found the batch /
// the workspace full.  Host bookkeeping only: what a test asserts to know which path it exercised.
enum { SRAD_WGRAD_FLUSH_EXPLICIT = 0, SRAD_WGRAD_FLUSH_BATCH = 1, SRAD_WGRAD_FLUSH_WS = 2 };
#define SRAD_WGRAD_LOG 64
struct WgradFlushLog { int count = 0; int by_why[3] = {0, 0, 0}; unsigned char why[SRAD_WGRAD_LOG] = {}; };   // the first SRAD_WGRAD_LOG reasons in order

// What the queue refuses, as negative codes (0 = fine; a positive value is the reduce callable's own error, passed through).
enum {
  SRAD_WGRAD_TOO_SMALL = -1,     // one reservation larger than the whole workspace (or no workspace)
  SRAD_WGRAD_NO_ROOM = -2,       // does not fit beside the pending layers even after a flush
  SRAD_WGRAD_BAD_NITEMS = -3,    // more items in one reservation than a batch can always take
  SRAD_WGRAD_NOT_EMPTY = -4,     // rebind with something queued, pending or reserved
};

struct WgradRegion { size_t off = 0, floats = 0; };   // [off, off + floats) of the workspace

// A queue lives on the host for the duration of one backward pass; flush before anyone reads the gradients.
struct WgradQueue {
  float* ws = nullptr; size_t ws_floats = 0;   // caller-owned device workspace, 16-byte aligned
  size_t used = 0;                             // everything at or above is free
  size_t hole_lo = 0, hole_end = 0;            // [hole_lo, hole_end) minus the pending regions: free space a flush left below `used`
  // the queued items: what the kernel will get (tile0 not yet set), and beside each its reduce tiles, the region its partials
  // lie in (two column-sum items may share one) and whether they are still to be written
  WgradReduceBatch batch{};
  int ntiles[SRAD_WGRAD_BATCH] = {};
  WgradRegion region[SRAD_WGRAD_BATCH] = {};
  bool pending[SRAD_WGRAD_BATCH] = {};
  // the deferred layers (multi.count of them pending, split or not) and their launch's statistics
  WgradMulti multi{};
  double multi_flops = 0, multi_bytes = 0;
  // Stream that writes the partials of everything but the deferred layers.  Set by a caller that sends the deferred layers to
  // another stream: a flush a reservation makes while layers are pending then goes here, whichever stream the call names.
  bool own_flush_stream = false; hipStream_t flush_stream = nullptr;
  size_t peak = 0;                             // highest end of a region handed out since the queue was built or rebound (floats)
  WgradFlushLog log{};
};

// ---- split geometry, shared by the kernels and their planners ---------------------------------------------------------------
// rows of one of `ksplit` row ranges of M rows, rounded up to whole workgroup steps of STEP rows.  STEP is a template argument
// and the device form is always_inline so that the kernels compile to exactly what they did with the formula written out in
// them (either one missing moved the register allocation of wgrad_kernel<bf16, conv>: 114 AGPRs instead of 116).
template <int STEP>
SRAD_WGRAD_HD static inline int srad_wgrad_rows_per(int M, int ksplit) { return ((M + ksplit - 1) / ksplit + STEP - 1) / STEP * STEP; }

// Row splits of a layer of `units` workgroups per split (tiles x taps) for about `wg_target` workgroups in all, at least two row
// steps per wave: the nearest power of two (rounding up from 1.43x) - so that from 8 up it is a multiple of 8, one XCD per row
// range, and the row ranges come out equal - less the splits that rounding the ranges up to whole steps leaves empty.
template <int STEP>
static inline int srad_wgrad_split_count(int M, long units, long wg_target) {
  long target = (wg_target + units - 1) / units;
  const long kmax = (M + 2 * STEP - 1) / (2 * STEP);
  if (target > kmax) target = kmax;
  int ksplit = 1;
  while (ksplit * 2 <= kmax && (long)ksplit * 10 <= target * 7) ksplit *= 2;
  const int rows_per = srad_wgrad_rows_per<STEP>(M, ksplit);
  return (M + rows_per - 1) / rows_per;
}

// ---- construction and rebinding -------------------------------------------------------------------------------------------
static inline WgradQueue wgrad_queue_on(float* ws, size_t floats) {
  WgradQueue q;
  q.ws = ws; q.ws_floats = floats;
  return q;
}
// flushes a reservation makes while layers are pending go to `stream` (see WgradQueue::flush_stream)
static inline void wgrad_queue_flush_on(WgradQueue& q, hipStream_t stream) { q.own_flush_stream = true; q.flush_stream = stream; }
static inline int wgrad_queue_pending_layers(const WgradQueue& q) { return q.multi.count; }
static inline bool wgrad_queue_empty(const WgradQueue& q) { return q.batch.count == 0 && q.multi.count == 0 && q.used == 0; }
// Moves the queue to another workspace (the engines' two halves for the two-stream blocks); `peak` restarts.  Only an empty
// queue can move: regions and partial pointers of anything queued, pending or reserved lie in the old workspace.
static inline int wgrad_queue_rebind(WgradQueue& q, float* ws, size_t floats) {
  if (!wgrad_queue_empty(q)) return SRAD_WGRAD_NOT_EMPTY;
  q.ws = ws; q.ws_floats = floats; q.peak = 0;
  return 0;
}

// ---- flush: reduce what is written, keep what is pending --------------------------------------------------------------------
// reduce(const WgradReduceBatch&, int tiles, int why) -> 0 or its error; called at most once, and not for an empty batch
template <class Reduce>
static int wgrad_queue_flush(WgradQueue& q, int why, Reduce&& reduce) {
  WgradReduceBatch now{};
  int now_tiles = 0;
  for (int i = 0; i < q.batch.count; ++i) {
    if (q.pending[i]) continue;
    WgradReduceItem& it = now.it[now.count++];
    it = q.batch.it[i];
    it.tile0 = now_tiles;
    now_tiles += q.ntiles[i];
  }
  if (now.count > 0) {
    const int rc = reduce(now, now_tiles, why);
    if (rc) return rc;
    WgradFlushLog& l = q.log;
    if (l.count < SRAD_WGRAD_LOG) l.why[l.count] = (unsigned char)why;
    ++l.count; ++l.by_why[why];
  }
  int keep = 0;
  size_t top = 0;
  for (int i = 0; i < q.batch.count; ++i) {
    if (!q.pending[i]) continue;
    q.batch.it[keep] = q.batch.it[i]; q.ntiles[keep] = q.ntiles[i]; q.region[keep] = q.region[i]; q.pending[keep] = true;
    const size_t end = q.region[keep].off + q.region[keep].floats;
    if (end > top) top = end;
    ++keep;
  }
  for (int i = keep; i < q.batch.count; ++i) q.pending[i] = false;
  q.batch.count = keep;
  q.used = top; q.hole_lo = 0; q.hole_end = top;      // nothing pending: top = 0, the workspace starts over
  return 0;
}

// a free region of `need` floats: a hole an earlier flush left under the pending layers, else the space above everything
static inline bool wgrad_queue_place(WgradQueue& q, size_t need, size_t* at) {
  if (q.hole_lo < q.hole_end) {
    size_t c = q.hole_lo;
    for (bool moved = true; moved;) {                     // past every pending region [b, e) that [c, c + need) would touch
      moved = false;
      for (int i = 0; i < q.batch.count; ++i) {
        if (!q.pending[i]) continue;
        const size_t b = q.region[i].off, e = b + q.region[i].floats;
        if (c < e && c + need > b) { c = e; moved = true; }
      }
    }
    if (c + need <= q.hole_end) { *at = c; q.hole_lo = c + need; return true; }
  }
  if (q.used + need > q.ws_floats) return false;
  *at = q.used; q.used += need;
  return true;
}

// The one place workspace is handed out: `need` floats (*r) and room for `nitems` more batch entries.  When the batch or the
// workspace is full the queue flushes itself first (wgrad_queue_flush: with layers pending only the written items) and refuses
// if the region still does not fit.  The caller pushes its `nitems` items afterwards.
template <class Reduce>
static int wgrad_queue_reserve(WgradQueue& q, size_t need, int nitems, Reduce&& reduce, WgradRegion* r) {
  if (!q.ws || need > q.ws_floats) return SRAD_WGRAD_TOO_SMALL;
  if (nitems < 0 || nitems > SRAD_WGRAD_BATCH - SRAD_WGRAD_MULTI) return SRAD_WGRAD_BAD_NITEMS;
  const bool batch_ok = q.batch.count + nitems <= SRAD_WGRAD_BATCH;
  size_t at = 0;
  if (!batch_ok || !wgrad_queue_place(q, need, &at)) {
    const int rc = wgrad_queue_flush(q, batch_ok ? SRAD_WGRAD_FLUSH_WS : SRAD_WGRAD_FLUSH_BATCH, reduce);
    if (rc) return rc;
    if (q.batch.count + nitems > SRAD_WGRAD_BATCH || !wgrad_queue_place(q, need, &at)) return SRAD_WGRAD_NO_ROOM;
  }
  r->off = at; r->floats = need;
  if (at + need > q.peak) q.peak = at + need;
  return 0;
}

// The one way to append: an item whose partials (item.part) lie in `r` (room was reserved with r) and that takes `ntiles` reduce tiles.
// pending: a deferred layer's item, not to be reduced before wgrad_queue_deferred_launched.
static inline void wgrad_queue_push(WgradQueue& q, const WgradReduceItem& item, int ntiles, const WgradRegion& r, bool pending = false) {
  const int i = q.batch.count++;
  q.batch.it[i] = item; q.batch.it[i].tile0 = 0;
  q.ntiles[i] = ntiles; q.region[i] = r; q.pending[i] = pending;
}

// the next slot of the deferred launch (the caller has made room: multi.count < SRAD_WGRAD_MULTI); the layer is pending from here
static inline int wgrad_queue_defer_slot(WgradQueue& q) { return q.multi.count++; }
// the deferred launch has gone out: nothing is pending any more, and the holes between the layers are not tracked
static inline void wgrad_queue_deferred_launched(WgradQueue& q) {
  for (int i = 0; i < q.batch.count; ++i) q.pending[i] = false;
  q.multi.count = 0; q.multi_flops = 0; q.multi_bytes = 0;
  q.hole_lo = q.hole_end;
}
