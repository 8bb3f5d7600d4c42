// drct_derived.h - the weights of the DRCT forward that are composed from several parameters.  Host-only: no HIP
// include (tests/host/drct_derived_check.cpp).  Such a weight is no entry of the parameter table: it has a region of the weight
// arena behind the table's packs, holding the fp32 sources in PyTorch layout and what is built from them (tail_fold.h, mlp_fold.h).
// The registry owns where the regions lie, which parameter is a source of which region, and which regions are stale.
#pragma once
#include "tail_fold.h"
#include "mlp_fold.h"
#include <string>
#include <unordered_map>
#include <vector>

enum DrctDerivedKind { DRCT_TAIL_FOLD = 0, DRCT_BLOCK_FOLD = 1, DRCT_DERIVED_KINDS = 2 };   // the folded output end; fc2 in a block's adjust conv
enum { DRCT_DERIVED_CAPTURING = -1 };                  // refresh(): something to build, and the stream captures
// kind, which of its kind (the block i * 5 + k), offset (a multiple of 256) and size in the arena, dirty: a source changed or the
// arena was bound since the last build
struct DrctDerivedRegion { int kind, index; size_t off, bytes; bool dirty; };
struct DrctDerivedSource { int region; size_t off; };  // off: of the source's fp32 copy inside the region

struct DrctDerived {
  std::vector<DrctDerivedRegion> regions;                        // in arena order
  std::unordered_map<std::string, DrctDerivedSource> sources;    // by parameter name
  size_t end = 0;                                                // arena bytes needed; starts as the parameter table's
  int first[DRCT_DERIVED_KINDS] = {-1, -1};                      // a kind's regions are added one after the other, index 0 first

  int add(int kind, int index, size_t bytes) {                   // a new region (dirty) at the next 256-byte boundary; returns its id
    const size_t off = (end + 255) / 256 * 256;
    regions.push_back({kind, index, off, bytes, true});
    end = off + bytes;
    if (first[kind] < 0) first[kind] = (int)regions.size() - 1;
    return (int)regions.size() - 1;
  }
  void add_source(const std::string& name, int region, size_t off) { sources[name] = {region, off}; }
  const DrctDerivedSource* find(const char* name) const { const auto it = sources.find(name); return it == sources.end() ? nullptr : &it->second; }
  bool has(int kind) const { return first[kind] >= 0; }
  const DrctDerivedRegion& region(int kind, int index) const { return regions[first[kind] + index]; }
  void mark(int region) { regions[region].dirty = true; }
  void mark_all() { for (DrctDerivedRegion& r : regions) r.dirty = true; }
  // build(region) -> 0 or an error code, for every dirty region of an active kind (bit 1 << kind of `kinds`) in arena order; one of
  // another kind stays dirty, and so does one whose build fails.  While the stream captures nothing may be built: with something
  // to build, DRCT_DERIVED_CAPTURING and nothing is cleared.  stale(kinds): is there something to build?
  template <class Build>
  int refresh(unsigned kinds, bool capturing, Build&& build) {
    for (DrctDerivedRegion& r : regions) {
      if (!r.dirty || !(kinds >> r.kind & 1)) continue;
      if (capturing) return DRCT_DERIVED_CAPTURING;
      if (const int err = build(static_cast<const DrctDerivedRegion&>(r))) return err;
      r.dirty = false;
    }
    return 0;
  }
  bool stale(unsigned kinds) const { for (const DrctDerivedRegion& r : regions) if (r.dirty && (kinds >> r.kind & 1)) return true; return false; }
};

// The model's two kinds, with their sources at the layouts' offsets (upsample.2 exists at scale 4 only; block k = 0 .. 4 of RDG rdg)
inline void drct_derived_add_tail(DrctDerived& r, const TailFoldLayout& l) {
  const int id = r.add(DRCT_TAIL_FOLD, 0, l.bytes);
  r.add_source("upsample.0.weight", id, l.w_up0); r.add_source("upsample.0.bias", id, l.b_up0);
  if (l.scale == 4) { r.add_source("upsample.2.weight", id, l.w_up1); r.add_source("upsample.2.bias", id, l.b_up1); }
  r.add_source("conv_last.weight", id, l.w_last); r.add_source("conv_last.bias", id, l.b_last);
}
inline void drct_derived_add_block(DrctDerived& r, int rdg, int k, const MlpFoldLayout& l) {
  const int id = r.add(DRCT_BLOCK_FOLD, rdg * 5 + k, l.bytes);
  const std::string li = "layers." + std::to_string(rdg), sk = std::to_string(k + 1);
  r.add_source(li + ".swin" + sk + ".mlp.fc2.weight", id, l.w2); r.add_source(li + ".swin" + sk + ".mlp.fc2.bias", id, l.b2);
  r.add_source(li + ".adjust" + sk + ".weight", id, l.a); r.add_source(li + ".adjust" + sk + ".bias", id, l.ba);
}
