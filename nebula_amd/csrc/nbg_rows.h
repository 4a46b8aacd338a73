// The result object behind nbg_rows_* (engine.cpp), the GO driver that builds it (go.cpp) and the
// stages over device rows (stages.cpp).
#pragma once
#include <string>
#include <unordered_map>
#include <vector>

#include "engine.h"

namespace nbg {
uint64_t query_rand_seed();   // a fresh seed for each query's rand32 / rand64 stream
// RowWriter's written form of one value (RowWriter.cpp:103-186, RowWriter.inl:9-33): the value
// itself (ID), or the default it falls back to for an incompatible column type — varint 0 / a
// false byte (ONE zero byte) or a 0.0 double (EIGHT zero bytes).
enum WClass : uint8_t { W_ID = 0, W_ONE = 1, W_EIGHT = 2 };
}

// The result of nbg_rows_encode (stages.cpp): the RowSetWriter bytes in pinned memory from the
// engine's pool, and the schema's field types.
struct nbg_rowset {
  nbg::Engine* eng = nullptr;
  uint8_t* data = nullptr;
  size_t cap = 0;                // the pinned block's size (returned to the pool with it)
  uint64_t len = 0;
  uint64_t rows = 0;
  std::vector<int32_t> types;    // NBG_T_* per column
};

struct nbg_rows {
  struct Seg {
    uint64_t begin = 0, end = 0;
    int type = 0;                          // index into kinds / const_str (OVER position)
  };
  std::vector<std::vector<nbg::VKind>> kinds;              // per OVER type: value kind of each column
  std::vector<std::vector<std::string>> const_str;    // per OVER type: string constants absent from the dictionary
  nbg::Engine* eng = nullptr;
  nbg::Workspace* ws = nullptr;               // the workspace holding the rows (device results)
  nbg::Workspace* owned_ws = nullptr;         // set when the engine handed that workspace over (ws_release)
  int ncols = 0;
  uint64_t count = 0;
  bool on_device = false;
  bool fetched = false;
  std::vector<int64_t*> dcols;           // column bases; rows live in segs (disjoint regions)
  // host copy (nbg_rows_fetch): column c at hbits + c * count, in pinned memory from the engine's
  // pool (DMA straight from the packed device copy, no staging and no zero-fill)
  int64_t* hbits = nullptr;
  size_t hbytes = 0;
  std::vector<std::vector<uint8_t>> tags;   // per-cell kinds, built on the first nbg_rows_col_tags
  std::vector<std::string> strings;
  std::unordered_map<int64_t, std::string> derived;   // STR_DERIVED codes -> their text
  std::vector<Seg> segs;                 // built on first use from the per-workgroup counts
  struct TypeBlocks {
    uint64_t region = 0, blk_cap = 0;
    std::vector<uint32_t> counts;        // rows per workgroup of the final expansion
  };
  std::vector<TypeBlocks> blocks;
  bool segs_built = false;
  void build_segs() {
    if (segs_built) return;
    segs_built = true;
    size_t n = 0;
    for (auto& tb : blocks)
      for (uint32_t c : tb.counts) n += c != 0;
    segs.reserve(n);
    for (size_t i = 0; i < blocks.size(); ++i) {
      const TypeBlocks& tb = blocks[i];
      for (size_t b = 0; b < tb.counts.size(); ++b) {
        if (!tb.counts[b]) continue;
        Seg seg;
        seg.begin = tb.region + (uint64_t)b * tb.blk_cap;
        seg.end = seg.begin + tb.counts[b];
        seg.type = (int)i;
        segs.push_back(seg);
      }
    }
  }
  int64_t* col(int c) const { return hbits + (uint64_t)c * count; }
  // the kind of column c when every OVER type gives it the same one (else -1: per-cell tags)
  int col_kind(int c) const {
    int k = -1;
    for (auto& kv : kinds) {
      if ((int)kv.size() <= c) continue;
      if (k < 0) k = kv[c];
      else if (k != kv[c]) return -1;
    }
    return k < 0 ? nbg::VK_INT : k;
  }
  uint64_t scanned = 0;
  std::vector<uint64_t> step_frontier, step_edges;
  // the result schema (GoExecutor::setupInterimResult): NBG_T_* per column, what RowWriter wrote
  // per (OVER type, column), and the read-back hazards it implies (see go_prepare)
  std::vector<int32_t> col_types;
  std::vector<std::vector<uint8_t>> wclass;
  bool small_ok = false;     // the end-of-query kernel may have packed these rows (ws_host_small_rows)
  bool misaligned = false;   // some column's written bytes differ in length from what its reader takes
  bool float_col = false;    // a FLOAT column: InterimResult::getRows fails on it
};
