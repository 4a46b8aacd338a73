// C ABI implementation (include/nbg.h): the engine's lifecycle, schema, loader and statistics
// entry points, the result rows (nbg_rows_*) and profiling.  The GO driver is go.cpp, the stages
// over device rows stages.cpp, FIND PATH path.cpp.
#include <chrono>
#include <algorithm>
#include <atomic>
#include <cstring>
#include <iterator>
#include <unordered_map>

#include "engine.h"
#include "nbg_rows.h"

static_assert(NBG_MAX_YIELDS == nbg::MAX_YIELDS && NBG_MAX_OVER == nbg::MAX_TYPES_Q,
              "include/nbg.h device limits match the engine's");

// a fresh seed for each query's rand32 / rand64 stream
uint64_t nbg::query_rand_seed() {
  static std::atomic<uint64_t> ctr{(uint64_t)std::chrono::steady_clock::now().time_since_epoch().count() * 0x9e3779b97f4a7c15ull};
  return ctr.fetch_add(0x9e3779b97f4a7c15ull, std::memory_order_relaxed);
}

using namespace nbg;

namespace nbg {

static void free_edge_type(DevEdgeType& d) {
  for (void* p : {(void*)d.row_ptr, (void*)d.col, (void*)d.dst_vid, (void*)d.rank, (void*)d.valid, (void*)d.d_props})
    if (p) (void)hipFree(p);
  for (auto* p : d.props)
    if (p) (void)hipFree(p);
  for (auto* p : d.narrow)
    if (p) (void)hipFree(p);
  if (d.old) {
    free_edge_type(*d.old);
    delete d.old;
    d.old = nullptr;
  }
}

void Engine::free_snapshot() {
  for (auto& kv : snap.types) free_edge_type(kv.second);
  for (auto& kv : snap.tags) {
    if (kv.second.decoded && kv.second.decoded != kv.second.present) (void)hipFree(kv.second.decoded);
    if (kv.second.present) (void)hipFree(kv.second.present);
    for (auto* p : kv.second.cols)
      if (p) (void)hipFree(p);
  }
  for (void* p : {(void*)snap.d_tcols, (void*)snap.d_tpres, (void*)snap.d_vids, (void*)snap.d_visible, (void*)snap.d_zero_rows,
                  (void*)snap.d_soff, (void*)snap.d_sbytes, (void*)snap.d_s2i, (void*)snap.d_s2f, (void*)snap.d_s2ok})
    if (p) (void)hipFree(p);
  snap = Snapshot();
}

// The dictionary's device tables: its bytes (piece lists of derived strings read them) and what
// Expression::toInt / toDouble make of every string (Expressions.h:294-321; a string that is not
// a whole number fails the cast, as the host's constant folding and the oracle decide it).
int32_t Engine::upload_strings() {
  const auto& d = snap.strings;
  if (d.empty()) return NBG_OK;
  const size_t n = d.size();
  std::vector<uint32_t> off(n + 1, 0);
  for (size_t i = 0; i < n; ++i) {
    if ((uint64_t)off[i] + d[i].size() > 0xFFFFFFFFull) return fail(NBG_E_UNSUPPORTED, "string dictionary over 4 GB");
    off[i + 1] = off[i] + (uint32_t)d[i].size();
  }
  std::vector<char> bytes(std::max<size_t>(off[n], 1));
  std::vector<int64_t> s2i(n), s2f(n);
  std::vector<uint8_t> ok(n);
  for (size_t i = 0; i < n; ++i) {
    memcpy(bytes.data() + off[i], d[i].data(), d[i].size());
    CVal vi, vf;
    uint8_t b = 0;
    if (evalCast(0, CVal(d[i]), &vi)) { s2i[i] = std::get<int64_t>(vi); b |= 1; }
    if (evalCast(2, CVal(d[i]), &vf)) { const double x = std::get<double>(vf); memcpy(&s2f[i], &x, 8); b |= 2; }
    ok[i] = b;
  }
  hipError_t e = hipMalloc((void**)&snap.d_soff, (n + 1) * 4);
  if (e == hipSuccess) e = hipMalloc((void**)&snap.d_sbytes, bytes.size());
  if (e == hipSuccess) e = hipMalloc((void**)&snap.d_s2i, n * 8);
  if (e == hipSuccess) e = hipMalloc((void**)&snap.d_s2f, n * 8);
  if (e == hipSuccess) e = hipMalloc((void**)&snap.d_s2ok, n);
  if (e == hipSuccess) e = hipMemcpy(snap.d_soff, off.data(), (n + 1) * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(snap.d_sbytes, bytes.data(), bytes.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(snap.d_s2i, s2i.data(), n * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(snap.d_s2f, s2f.data(), n * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(snap.d_s2ok, ok.data(), n, hipMemcpyHostToDevice);
  if (e != hipSuccess) return fail(NBG_E_OUT_OF_MEMORY, std::string("string tables: ") + hipGetErrorString(e));
  snap.device_bytes += (n + 1) * 4 + bytes.size() + n * 17;
  return NBG_OK;
}

DevStrings Engine::dev_strings() const {
  DevStrings s;
  s.off = snap.d_soff;
  s.bytes = snap.d_sbytes;
  s.s2i = snap.d_s2i;
  s.s2f = snap.d_s2f;
  s.s2ok = snap.d_s2ok;
  s.n = snap.strings.size();
  return s;
}

uint64_t Engine::sp_item_cap() const {
  // a level claims each vertex once; its items are its 64-entry runs over the side's types
  uint64_t pos_types = 0, e_out = 0, e_in = 0;
  for (auto& kv : snap.types) {
    if (kv.first > 0) { ++pos_types; e_out += kv.second.num_edges; }
    else e_in += kv.second.num_edges;
  }
  return snap.nv * std::max<uint64_t>(pos_types, 1) + std::max(e_out, e_in) / 64 + 1024;
}

uint64_t Engine::sp_edge_cap() const {
  uint64_t e_out = 0, e_in = 0;
  for (auto& kv : snap.types) (kv.first > 0 ? e_out : e_in) += kv.second.num_edges;
  return std::max(e_out, e_in) + 1;
}

SpCtx* Engine::new_sp(hipStream_t s, std::string* err) {
  SpCtx* c = sp_create(snap.nv, sp_item_cap(), sp_edge_cap(), s, err);
  if (c && prof_mode) sp_profile(c, prof_mode);
  return c;
}

uint32_t Engine::dense(int64_t vid) const {
  auto& v = snap.h_vids;
  auto it = std::lower_bound(v.begin(), v.end(), vid);
  return (it != v.end() && *it == vid) ? (uint32_t)(it - v.begin()) : NO_ROW;
}

}  // namespace nbg


namespace nbg {

// Pinned host blocks for fetched rows, reused across queries (a fresh pinned allocation per fetch
// would cost more than the copy itself); at most kPinnedIdle blocks are kept idle.
constexpr size_t kPinnedIdle = 4;

void* Engine::pinned_get(size_t bytes, size_t* got) {
  std::lock_guard<std::mutex> lg(pinned_mu);
  size_t best = pinned_free.size();
  for (size_t i = 0; i < pinned_free.size(); ++i)
    if (pinned_free[i].first >= bytes && (best == pinned_free.size() || pinned_free[i].first < pinned_free[best].first))
      best = i;
  if (best < pinned_free.size()) {
    void* p = pinned_free[best].second;
    *got = pinned_free[best].first;
    pinned_free.erase(pinned_free.begin() + (ptrdiff_t)best);
    return p;
  }
  const size_t cap = std::max<size_t>(bytes + bytes / 8, 1 << 20);   // a little room to grow into
  void* p = nullptr;
  if (hipHostMalloc(&p, cap, hipHostMallocDefault) != hipSuccess) return nullptr;
  *got = cap;
  return p;
}

void Engine::pinned_put(void* p, size_t bytes) {
  if (!p) return;
  std::lock_guard<std::mutex> lg(pinned_mu);
  pinned_free.emplace_back(bytes, p);
  if (pinned_free.size() > kPinnedIdle) {   // drop the smallest idle block
    size_t small = 0;
    for (size_t i = 1; i < pinned_free.size(); ++i)
      if (pinned_free[i].first < pinned_free[small].first) small = i;
    (void)hipHostFree(pinned_free[small].second);
    pinned_free.erase(pinned_free.begin() + (ptrdiff_t)small);
  }
}

void Engine::pinned_release() {
  std::lock_guard<std::mutex> lg(pinned_mu);
  for (auto& b : pinned_free) (void)hipHostFree(b.second);
  pinned_free.clear();
}

}  // namespace nbg

namespace {

// Rows whose schema makes RowReader read columns at shifted positions: the reference's bytes are
// rebuilt per row (RowWriter with the result schema) and read back column by column as
// InterimResult::getRows does (InterimResult.cpp:74-153); a read past the row's end fails the
// query.  Runs on the fetched host copy (strings already dictionary-decoded).
int32_t reread_rows(nbg_rows* r) {
  Engine& E = *r->eng;
  const int nc = r->ncols;
  std::vector<uint8_t> b;
  uint64_t o = 0;
  for (auto& s : r->segs) {
    const uint64_t len = s.end - s.begin;
    const std::vector<uint8_t>& wc = r->wclass[s.type];
    for (uint64_t i = o; i < o + len; ++i) {
      b.clear();
      for (int c = 0; c < nc; ++c) {
        const int64_t v = r->col(c)[i];
        const int32_t t = r->col_types[c];
        if (wc[c] == W_ONE) { b.push_back(0); continue; }
        if (wc[c] == W_EIGHT) { b.insert(b.end(), 8, 0); continue; }
        switch (t) {
          case NBG_T_BOOL: b.push_back(v != 0); break;
          case NBG_T_VID: case NBG_T_DOUBLE:
            for (int k = 0; k < 8; ++k) b.push_back((uint8_t)((uint64_t)v >> (8 * k)));
            break;
          case NBG_T_STRING: {
            const std::string& str = r->strings[(size_t)v];
            for (uint64_t n = str.size();; n >>= 7) {
              b.push_back((uint8_t)((n & 0x7f) | (n > 0x7f ? 0x80 : 0)));
              if (n <= 0x7f) break;
            }
            b.insert(b.end(), str.begin(), str.end());
            break;
          }
          default:   // INT / TIMESTAMP: varint of the two's-complement bits
            for (uint64_t n = (uint64_t)v;; n >>= 7) {
              b.push_back((uint8_t)((n & 0x7f) | (n > 0x7f ? 0x80 : 0)));
              if (n <= 0x7f) break;
            }
        }
      }
      size_t p = 0;
      for (int c = 0; c < nc; ++c) {
        const int32_t t = r->col_types[c];
        int64_t out = 0;
        bool ok = true;
        auto varint = [&](uint64_t* x) {
          *x = 0;
          for (int sh = 0; sh < 64; sh += 7) {
            if (p >= b.size()) return false;
            const uint8_t y = b[p++];
            *x |= (uint64_t)(y & 0x7f) << sh;
            if (!(y & 0x80)) return true;
          }
          return false;
        };
        switch (t) {
          case NBG_T_BOOL:
            ok = p < b.size();
            if (ok) out = b[p++] != 0;
            break;
          case NBG_T_VID: case NBG_T_DOUBLE:
            ok = p + 8 <= b.size();
            if (ok) {
              uint64_t x = 0;
              for (int k = 0; k < 8; ++k) x |= (uint64_t)b[p + k] << (8 * k);
              p += 8;
              out = (int64_t)x;
            }
            break;
          case NBG_T_STRING: {
            uint64_t n = 0;
            ok = varint(&n) && n <= b.size() - p;
            if (ok) {
              out = (int64_t)r->strings.size();
              r->strings.emplace_back(reinterpret_cast<const char*>(b.data() + p), (size_t)n);
              p += n;
            }
            break;
          }
          default: {
            uint64_t x = 0;
            ok = varint(&x);
            out = (int64_t)x;
          }
        }
        if (!ok) return E.fail(NBG_E_EXECUTION_ERROR, "Get value from interim failed (column " + std::to_string(c) + ")");
        r->col(c)[i] = out;
      }
    }
    o += len;
  }
  return NBG_OK;
}

// per-cell kinds of column c (nbg_rows_col_tags), built on first use
const uint8_t* cell_tags(nbg_rows* r, int c) {
  if (r->tags.empty()) r->tags.resize(r->ncols);
  std::vector<uint8_t>& t = r->tags[c];
  if (t.size() != r->count) {
    t.resize(r->count);
    uint64_t o = 0;
    for (auto& s : r->segs) {
      const uint64_t len = s.end - s.begin;
      std::fill(t.begin() + (ptrdiff_t)o, t.begin() + (ptrdiff_t)(o + len), (uint8_t)r->kinds[s.type][c]);
      o += len;
    }
  }
  return t.data();
}

}  // namespace

// The rows of a result into host memory: the device packs the segments into contiguous columns
// and DMAs them into a pinned block (nbg.h nbg_rows_fetch).  Only STRING columns are touched per
// cell on the host (dictionary code -> the result's string table).
int32_t nbg::materialize_rows(nbg_rows* r) {
  if (r->fetched) return NBG_OK;
  r->build_segs();
  Engine& E = *r->eng;
  // InterimResult::getRows has no case for a FLOAT column: "Unknown Type: 4" (InterimResult.cpp:142-146)
  if (r->float_col && r->count) return E.fail(NBG_E_EXECUTION_ERROR, "Unknown Type: 4");
  const auto& dict = E.snap.strings;
  const size_t bytes = std::max<size_t>((size_t)r->count * (size_t)r->ncols * 8, 8);
  r->hbits = static_cast<int64_t*>(E.pinned_get(bytes, &r->hbytes));
  if (!r->hbits) return NBG_E_OUT_OF_MEMORY;
  // packed at the query's end already (a small result, go_launch): the segments' cells in this order
  const int64_t* pre = r->count && r->ws && r->small_ok ? ws_host_small_rows(r->ws, r->count) : nullptr;
  if (pre) {
    memcpy(r->hbits, pre, (size_t)r->count * (size_t)r->ncols * 8);
  } else if (r->count) {
    std::vector<std::pair<uint64_t, uint64_t>> segs;
    segs.reserve(r->segs.size());
    for (auto& s : r->segs) segs.emplace_back(s.begin, s.end - s.begin);
    const hipError_t he = ws_fetch_rows_pinned(r->ws ? r->ws : E.ws, segs, r->ncols, r->count, r->hbits);
    if (he != hipSuccess)   // (named: round 4's one "row fetch failed" left no trace of the failing call)
      return E.fail(NBG_E_DEVICE, std::string("row fetch failed: ") + hipGetErrorName(he) + " (" +
                                      hipGetErrorString(he) + "), " + std::to_string(segs.size()) + " segments, " +
                                      std::to_string(r->count) + " rows");
  }
  bool any_string = false;
  for (auto& kv : r->kinds)
    for (VKind k : kv) any_string = any_string || k == VK_STRING;
  if (any_string) {
    std::unordered_map<int64_t, int64_t> sidx;
    uint64_t o = 0;
    for (auto& s : r->segs) {
      const uint64_t len = s.end - s.begin;
      for (int c = 0; c < r->ncols; ++c) {
        if (r->kinds[s.type][c] != VK_STRING) continue;   // payloads are final as copied
        int64_t* col = r->col(c);
        for (uint64_t i = o; i < o + len; ++i) {
          const int64_t code = col[i];
          auto it = sidx.find(code);
          if (it == sidx.end()) {
            std::string txt;
            if (is_derived_code(code)) {
              auto d = r->derived.find(code);
              if (d == r->derived.end()) return E.fail(NBG_E_DEVICE, "a derived string's text is missing");
              txt = d->second;
            } else {
              txt = (code >= 0 && (code & 1) == 0 && (uint64_t)(code / 2) < dict.size()) ? dict[code / 2]
                                                                                          : r->const_str[s.type][c];
            }
            it = sidx.emplace(code, (int64_t)r->strings.size()).first;
            r->strings.push_back(txt);
          }
          col[i] = it->second;
        }
      }
      o += len;
    }
  }
  if (r->misaligned && r->count) {
    const int32_t rc = reread_rows(r);
    if (rc) return rc;
  }
  r->fetched = true;
  return NBG_OK;
}

Workspace* nbg::ws_fresh(Engine& E, uint64_t max_frontier, uint64_t e_max, hipStream_t stream, Comm* comm,
                        Workspace* old, std::string* err) {
  Workspace* fresh = ws_create(max_frontier, E.snap.nv, e_max, stream, err);
  if (fresh && E.partitioned() && ws_set_partition(fresh, comm, E.npad) != hipSuccess) {
    ws_destroy(fresh);
    fresh = nullptr;
    *err = "partition buffers";
  }
  if (fresh && E.row_reserve && ws_reserve_rows(fresh, E.row_reserve, E.col_reserve) != hipSuccess) {
    ws_destroy(fresh);
    fresh = nullptr;
    *err = "result rows";
  }
  if (fresh && old) ws_profile_inherit(fresh, old);
  return fresh;
}

int32_t nbg::ws_release(Engine& E, Workspace** wsp, hipStream_t stream) {
  auto it = E.holders.find(*wsp);
  if (it == E.holders.end()) return NBG_OK;
  // the fresh workspace first: on failure nothing changes (the rows keep their workspace, which
  // stays busy until they are freed)
  Comm* cm = ws_get_comm(*wsp);   // (the fresh workspace keeps the slot's communicator)
  std::string err;
  Workspace* fresh =
      ws_fresh(E, E.snap.nv + 1024, E.snap.max_edges(), stream, cm ? cm : E.comm.get(), *wsp, &err);
  if (!fresh)
    return E.fail(NBG_E_OUT_OF_MEMORY, "a held device result occupies the query workspace and a new one could not be "
                                       "allocated (" + err + "); free device results first");
  nbg_rows* r = it->second;
  E.holders.erase(it);
  r->owned_ws = *wsp;
  *wsp = fresh;
  return NBG_OK;
}

// The query workspace of a finalized (or snapshot-loaded) engine.
int32_t nbg::engine_ready(Engine& E) {
  if (int32_t rc = E.upload_strings()) return rc;
  if (E.partitioned() && !E.snap.d_zero_rows) {   // (path.cpp: OVER types this rank has no edges of)
    const size_t zb = ((size_t)E.snap.nv + 1) * 4;
    if (hipMalloc((void**)&E.snap.d_zero_rows, zb) != hipSuccess || hipMemset(E.snap.d_zero_rows, 0, zb) != hipSuccess)
      return E.fail(NBG_E_OUT_OF_MEMORY, "empty CSR rows");
  }
  static const bool tiny_on = !getenv("NBG_TINY") || atoi(getenv("NBG_TINY")) != 0;
  if (!E.partitioned() && tiny_on) {   // walk bounds of the tiny GO path (a failure only disables it)
    for (auto& kv : E.snap.types)
      if (kv.first > 0)
        (void)tiny_bounds(kv.second.row_ptr, kv.second.col, E.snap.d_visible, E.edge_cap(), E.snap.nv,
                          &kv.second.h_w2, &kv.second.h_w3, E.stream);
  }
  std::string err;
  E.ws = ws_create(E.snap.nv + 1024, E.snap.nv, E.snap.max_edges(), E.stream, &err);
  if (!E.ws) return E.fail(NBG_E_OUT_OF_MEMORY, err);
  if (E.partitioned()) {
    hipError_t he = ws_set_partition(E.ws, E.comm.get(), E.npad);
    const size_t G = (size_t)E.cfg.num_gpus, seg = E.npad / 8, gw = part_gst_words((int)G);
    if (he == hipSuccess) he = hipMalloc(&E.fb_send, G * seg);
    if (he == hipSuccess) he = hipMemset(E.fb_send, 0, G * seg);
    if (he == hipSuccess) he = hipMalloc(&E.fb_recv, G * seg);
    if (he == hipSuccess) he = hipMalloc((void**)&E.fb_gst, gw * 8);
    if (he == hipSuccess) he = hipHostMalloc((void**)&E.fb_hgst, gw * 8, hipHostMallocDefault);
    if (he != hipSuccess) return E.fail(NBG_E_OUT_OF_MEMORY, std::string("partition buffers: ") + hipGetErrorString(he));
    return build_path_replica(E);   // collective: every rank finalizes together
  }
  return NBG_OK;
}

// ============================================================================= C ABI
extern "C" {

int32_t nbg_create(const nbg_config* cfg, nbg_engine** out) {
  if (!cfg || !out) return NBG_E_INVALID_ARGUMENT;
  if (cfg->num_parts <= 0 || cfg->num_gpus <= 0 || cfg->rank < 0 || cfg->rank >= cfg->num_gpus)
    return NBG_E_INVALID_ARGUMENT;
  auto* h = new nbg_engine();
  h->e.cfg = *cfg;
  if (h->e.cfg.max_edge_returned_per_vertex <= 0) h->e.cfg.max_edge_returned_per_vertex = 0x7fffffff;
  *out = h;
  return NBG_OK;
}

void nbg_destroy(nbg_engine* h) {
  if (!h) return;
  Engine& E = h->e;
  go_drain(E);         // tickets never waited for
  E.holders.clear();  // results must be freed before nbg_destroy (nbg.h)
  for (auto& q : E.slots) {
    if (q.stream) (void)hipStreamSynchronize(q.stream);
    if (q.ws) ws_destroy(q.ws);
    q.comm.reset();
    if (q.stream) (void)hipStreamDestroy(q.stream);
  }
  path_slots_release(E);
  destroy_path_replica(E);
  if (E.stream) (void)hipStreamSynchronize(E.stream);
  for (void* p : {E.fb_send, E.fb_recv, (void*)E.fb_gst})
    if (p) (void)hipFree(p);
  if (E.fb_hgst) (void)hipHostFree(E.fb_hgst);
  E.pinned_release();
  if (E.ws) ws_destroy(E.ws);
  if (E.sp) sp_destroy(E.sp);
  E.free_snapshot();
  if (E.stream) (void)hipStreamDestroy(E.stream);
  delete h;
}

int32_t nbg_inject_fault(nbg_engine* h, int32_t site, int32_t count) {
  if (!h || site < 0 || count < 0) return NBG_E_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lg(h->e.mu);
  h->e.fault_site = count ? site : 0;
  h->e.fault_count = count;
  return NBG_OK;
}

int32_t nbg_staged_edges(const nbg_engine* h, int32_t type, int64_t* src, int64_t* dst, int64_t* rank, uint64_t cap,
                         uint64_t* n) {
  if (!h || !n || type == 0) return NBG_E_INVALID_ARGUMENT;
  const Engine& E = h->e;
  std::lock_guard<std::mutex> lg(const_cast<Engine&>(E).mu);
  if (E.finalized) return NBG_E_STATE;
  *n = 0;
  auto it = E.stage.find(type);
  if (it == E.stage.end()) return NBG_OK;
  const EdgeStage& st = it->second;
  *n = st.size();
  const uint64_t m = std::min<uint64_t>(cap, st.size());
  for (uint64_t i = 0; i < m; ++i) {
    if (src) src[i] = st.src[i];
    if (dst) dst[i] = st.dst[i];
    if (rank) rank[i] = st.rank.empty() ? 0 : st.rank[i];
  }
  return NBG_OK;
}

const char* nbg_last_error(const nbg_engine* h) { return h ? h->e.last_error.c_str() : "null engine"; }

static int32_t reg_schema(std::map<int32_t, SchemaSet>& m, int32_t id, const char* name, int64_t ver,
                          const nbg_column_def* cols, int32_t ncols) {
  if (!name || ncols < 0 || (ncols && !cols)) return NBG_E_INVALID_ARGUMENT;
  SchemaSet& ss = m[id];
  ss.name = name;
  Schema s;
  s.version = ver;
  for (int32_t i = 0; i < ncols; ++i) {
    if (!cols[i].name) return NBG_E_INVALID_ARGUMENT;
    s.cols.push_back(Column{cols[i].name, cols[i].type});
  }
  ss.versions[ver] = s;
  return NBG_OK;
}

int32_t nbg_register_tag(nbg_engine* h, int32_t tag_id, const char* name, int64_t ver, const nbg_column_def* cols,
                         int32_t ncols) {
  if (!h) return NBG_E_INVALID_ARGUMENT;
  if (h->e.finalized) return h->e.fail(NBG_E_STATE, "engine already finalized");
  return reg_schema(h->e.tags, tag_id, name, ver, cols, ncols);
}

int32_t nbg_register_edge(nbg_engine* h, int32_t edge_type, const char* name, int64_t ver,
                          const nbg_column_def* cols, int32_t ncols) {
  if (!h) return NBG_E_INVALID_ARGUMENT;
  if (h->e.finalized) return h->e.fail(NBG_E_STATE, "engine already finalized");
  if (edge_type <= 0) return h->e.fail(NBG_E_INVALID_ARGUMENT, "edge types are positive");
  return reg_schema(h->e.edges, edge_type, name, ver, cols, ncols);
}

int32_t nbg_load_part_kv(nbg_engine* h, int32_t part, const uint8_t* kd, const uint64_t* ko, const uint8_t* vd,
                         const uint64_t* vo, uint64_t n) {
  if (!h || (n && (!kd || !ko || !vd || !vo))) return NBG_E_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lg(h->e.mu);
  return h->e.load_part_kv(part, kd, ko, vd, vo, n);
}

int32_t nbg_load_edges(nbg_engine* h, int32_t edge_type, const int64_t* src, const int64_t* dst, const int64_t* rank,
                       uint64_t n, const void* const* prop_cols, int32_t ncols) {
  if (!h || (n && (!src || !dst)) || (ncols && !prop_cols)) return NBG_E_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lg(h->e.mu);
  return h->e.load_edges(edge_type, src, dst, rank, n, prop_cols, ncols);
}

int32_t nbg_finalize(nbg_engine* h) {
  if (!h) return NBG_E_INVALID_ARGUMENT;
  Engine& E = h->e;
  std::lock_guard<std::mutex> lg(E.mu);
  if (hipSetDevice(E.cfg.device) != hipSuccess) return E.fail(NBG_E_DEVICE, "hipSetDevice failed");
  if (!E.stream && hipStreamCreateWithFlags(&E.stream, hipStreamNonBlocking) != hipSuccess)
    return E.fail(NBG_E_DEVICE, "hipStreamCreate failed");
  int32_t rc = E.finalize();
  if (rc) return rc;
  return engine_ready(E);
}

int32_t nbg_get_stats(const nbg_engine* h, nbg_stats* out) {
  if (!h || !out) return NBG_E_INVALID_ARGUMENT;
  const Engine& E = h->e;
  memset(out, 0, sizeof(*out));
  out->num_vertices = E.snap.nv;
  for (auto& kv : E.snap.types) out->num_edges += kv.second.num_edges;
  out->device_bytes = E.snap.device_bytes;
  out->num_edge_types = (int32_t)E.snap.types.size();
  out->tiny_queries = E.tiny_queries;
  out->host_agreements = E.host_agreements;
  out->path_batch_contexts = E.batch_sp.size();
  out->path_batch_reruns = E.batch_reruns;
  uint64_t hb = 0;
  for (const std::string& x : E.snap.strings) hb += x.size() + sizeof(std::string);
  for (auto& kv : E.snap.types)
    hb += (kv.second.h_row_ptr.size() + kv.second.h_w2.size() / 2 + kv.second.h_w3.size() / 2) * 4;
  hb += E.snap.h_visible.size();
  out->host_bytes = hb;
  return NBG_OK;
}

int64_t nbg_rows_count(const nbg_rows* r) { return r ? (int64_t)r->count : -1; }
int32_t nbg_rows_num_cols(const nbg_rows* r) { return r ? r->ncols : -1; }
uint64_t nbg_rows_edges_scanned(const nbg_rows* r) { return r ? r->scanned : 0; }

int32_t nbg_rows_step_stats(const nbg_rows* r, uint64_t* frontier, uint64_t* edges, int32_t cap) {
  if (!r) return NBG_E_INVALID_ARGUMENT;
  int32_t k = 0;
  for (; k < cap && k < (int32_t)r->step_frontier.size(); ++k) {
    if (frontier) frontier[k] = r->step_frontier[k];
    if (edges) edges[k] = k < (int32_t)r->step_edges.size() ? r->step_edges[k] : 0;
  }
  return k;
}

int32_t nbg_rows_fetch(nbg_rows* r) {
  if (!r) return NBG_E_INVALID_ARGUMENT;
  if (r->fetched) return NBG_OK;
  std::lock_guard<std::mutex> lg(r->eng->mu);   // the fetch runs on the result's workspace stream
  if (hipSetDevice(r->eng->cfg.device) != hipSuccess) return NBG_E_DEVICE;
  return materialize_rows(r);
}

const int64_t* nbg_rows_col_bits(const nbg_rows* r, int32_t col) {
  if (!r || !r->fetched || col < 0 || col >= r->ncols) return nullptr;
  return r->col(col);
}
const uint8_t* nbg_rows_col_tags(const nbg_rows* r, int32_t col) {
  if (!r || !r->fetched || col < 0 || col >= r->ncols) return nullptr;
  return cell_tags(const_cast<nbg_rows*>(r), col);
}
int32_t nbg_rows_col_kind(const nbg_rows* r, int32_t col) {
  if (!r || col < 0 || col >= r->ncols) return -1;
  return r->col_kind(col);
}
const char* nbg_rows_string(const nbg_rows* r, int64_t id) {
  if (!r || id < 0 || id >= (int64_t)r->strings.size()) return nullptr;
  return r->strings[id].c_str();
}
int64_t nbg_rows_num_segments(const nbg_rows* r) {
  if (!r) return -1;
  const_cast<nbg_rows*>(r)->build_segs();
  return (int64_t)r->segs.size();
}
int32_t nbg_rows_segment(const nbg_rows* r, int64_t i, uint64_t* begin, uint64_t* end) {
  if (r) const_cast<nbg_rows*>(r)->build_segs();
  if (!r || i < 0 || i >= (int64_t)r->segs.size() || !begin || !end) return NBG_E_INVALID_ARGUMENT;
  *begin = r->segs[i].begin;
  *end = r->segs[i].end;
  return NBG_OK;
}
const void* nbg_rows_device_col(const nbg_rows* r, int32_t col) {
  if (!r || col < 0 || col >= (int32_t)r->dcols.size()) return nullptr;
  return r->dcols[col];
}
int32_t nbg_rows_digest(const nbg_rows* r, uint64_t* out) {
  if (!r || !out) return NBG_E_INVALID_ARGUMENT;
  out[0] = out[1] = out[2] = 0;
  if (!r->count) return NBG_OK;
  if (r->fetched && !r->on_device) {   // host rows: the same chain on the host
    for (uint64_t i = 0; i < r->count; ++i) {
      uint64_t h = 0;
      for (int c = 0; c < r->ncols; ++c) {
        uint64_t z = (h ^ (uint64_t)r->col(c)[i]) + 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        h = z ^ (z >> 31);
      }
      ++out[0];
      out[1] ^= h;
      out[2] += h;
    }
    return NBG_OK;
  }
  Engine& E = *r->eng;
  std::lock_guard<std::mutex> lg(E.mu);
  if (hipSetDevice(E.cfg.device) != hipSuccess) return E.fail(NBG_E_DEVICE, "hipSetDevice failed");
  auto* m = const_cast<nbg_rows*>(r);
  m->build_segs();
  std::vector<std::pair<uint64_t, uint64_t>> segs;
  for (auto& sg : m->segs) segs.emplace_back(sg.begin, sg.end - sg.begin);
  const hipError_t he = ws_rows_digest(r->owned_ws ? r->owned_ws : r->ws, segs, r->ncols, out);
  return he == hipSuccess ? NBG_OK : E.fail(NBG_E_DEVICE, std::string("digest: ") + hipGetErrorString(he));
}

void nbg_rows_free(nbg_rows* r) {
  if (!r) return;
  if (r->eng && r->hbits) r->eng->pinned_put(r->hbits, r->hbytes);
  if (r->eng && (r->owned_ws || r->ws)) {
    Engine& E = *r->eng;
    std::lock_guard<std::mutex> lg(E.mu);
    auto it = E.holders.find(r->ws);
    if (it != E.holders.end() && it->second == r) E.holders.erase(it);
    if (r->owned_ws) {
      (void)hipSetDevice(E.cfg.device);
      ws_destroy(r->owned_ws);
    }
  }
  delete r;
}

int32_t nbg_set_path_replica(nbg_engine* h, int32_t mode) {
  if (!h || mode < 0 || mode > 1) return NBG_E_INVALID_ARGUMENT;
  Engine& E = h->e;
  std::lock_guard<std::mutex> lg(E.mu);
  if (!E.finalized) {   // before finalize: whether to build it
    E.path_replica_mode = mode;
    return NBG_OK;
  }
  if (mode && !E.rep) return E.fail(NBG_E_STATE, "this engine has no FIND PATH replica");
  E.path_replica_use = mode != 0;   // after: whether FIND PATH uses it
  return NBG_OK;
}

int32_t nbg_path_replica_active(const nbg_engine* h) { return h && h->e.rep && h->e.path_replica_use ? 1 : 0; }

int32_t nbg_profile(nbg_engine* h, int32_t enable) {
  if (!h) return NBG_E_INVALID_ARGUMENT;
  Engine& E = h->e;
  std::lock_guard<std::mutex> lg(E.mu);
  if (!E.ws) return E.fail(NBG_E_STATE, "engine not finalized");
  const int mode = enable == 2 ? 2 : (enable != 0 ? 1 : 0);
  ws_profile(E.ws, mode);
  for_stage_profs(E, [&](const char* const*, auto& p) {   // (enabling resets the counters, as ws_profile does)
    if (mode) p = {};
    p.on = mode == 1;
  });
  // the one-pair SHORTEST contexts (device-driven chains): their launches and algorithmic bytes
  for (Engine* P : {&E, E.rep.get()}) {   // (and the FIND PATH replica's)
    if (!P) continue;
    P->prof_mode = mode;
    sp_profile(P->sp, mode);
    for (auto& ps : P->path_slots) sp_profile(ps.sp, mode);
    for (SpCtx* c : P->batch_sp) sp_profile(c, mode);
  }
  return NBG_OK;
}

int32_t nbg_profile_read(const nbg_engine* h, nbg_kernel_stat* out, int32_t cap) {
  if (!h || !out || !h->e.ws) return 0;
  const Engine& E = h->e;
  int n = ws_profile_read(E.ws, out, cap);
  double launches[CHAIN_KINDS] = {}, ms[CHAIN_KINDS] = {}, bytes[CHAIN_KINDS] = {};
  for (const Engine* P : {&E, (const Engine*)E.rep.get()}) {
    if (!P) continue;
    sp_profile_accum(P->sp, launches, ms, bytes);
    for (auto& ps : P->path_slots) sp_profile_accum(ps.sp, launches, ms, bytes);
    for (SpCtx* c : P->batch_sp) sp_profile_accum(c, launches, ms, bytes);
  }
  for (int k = 0; k < CHAIN_KINDS && n < cap; ++k, ++n) {
    out[n].name = kChainKernelNames[k];
    out[n].launches = (uint64_t)launches[k];
    out[n].total_ms = ms[k];
    out[n].algo_bytes = bytes[k];
  }
  for_stage_profs(E, [&](const char* const* names, const auto& p) {
    for (int k = 0; k < (int)std::size(p.ms) && n < cap; ++k, ++n) {
      out[n].name = names[k];
      out[n].launches = p.launches[k];
      out[n].total_ms = p.ms[k];
      out[n].algo_bytes = p.bytes[k];
    }
  });
  return n;
}

int32_t nbg_find_path(nbg_engine* h, const nbg_path_request* req, nbg_paths** out);

int64_t nbg_paths_count(const nbg_paths* p) { return p ? (int64_t)p->paths.size() : -1; }
int64_t nbg_path_len(const nbg_paths* p, int64_t i) {
  return (p && i >= 0 && i < (int64_t)p->paths.size()) ? (int64_t)p->paths[i].size() : -1;
}
const int64_t* nbg_path_entries(const nbg_paths* p, int64_t i) {
  return (p && i >= 0 && i < (int64_t)p->paths.size()) ? p->paths[i].data() : nullptr;
}
uint64_t nbg_paths_edges_scanned(const nbg_paths* p) { return p ? p->edges : 0; }
uint32_t nbg_paths_chain_batches(const nbg_paths* p) { return p ? p->batches : 0; }
void nbg_paths_free(nbg_paths* p) { delete p; }

}  // extern "C"
