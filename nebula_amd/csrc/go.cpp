// The GO N STEPS driver: prepared statements, the synchronous and the asynchronous entry points, and
// GO FROM $-.col over a device-resident result (nbg_go_piped; its kernels are in gopipe.hip).
//
// GO N STEPS follows GoExecutor (src/graph/GoExecutor.cpp):
//   * starts keep duplicates (prepareFrom :136-195); unknown vids contribute nothing;
//   * steps 1..N-1: frontier_{s+1} = SET of _dst over every live edge of every OVER type
//     (getDstIdsFromResp :501-541) — no global visited set; empty frontier -> empty result
//     (onEmptyInputs :791-800);
//   * step N: one row per (frontier entry, live edge) passing WHERE; WHERE/YIELD evaluation
//     errors fail the query (processFinalResult :948-969).
// Each hop runs on the device: degree scan -> merge-path partition -> expand (+ byte-flag
// dedup and compaction, or the final-step bytecode + row compaction).
#include <algorithm>
#include <array>
#include <atomic>
#include <cstring>
#include <ctime>
#include <iterator>
#include <set>
#include <unordered_map>

#include "engine.h"
#include "nbg_rows.h"

using namespace nbg;

// ============================================================================= prepared statements
// A prepared GO statement: GoExecutor::prepare() (OVER / WHERE / YIELD validated, compiled once
// per OVER type, GoExecutor.cpp:136-263); execute() runs it from a start list.
struct nbg_go_stmt {
  Engine* eng = nullptr;
  uint64_t id = 0;                   // device program cache key
  std::vector<int32_t> over;
  std::vector<TypeProgram> plist;    // OVER order (default program where compilation deferred)
  int ncols = 0;
  uint32_t steps = 1;
  int32_t deferred = NBG_OK;         // name-resolution error, reported only if the final step runs
  std::string deferred_msg;
  std::string dst_unknown;           // a $$ tag name is unknown: fails once the final step has edges
  bool distinct = false;             // YIELD DISTINCT: distinct starts and rows
  std::vector<int32_t> col_types;    // the result schema (NBG_T_* per column)
  std::vector<std::vector<uint8_t>> wclass;   // per OVER position: WClass of each column
  bool misaligned = false, float_col = false;
  bool derived = false;              // some YIELD stores derived strings (OP_SOUT: the string arena)
  uint64_t sout_row_bytes = 0;       // arena bytes one final edge may store (the largest type's bound)
  // $- / $var input: index rows (the FROM vid, ascending; last row per vid) and their columns,
  // uploaded on first execution (the same index on every rank of a partitioned engine)
  bool uses_input = false;
  std::vector<int64_t> in_ids;
  std::vector<std::vector<int64_t>> in_cols;
  uint64_t in_n = 0;                 // index rows (in_ids.size(), or what gopipe_index built on the device)
  int64_t* d_in_ids = nullptr;
  int64_t** d_in_cols = nullptr;
  std::vector<int64_t*> d_in_col_ptrs;
  // input strings absent from the snapshot's dictionary (codes STR_INPUT | index), their bytes
  // uploaded with the index
  std::vector<std::string> in_xstr;
  uint32_t* d_xoff = nullptr;
  char* d_xbytes = nullptr;
  // the filtered adjacency over the first OVER type (stmtidx.hip; nbg.h, nbg_go_prepare): built once
  // the statement's completed executions have scanned idx_after x the type's edges in final steps
  bool idx_on = false;               // made by nbg_go_prepare and not switched off
  double idx_after = 0.25;           // NBG_STMT_INDEX_AFTER
  uint64_t idx_budget = UINT64_MAX;  // NBG_STMT_INDEX_MB, in bytes
  uint64_t final_scanned = 0;        // final-step edges of the completed executions
  StmtIndex idx;
  bool idx_tried = false;
  void free_input_index() {
    for (void* p : {(void*)d_in_ids, (void*)d_in_cols, (void*)d_xoff, (void*)d_xbytes})
      if (p) (void)hipFree(p);
    for (auto* p : d_in_col_ptrs)
      if (p) (void)hipFree(p);
    d_in_ids = nullptr;
    d_in_cols = nullptr;
    d_xoff = nullptr;
    d_xbytes = nullptr;
    d_in_col_ptrs.clear();
  }
  ~nbg_go_stmt() {
    stmtidx_free(&idx);
    free_input_index();
  }
};

static bool has_input_prop(const Node* n) {
  if (!n) return false;
  if (n->kind == EK_INPUT || n->kind == EK_VAR) return true;
  for (auto& k : n->kids)
    if (has_input_prop(k.get())) return true;
  return false;
}

// Props a query names on each edge alias (Expression::prepare's alias set, Expressions.cpp:314-400)
using AliasProps = std::map<std::string, std::set<std::string>>;
static void alias_props(const Node* n, AliasProps& out) {
  if (!n) return;
  switch (n->kind) {
    case EK_ALIAS: case EK_DST: case EK_SRCID: case EK_RANK: case EK_TYPE:
      out[n->alias].insert(n->prop);
      break;
    default: break;
  }
  for (auto& k : n->kids) alias_props(k.get(), out);
}

// OVER * without YIELD: GoExecutor::finishExecution names one `<edge>._dst` column per entry of
// the first response's edge_schema, in that map's iteration order (GoExecutor.cpp:481-499,
// 546-561).  The order is libstdc++'s: storaged fills edgeContexts_ (an unordered_map, from the
// request's edge types, QueryBaseProcessor.inl:46-57, QueryBaseProcessor.h:114), copies it into
// the response's edge_schema (an unordered_map, QueryBoundProcessor.cpp:139-158), and graphd
// decodes that into another unordered_map (storage.thrift:104).  The same three containers, keyed
// the same way, reproduce it.
// the iteration order of storaged's edgeContexts_ for a request's edge types: the order
// processVertex emits a vertex's edge data in (QueryBaseProcessor.inl:46-57, QueryBoundProcessor.cpp:120-167)
static std::vector<int32_t> edge_context_order(const std::vector<int32_t>& req) {
  std::unordered_map<int32_t, int> contexts;
  std::transform(req.begin(), req.end(), std::inserter(contexts, contexts.end()),
                 [](int32_t t) { return std::make_pair(t, 0); });
  std::vector<int32_t> order;
  for (const auto& kv : contexts) order.push_back(kv.first);
  return order;
}

static std::vector<int32_t> response_schema_order(const std::vector<int32_t>& req) {
  std::unordered_map<int32_t, int> schema;
  for (int32_t t : edge_context_order(req))
    if (schema.find(t) == schema.end()) schema.emplace(t, 0);
  std::unordered_map<int32_t, int> decoded;
  for (const auto& kv : schema) decoded.emplace(kv.first, 0);
  std::vector<int32_t> order;
  for (const auto& kv : decoded) order.push_back(kv.first);
  return order;
}

namespace {   // (to the end of the synchronous driver, go_impl)

// ----------------------------------------------------------------------------- go_prepare's phases
// What go_prepare decodes from the request and needs only until the programs are compiled.
struct GoClauses {
  std::unique_ptr<Node> where;
  std::vector<std::unique_ptr<Node>> yields;
  AliasProps named;                     // props named per edge alias, over WHERE and every YIELD
  std::vector<std::string> in_names;    // the input table's columns
  std::vector<VKind> in_kinds;
  std::map<int32_t, TypeProgram> progs;   // per OVER type (none where compilation was deferred)
};

// OVER (prepareOver / prepareOverAll, GoExecutor.cpp:197-263)
static int32_t prepare_over(Engine& E, const nbg_go_request* rq, std::vector<int32_t>* over) {
  if (rq->over_all) {
    for (auto& kv : E.edges) over->push_back(kv.first);
  } else {
    for (int32_t i = 0; i < rq->num_edge_types; ++i) {
      int32_t t = rq->edge_types[i];
      if (t <= 0) return E.fail(NBG_E_EXECUTION_ERROR, "`REVERSELY' not supported yet");
      if (!E.edges.count(t)) return E.fail(NBG_E_EXECUTION_ERROR, "edge type not found");
      over->push_back(t);
    }
  }
  if (over->empty()) return E.fail(NBG_E_EXECUTION_ERROR, "empty OVER clause");
  return NBG_OK;
}

// WHERE / YIELD
static int32_t prepare_clauses(Engine& E, const nbg_go_request* rq, const std::vector<int32_t>& over, GoClauses* cl) {
  std::string err;
  if (rq->where && rq->where_len) {
    cl->where = decode_expr(rq->where, rq->where_len, &err);
    if (!cl->where) return E.fail(NBG_E_INVALID_ARGUMENT, "WHERE: " + err);
  }
  for (int32_t i = 0; i < rq->num_yields; ++i) {
    auto y = decode_expr(rq->yields[i], rq->yield_lens[i], &err);
    if (!y) return E.fail(NBG_E_INVALID_ARGUMENT, "YIELD: " + err);
    cl->yields.push_back(std::move(y));
  }
  if (cl->yields.empty()) {   // default YIELD <edge>._dst per OVER edge (parser.yy:518-531)
    for (int32_t t : rq->over_all ? response_schema_order(over) : over) {
      auto n = std::make_unique<Node>();
      n->kind = EK_DST;
      n->alias = E.edges[t].name;
      n->prop = "_dst";
      cl->yields.push_back(std::move(n));
    }
  }
  if ((int)cl->yields.size() > MAX_YIELDS) return E.fail(NBG_E_UNSUPPORTED, "too many YIELD columns");
  return NBG_OK;
}

// $- / $var input: the index GoExecutor::setupStarts builds on the FROM column.  `piped` (nbg_go_piped):
// the input is a device-resident result; its columns' kinds are its own and the index is built on the
// device once the statement is prepared (gopipe_index), so only the names and kinds are taken here.
static int32_t prepare_input(Engine& E, const nbg_go_request* rq, nbg_go_stmt* st, GoClauses* cl, const nbg_rows* piped) {
  if (!st->uses_input) return NBG_OK;
  if (rq->num_input_cols <= 0) return E.fail(NBG_E_EXECUTION_ERROR, "$- / $var props need the piped or variable input");
  if (rq->num_input_cols > MAX_INPUT_COLS)
    return E.fail(NBG_E_UNSUPPORTED, "more than " + std::to_string(MAX_INPUT_COLS) + " input columns");
  if (piped) {
    for (int32_t c = 0; c < rq->num_input_cols; ++c) {
      const int k = piped->col_kind(c);
      cl->in_names.emplace_back(rq->input_names[c] ? rq->input_names[c] : "");
      cl->in_kinds.push_back(k < 0 ? VK_INT : (VKind)k);
    }
    return NBG_OK;
  }
  if (!rq->input_names || !rq->input_kinds || !rq->input_cols ||
      rq->input_vid_col < 0 || rq->input_vid_col >= rq->num_input_cols)
    return E.fail(NBG_E_INVALID_ARGUMENT, "input table");
  const uint64_t n = rq->num_input_rows;
  for (int32_t c = 0; c < rq->num_input_cols; ++c) {
    cl->in_names.emplace_back(rq->input_names[c] ? rq->input_names[c] : "");
    cl->in_kinds.push_back((VKind)rq->input_kinds[c]);
  }
  const int64_t* vidc = static_cast<const int64_t*>(rq->input_cols[rq->input_vid_col]);
  std::vector<std::pair<int64_t, uint64_t>> rowof;   // (vid, last row)
  {
    std::unordered_map<int64_t, uint64_t> last;
    for (uint64_t r = 0; r < n; ++r) last[vidc[r]] = r;   // vidToRowIndex_[v] = row: the last wins
    for (auto& kv : last) rowof.emplace_back(kv.first, kv.second);
    std::sort(rowof.begin(), rowof.end());
  }
  st->in_cols.assign(rq->num_input_cols, std::vector<int64_t>(rowof.size()));
  for (auto& pr : rowof) st->in_ids.push_back(pr.first);
  st->in_n = st->in_ids.size();
  // strings the dictionary lacks (a string derived by an earlier statement of the pipe): a table of
  // their own, so they keep their bytes (a dictionary code between neighbours would not)
  std::vector<std::string>& in_xstr = st->in_xstr;   // (sorted, unique)
  auto text = [&](int32_t c, uint64_t r) {
    const char* str = static_cast<const char* const*>(rq->input_cols[c])[r];
    return std::string(str ? str : "");
  };
  for (int32_t c = 0; c < rq->num_input_cols; ++c)
    if (cl->in_kinds[c] == VK_STRING)
      for (auto& pr : rowof)
        if (string_code(E.snap.strings, text(c, pr.second)) & 1) in_xstr.push_back(text(c, pr.second));
  std::sort(in_xstr.begin(), in_xstr.end());
  in_xstr.erase(std::unique(in_xstr.begin(), in_xstr.end()), in_xstr.end());
  for (int32_t c = 0; c < rq->num_input_cols; ++c) {
    for (size_t k = 0; k < rowof.size(); ++k) {
      const uint64_t r = rowof[k].second;
      if (cl->in_kinds[c] == VK_STRING) {
        int64_t code = string_code(E.snap.strings, text(c, r));
        if (code & 1)
          code = STR_INPUT | (int64_t)(std::lower_bound(in_xstr.begin(), in_xstr.end(), text(c, r)) - in_xstr.begin());
        st->in_cols[c][k] = code;
      } else {
        st->in_cols[c][k] = static_cast<const int64_t*>(rq->input_cols[c])[r];
      }
    }
  }
  return NBG_OK;
}

// Compile WHERE and the YIELDs for OVER type t; name-resolution errors are reported only if the
// final step runs (the statement's deferred code; the type then keeps the default program)
static int32_t compile_type(Engine& E, nbg_go_stmt* st, int32_t t, GoClauses* cl) {
  std::string err;
  auto it = E.snap.types.find(t);
  CompileEnv env{t, &st->over, &E.edges, &E.snap.strings,
                 it != E.snap.types.end() && it->second.valid != nullptr,
                 it != E.snap.types.end() && it->second.rank != nullptr};
  env.max_dict_len = E.max_dict_len;
  // the response edge row schema of type t: _dst, then the props named on t (getStepOutProps,
  // GoExecutor.cpp:587-630)
  std::map<std::string, VKind> row_cols{{"_dst", VK_INT}};
  const SchemaSet& es = E.edges[t];
  for (auto& p : cl->named[es.name]) {
    if (p == "_src" || p == "_dst" || p == "_type" || p == "_rank") { row_cols.emplace(p, VK_INT); continue; }
    const Schema* sc = es.latest();
    const int c = sc ? sc->find(p) : -1;
    if (c >= 0) row_cols.emplace(p, kindOfType(sc->cols[c].type));
  }
  uint32_t probe = 0;
  env.tags = &E.tags;
  env.dtags = &E.snap.tags;
  env.row_cols = &row_cols;
  env.partitioned = E.partitioned();
  env.dst_unknown = &st->dst_unknown;
  env.probe_mask = &probe;
  if (st->uses_input) {
    env.input_names = &cl->in_names;
    env.input_kinds = &cl->in_kinds;
    env.input_derived = !st->in_xstr.empty();
    for (const std::string& x : st->in_xstr) env.max_dict_len = std::max<uint64_t>(env.max_dict_len, x.size());
  }
  ProgramBuilder pb;
  TypeProgram tp;
  tp.etype = t;
  int32_t rc = NBG_OK;
  if (cl->where) {
    Compiled c;
    rc = compile_expr(*cl->where, env, pb, &c, &err);
    if (rc == NBG_OK) {
      tp.where_len = (int)pb.code.size();
      if (c.is_const) {
        bool tv;
        switch (c.kind) {
          case VK_STRING: tv = c.const_str.empty(); break;
          case VK_DOUBLE: { double d; memcpy(&d, &c.const_bits, 8); tv = d != 0.0; break; }
          default: tv = c.const_bits != 0;
        }
        tp.where_const = true;
        tp.where_const_val = tv;
        tp.where_len = 0;
        pb.code.clear();
      } else {
        // asBool of the WHERE value (GoExecutor.cpp:954)
        int r = c.reg;
        if (c.kind == VK_INT) pb.code.push_back(Ins{OP_TRUTHY_I, (uint8_t)r, (uint8_t)r, 0, 0, 0});
        else if (c.kind == VK_DOUBLE) pb.code.push_back(Ins{OP_TRUTHY_F, (uint8_t)r, (uint8_t)r, 0, 0, 0});
        else if (c.kind == VK_STRING)
          pb.code.push_back(Ins{OP_TRUTHY_S, (uint8_t)r, (uint8_t)r, 0, 0, string_code(E.snap.strings, "")});
        tp.where_len = (int)pb.code.size();
        tp.where_reg = r;
        tp.where_always_error = c.always_error;
      }
      pb.next_reg = 0;   // WHERE registers are dead once its value is read
    }
  }
  for (int y = 0; rc == NBG_OK && y < st->ncols; ++y) {
    Compiled c;
    rc = compile_expr(*cl->yields[y], env, pb, &c, &err, true);
    if (rc) break;
    tp.yield_kind.push_back(c.kind);
    tp.yield_reg.push_back(c.is_const ? -1 : c.reg);
    tp.yield_const.push_back(c.is_const ? c.const_bits : 0);
    tp.yield_const_str.push_back(c.is_const ? c.const_str : std::string());
  }
  if (rc == NBG_E_UNSUPPORTED || rc == NBG_E_INVALID_ARGUMENT) return E.fail(rc, err);
  if (rc) {
    if (!st->deferred) { st->deferred = rc; st->deferred_msg = err; }
    return NBG_OK;
  }
  tp.code = pb.code;
  tp.data = pb.data;
  for (const Ins& i : tp.code) tp.sout = tp.sout || i.op == OP_SOUT || i.op == OP_SMAT;   // (the arena)
  tp.sout_bytes = pb.sout_bytes;
  tp.probe_mask = probe;
  tp.nregs = std::max(1, pb.max_reg);
  if ((int)(tp.code.size() + tp.data.size()) > MAX_PROGRAM) return E.fail(NBG_E_UNSUPPORTED, "program too long");
  if (tp.nregs > interp_max_regs())
    return E.fail(NBG_E_UNSUPPORTED, "expression too deep for the device register file (" + std::to_string(tp.nregs) +
                                         " registers, " + std::to_string(interp_max_regs()) + " fit the LDS)");
  cl->progs[t] = std::move(tp);
  return NBG_OK;
}

WClass written_class(VKind k, int32_t t) {
  switch (k) {
    case VK_INT: return (t == NBG_T_INT || t == NBG_T_TIMESTAMP || t == NBG_T_VID) ? W_ID : W_ONE;
    case VK_DOUBLE: return (t == NBG_T_DOUBLE || t == NBG_T_FLOAT) ? W_ID : W_EIGHT;
    case VK_BOOL: return t == NBG_T_BOOL ? W_ID : W_ONE;
    default: return t == NBG_T_STRING ? W_ID : W_ONE;
  }
}
// does the reader of a `t` column take exactly the bytes written? (else the row's later columns
// are read at shifted positions)
bool read_aligned(WClass w, int32_t t) {
  if (w == W_ID) return true;
  if (w == W_ONE) return t == NBG_T_INT || t == NBG_T_TIMESTAMP || t == NBG_T_BOOL || t == NBG_T_STRING;
  return t == NBG_T_VID;
}
VKind read_kind(int32_t t) {   // the value InterimResult::getRows reads from a `t` column
  switch (t) {
    case NBG_T_BOOL: return VK_BOOL;
    case NBG_T_FLOAT: case NBG_T_DOUBLE: return VK_DOUBLE;
    case NBG_T_STRING: return VK_STRING;
    default: return VK_INT;
  }
}

// ---- the result schema and what RowWriter makes of each value (GoExecutor::setupInterimResult,
// GoExecutor.cpp:707-788).  The reference types every column from the FIRST row it evaluates
// (yield_column_type) and writes every row through that schema: a value of another kind becomes
// the writer's default (RowWriter.cpp:103-186), and a default of another length shifts the
// columns after it when InterimResult::getRows reads the row back.  Which row is first follows
// hash-map order; the canonical row here is an edge of the first type in the request's
// edge-context order (QueryBaseProcessor.inl:46-57, the order processVertex emits edge data in)
// whose source has the $^ tags the columns read.  Aligned defaults become constants of the
// compiled programs (the expression still runs, so its errors still fail the query); shifted
// rows are re-read on the host copy (reread_rows); a FLOAT column fails the fetch.
static void prepare_schema(Engine& E, nbg_go_stmt* st, GoClauses* cl) {
  const std::vector<int32_t>& over = st->over;
  const int ncols = st->ncols;
  std::map<int32_t, TypeProgram>& progs = cl->progs;
  std::vector<int32_t>& ctype = st->col_types;
  ctype.assign(ncols, NBG_T_INT);
  st->wclass.assign(over.size(), std::vector<uint8_t>(ncols, W_ID));
  const int32_t t0 = edge_context_order(over)[0];
  std::map<std::string, int32_t> row_types{{"_dst", NBG_T_VID}};
  for (auto& p : cl->named[E.edges[t0].name]) {
    if (p == "_src" || p == "_dst") { row_types[p] = NBG_T_VID; continue; }
    if (p == "_rank" || p == "_type") { row_types[p] = NBG_T_INT; continue; }
    const Schema* sc = E.edges[t0].latest();
    const int c = sc ? sc->find(p) : -1;
    if (c >= 0) row_types[p] = sc->cols[c].type;
  }
  ColTypeEnv cenv;
  cenv.row_type = t0;
  cenv.edges = &E.edges;
  cenv.tags = &E.tags;
  cenv.row_types = &row_types;
  if (st->uses_input) {
    cenv.input_names = &cl->in_names;
    cenv.input_kinds = &cl->in_kinds;
  }
  auto p0 = progs.find(t0);
  if (p0 == progs.end()) p0 = progs.begin();
  for (int y = 0; y < ncols; ++y) {
    ctype[y] = yield_column_type(*cl->yields[y], cenv);
    if (!ctype[y] && p0 != progs.end()) {
      const VKind k = p0->second.yield_kind[y];
      ctype[y] = k == VK_DOUBLE ? NBG_T_DOUBLE : k == VK_BOOL ? NBG_T_BOOL : k == VK_STRING ? NBG_T_STRING : NBG_T_INT;
    }
    if (!ctype[y]) ctype[y] = NBG_T_INT;
    st->float_col = st->float_col || ctype[y] == NBG_T_FLOAT;
  }
  for (size_t i = 0; i < over.size(); ++i) {
    auto it = progs.find(over[i]);
    if (it == progs.end()) continue;
    TypeProgram& tp = it->second;
    for (int y = 0; y < ncols; ++y) {
      const WClass w = written_class(tp.yield_kind[y], ctype[y]);
      st->wclass[i][y] = w;
      if (w == W_ID) continue;
      st->misaligned = st->misaligned || !read_aligned(w, ctype[y]);
      const VKind rk = read_kind(ctype[y]);
      tp.yield_reg[y] = -1;
      tp.yield_kind[y] = rk;
      tp.yield_const[y] = rk == VK_STRING ? string_code(E.snap.strings, "") : 0;
      tp.yield_const_str[y] = std::string();
    }
  }
}

// Derived strings (concatenation, casts to string): a YIELD column's string has ONE code
// whatever produced it — the dictionary's, else STR_DERIVED | its content hash — so constant
// strings absent from the dictionary take the hash code too (YIELD DISTINCT compares codes).
static void prepare_derived(nbg_go_stmt* st, GoClauses* cl) {
  for (auto& kv : cl->progs) {
    st->derived = st->derived || kv.second.sout;
    st->sout_row_bytes = std::max(st->sout_row_bytes, kv.second.sout_bytes);
  }
  if (!st->derived) return;
  for (auto& kv : cl->progs)
    for (int y = 0; y < st->ncols; ++y) {
      TypeProgram& tp = kv.second;
      if (tp.yield_reg[y] >= 0 || tp.yield_kind[y] != VK_STRING || !(tp.yield_const[y] & 1)) continue;
      uint64_t h = STR_HASH_INIT;
      for (char ch : tp.yield_const_str[y]) h = str_hash_step(h, (uint8_t)ch);
      tp.yield_const[y] = str_derived_code(h, tp.yield_const_str[y].size());
    }
}

static int32_t go_prepare(Engine& E, const nbg_go_request* rq, nbg_go_stmt** out, const nbg_rows* piped = nullptr) {
  if (!rq || !out) return E.fail(NBG_E_INVALID_ARGUMENT, "null argument");
  *out = nullptr;
  if (!E.finalized) return E.fail(NBG_E_STATE, "engine not finalized");
  if (rq->steps < 1) return E.fail(NBG_E_INVALID_ARGUMENT, "steps must be >= 1");
  auto st = std::make_unique<nbg_go_stmt>();
  st->eng = &E;
  st->steps = rq->steps;
  st->distinct = rq->distinct != 0;
  GoClauses cl;
  if (int32_t rc = prepare_over(E, rq, &st->over)) return rc;
  if (int32_t rc = prepare_clauses(E, rq, st->over, &cl)) return rc;
  st->ncols = (int)cl.yields.size();
  st->uses_input = has_input_prop(cl.where.get());
  for (auto& y : cl.yields) st->uses_input = st->uses_input || has_input_prop(y.get());
  if (int32_t rc = prepare_input(E, rq, st.get(), &cl, piped)) return rc;
  // compile per OVER type
  alias_props(cl.where.get(), cl.named);
  for (auto& y : cl.yields) alias_props(y.get(), cl.named);
  E.refresh_max_dict_len();
  for (int32_t t : st->over)
    if (int32_t rc = compile_type(E, st.get(), t, &cl)) return rc;
  if ((int)st->over.size() > MAX_TYPES_Q || rq->steps > (uint32_t)MAX_STEPS)
    return E.fail(NBG_E_UNSUPPORTED, "too many OVER types or steps");
  prepare_schema(E, st.get(), &cl);
  prepare_derived(st.get(), &cl);
  static std::atomic<uint64_t> next_id{1};
  st->id = next_id++;
  st->plist.resize(st->over.size());
  for (size_t i = 0; i < st->over.size(); ++i) {
    auto it = cl.progs.find(st->over[i]);
    if (it != cl.progs.end()) st->plist[i] = std::move(it->second);
  }
  *out = st.release();
  return NBG_OK;
}

// ============================================================================= one query
// A GO query enqueued on a workspace, completed by go_collect.
struct GoPending {
  std::unique_ptr<nbg_rows> rows;
  Workspace* ws = nullptr;
  bool device = false;
  bool finished = false;                 // nothing was enqueued (no start has rows)
  // partitioned, in band: this rank's preparation failed but it took part in the query's
  // collectives; nbg_go_submit keeps the ticket in its slot (so every rank's slot sequence stays
  // the same) and nbg_go_wait reports the code
  int32_t failed_rc = NBG_OK;
  std::string failed_msg;
  std::vector<uint64_t> region, blk_cap;
};

// The start list of one query: f0, the starts as dense ids (duplicates kept; sorted and unique
// under DISTINCT), and per OVER position its edge space — capped degrees, one pass over f0 per type.
// Two sums, on purpose:
//   * `all` counts every start: the device lists and the row regions are sized before the kernels
//     look at visibility (start_edges, and the final step's edge bound when steps == 1);
//   * `visible` skips invisible starts, as the kernels do: the inline list's entries and the
//     one-step bound of the tiny path.
struct GoStarts {
  struct PerType {
    uint64_t all = 0, visible = 0;
    InlineList il{};   // filled when the list is short (inline_list())
  };
  std::vector<uint32_t> f0;     // (empty when the list is built on the device: `pipe`)
  uint64_t n = 0;               // the list's entries
  GoPipe* pipe = nullptr;       // nbg_go_piped: gopipe_list writes the list into the workspace
  std::vector<PerType> types;   // OVER order
  uint64_t start_edges = 0;     // the largest `all`

  GoStarts(const Engine& E, const nbg_go_stmt& st, const int64_t* starts, uint64_t num_starts, uint32_t cap) {
    // starts -> dense ids (duplicates kept)
    f0.reserve(num_starts);
    for (uint64_t i = 0; i < num_starts; ++i) {
      uint32_t d = E.dense(starts[i]);
      if (d != NO_ROW) f0.push_back(d);
    }
    from_dense(E, st, cap);
  }
  // a short piped list, read back as dense ids in fetch order (nbg_go_piped)
  GoStarts(const Engine& E, const nbg_go_stmt& st, std::vector<uint32_t> dense, uint32_t cap) : f0(std::move(dense)) {
    from_dense(E, st, cap);
  }
  // a piped list that stays on the device: `count` entries (already unique under DISTINCT) whose
  // capped degrees over OVER position i sum to all[i] (GpCounts::deg of the types that have a CSR)
  GoStarts(const nbg_go_stmt& st, GoPipe* p, uint64_t count, const std::vector<uint64_t>& all) : n(count), pipe(p) {
    types.resize(st.over.size());
    for (size_t i = 0; i < st.over.size(); ++i) {
      types[i].all = all[i];
      types[i].il.n_in = (uint32_t)n;
      start_edges = std::max(start_edges, all[i]);
    }
  }
  // a short start list travels to the first expansion in its kernel arguments, with its edge
  // space over each OVER type computed here from the host CSR offsets (no k_relist launch)
  bool inline_list() const { return !pipe && n <= (uint64_t)INLINE_STARTS; }
  const InlineList* inline_of(size_t i, uint32_t step) const { return step == 1 && inline_list() ? &types[i].il : nullptr; }

 private:
  void from_dense(const Engine& E, const nbg_go_stmt& st, uint32_t cap) {
    if (st.distinct) {   // DISTINCT de-duplicates the starts too (GoExecutor.cpp:101-107)
      std::sort(f0.begin(), f0.end());
      f0.erase(std::unique(f0.begin(), f0.end()), f0.end());
    }
    n = f0.size();
    types.resize(st.over.size());
    const std::vector<uint8_t>& vis = E.snap.h_visible;
    for (size_t i = 0; i < st.over.size(); ++i) {
      PerType& pt = types[i];
      pt.il.n_in = (uint32_t)f0.size();
      auto it = E.snap.types.find(st.over[i]);
      if (it == E.snap.types.end()) continue;
      const std::vector<uint32_t>& rp = it->second.h_row_ptr;
      const bool inl = inline_list();
      InlineList& il = pt.il;
      for (uint32_t d : f0) {
        const uint32_t deg = std::min<uint32_t>(rp[d + 1] - rp[d], cap);
        pt.all += deg;
        if (!deg || (!vis.empty() && !vis[d])) continue;
        pt.visible += deg;
        if (!inl) continue;
        il.total += deg;
        il.id[il.n] = d;
        il.end[il.n] = il.total;
        il.rs[il.n] = rp[d];
        ++il.n;
      }
      start_edges = std::max(start_edges, pt.all);
    }
  }
};

// What the phases of one go_launch share.
struct GoQuery {
  Engine& E;
  nbg_go_stmt* st;
  hipStream_t stream;
  Comm* qcomm;
  const bool part;
  const uint32_t cap;   // max_edge_returned_per_vertex
  Workspace* ws = nullptr;
  int64_t *bt = nullptr, *bt_in = nullptr;   // VertexBackTracker roots ($- / $var props after >= 2 steps)
  // now() is the query's wall-clock second (WallClock::fastNowInSec); rand32 / rand64 draw from a
  // stream of the query's own
  int64_t now = 0;
  uint64_t seed = 0;
  // ---- rank-local preparation: the first failure is kept and agreed (go_agree)
  int32_t lrc = NBG_OK;
  std::string lmsg;
  void local_fail(int32_t code, const std::string& msg) {
    if (!lrc) { lrc = code; lmsg = msg; }
  }

  ExpandArgs args_for(const DevEdgeType& dt) const {
    ExpandArgs a{};
    a.now_sec = now;
    a.rand_seed = seed;
    a.row_ptr = dt.row_ptr;
    a.col = dt.col;
    a.dst_vid = dt.dst_vid;
    a.rank = dt.rank;
    a.valid = dt.valid;
    a.visible = E.snap.d_visible;
    a.vids = E.snap.d_vids;
    a.props = dt.d_props;
    a.hprops = dt.props.data();
    a.hnarrow = dt.narrow.empty() ? nullptr : dt.narrow.data();
    a.hnarrow_bytes = dt.narrow_bytes.empty() ? nullptr : dt.narrow_bytes.data();
    a.cap = cap;
    a.tcols = E.snap.d_tcols;
    a.tpres = E.snap.d_tpres;
    a.gbase = E.partitioned() ? (uint32_t)((uint64_t)E.cfg.rank * E.npad) : 0u;
    a.bt = bt;
    a.bt_in = bt_in;
    a.str = E.dev_strings();
    if (st->uses_input) {
      a.in_ids = st->d_in_ids;
      a.in_n = st->in_n;
      a.in_cols = st->d_in_cols;
      a.str.xoff = st->d_xoff;
      a.str.xbytes = st->d_xbytes;
      a.str.xn = st->in_xstr.size();
    }
    return a;
  }
  // the final step (and the list the step before it hands over) runs over the statement's
  // filtered rows where it has them; queries already launched keep the arguments they have
  const StmtIndex* index_of(size_t i) const {
    return st->steps >= 2 && !part && i == 0 && st->idx.rp ? &st->idx : nullptr;
  }
};

// Build the statement's filtered adjacency when it is due (under the engine mutex, before the
// launch, on the engine's stream).  It is tried once: a skipped or failed build leaves the
// statement on the WHERE path for good.  The first OVER type only: the final list of a later one
// is a k_relist of the frontier, which drops the vertices whose edges all fail, and E_N counts them.
static void stmt_index_build(const GoQuery& q) {
  Engine& E = q.E;
  nbg_go_stmt* st = q.st;
  if (!st->idx_on || st->idx_tried || st->steps < 2 || E.partitioned() || st->deferred || st->over.empty()) return;
  auto it = E.snap.types.find(st->over[0]);
  if (it == E.snap.types.end()) return;
  const DevEdgeType& dt = it->second;
  if ((double)st->final_scanned < st->idx_after * (double)dt.num_edges) return;
  st->idx_tried = true;
  // a binding max_edge_returned_per_vertex clips the scanned degree before the WHERE runs: a cap
  // over filtered degrees would change the results
  if ((uint64_t)q.cap < (uint64_t)std::max(dt.max_degree, 0)) return;
  const TypeProgram& prog = st->plist[0];
  if (prog.where_const) return;   // (folded: nothing to filter, or a scan-only final step)
  StmtIndexSpec sp{};
  if (!ws_final_where(prog, q.args_for(dt), &sp)) return;
  sp.nv = E.snap.nv;
  sp.edges = dt.num_edges;
  double ms = 0;
  const bool ok = stmtidx_build(sp, st->idx_budget, E.stream, &st->idx, &ms);
  if (getenv("NBG_STMT_INDEX_TRACE")) {
    if (ok)
      fprintf(stderr, "[stmt index] statement %llu type %d: built in %.3f ms after %llu final-step edges, %llu of %llu "
                      "edges pass, %.1f MB\n", (unsigned long long)st->id, st->over[0], ms,
              (unsigned long long)st->final_scanned, (unsigned long long)st->idx.rows,
              (unsigned long long)dt.num_edges, (double)st->idx.bytes / 1e6);
    else
      fprintf(stderr, "[stmt index] statement %llu type %d: not built (memory budget or allocation), %.3f ms\n",
              (unsigned long long)st->id, st->over[0], ms);
  }
}

// ----------------------------------------------------------------------------- go_launch's phases
// The query's workspace: *wsp freed of an earlier device result's rows (ws_release), then grown
// when the start list does not fit it.
static void go_workspace(GoQuery& q, const GoStarts& S, uint64_t num_starts, Workspace** wsp) {
  Engine& E = q.E;
  if (!q.lrc && *wsp) {   // rows of an earlier device result still there: hand the workspace to them
    const int32_t rrc = ws_release(E, wsp, q.stream);
    if (rrc) q.local_fail(rrc, E.last_error);
  }
  // room for a duplicated start list: the decision comes from the whole start list, the same on
  // every rank of a partitioned engine (its own share, f0, is at most that)
  const uint64_t need = q.part ? std::max<uint64_t>(num_starts, 1) : S.n;
  const uint64_t e_need = std::max<uint64_t>(E.snap.max_edges(), S.start_edges);
  if (!q.lrc && (!*wsp || need > ws_cap_frontier(*wsp) || S.n + S.start_edges > ws_cap_items(*wsp))) {
    const uint64_t fcap = std::max<uint64_t>({need, E.snap.nv + 1024, ws_cap_frontier(*wsp ? *wsp : nullptr)});
    std::string err;
    Workspace* fresh = ws_fresh(E, fcap, e_need, q.stream, q.qcomm, *wsp, &err);
    if (!fresh) {
      q.local_fail(NBG_E_OUT_OF_MEMORY, err);
    } else {
      if (*wsp) ws_destroy(*wsp);
      *wsp = fresh;
    }
  }
  q.ws = *wsp;
}

// The $- / $var input index of a statement, uploaded on its first execution.  False: nothing is
// held, and a later execution retries the upload from scratch.
static bool upload_input_index(nbg_go_stmt* st) {
  if (st->d_in_ids) return true;
  // `bytes` of h into a device array of at least one 8-byte entry
  auto up = [](auto** d, const void* h, size_t bytes) {
    return hipMalloc((void**)d, std::max<size_t>(bytes, 8)) == hipSuccess &&
           hipMemcpy(*d, h, bytes, hipMemcpyHostToDevice) == hipSuccess;
  };
  bool ok = up(&st->d_in_ids, st->in_ids.data(), st->in_ids.size() * 8);
  st->d_in_col_ptrs.assign(st->in_cols.size(), nullptr);
  for (size_t c = 0; ok && c < st->in_cols.size(); ++c)
    ok = up(&st->d_in_col_ptrs[c], st->in_cols[c].data(), st->in_cols[c].size() * 8);
  ok = ok && up(&st->d_in_cols, st->d_in_col_ptrs.data(), st->in_cols.size() * 8);
  if (ok && !st->in_xstr.empty()) {   // the input-string table (DevStrings::x*)
    std::vector<uint32_t> off{0};
    std::string bytes;
    for (const std::string& x : st->in_xstr) {
      bytes += x;
      off.push_back((uint32_t)bytes.size());
    }
    ok = bytes.size() < 0xFFFFFFFFull && up(&st->d_xoff, off.data(), off.size() * 4) &&
         up(&st->d_xbytes, bytes.data(), bytes.size());
  }
  if (!ok) st->free_input_index();
  return ok;
}

// Final-step row regions: per OVER position, ws_final_grid workgroups of ws_final_blk_cap rows
// each, one type's region after the other.  n_final bounds the frontier entering the final step,
// ebound[i] its edges of type i.
struct RowPlan {
  std::vector<uint64_t> region, blk_cap;
  uint64_t cap_rows = 0;
};
static RowPlan row_regions(uint64_t n_final, const std::vector<uint64_t>& ebound) {
  RowPlan rp;
  for (uint64_t eb : ebound) {
    rp.blk_cap.push_back(ws_final_blk_cap(n_final, eb));
    rp.region.push_back(rp.cap_rows);
    rp.cap_rows += rp.blk_cap.back() * ws_final_grid(n_final, eb);
  }
  return rp;
}

// Result rows of a statement whose final frontier is a step's SET (N >= 2): the plan go_launch
// makes per query, so a prepared statement's first execution allocates nothing.
static uint64_t stmt_row_bound(const Engine& E, const nbg_go_stmt* st) {
  std::vector<uint64_t> ebound;
  for (int32_t t : st->over) {
    auto it = E.snap.types.find(t);
    ebound.push_back(it == E.snap.types.end() ? 0 : it->second.num_edges);
  }
  return row_regions(E.snap.nv, ebound).cap_rows;
}

// The derived-string arena a query of cap_rows result rows reserves.
static uint64_t arena_size(const nbg_go_stmt* st, uint64_t cap_rows) {
  // derived strings: every final edge's OP_SOUTs may store up to the program's bound (the
  // longest text its piece lists can spell, plus each entry's header; ProgramBuilder::sout_bytes)
  // up to NBG_STR_ARENA_KB (default 2 GB); a query whose strings need more fails with
  // E_OUT_OF_MEMORY.  The bound covers every row the result can hold, so below the cap the
  // arena never overflows.
  static const uint64_t cap_kb =
      getenv("NBG_STR_ARENA_KB") ? strtoull(getenv("NBG_STR_ARENA_KB"), nullptr, 10) : (2ull << 20);
  // (a pad length read per edge leaves the bound unknown — ProgramBuilder::value_reg's 2^40 — so
  // such a statement reserves 256 bytes per row instead of the whole cap on every workspace, and a
  // query whose strings outgrow that fails with E_OUT_OF_MEMORY through the arena's overflow
  // flag, never truncates)
  const uint64_t per_row =
      st->sout_row_bytes >= (1ull << 40) ? 256 : std::max<uint64_t>(st->sout_row_bytes, 32);
  const uint64_t need = cap_rows > UINT64_MAX / per_row ? UINT64_MAX : cap_rows * per_row;
  return std::min<uint64_t>(std::max<uint64_t>(need, 1ull << 20), std::max<uint64_t>(cap_kb, 1) << 10);
}

// A small first hop travels as per-owner slot arrays instead of npad-bit bitmaps (ws_set_hop_slots:
// the single-root hop is one row on one rank, and sent 3.6 MB per rank at RMAT-26 / G = 8).  Its
// bound comes from the degrees every rank holds (Engine::first_hop_bound), so every rank — a
// failing one too — picks the same format.  NBG_GO_SLOTS=0 keeps bitmaps (read per query).
// Returns the slot stride, 0 for bitmaps.
static uint64_t hop1_slot_stride(const GoQuery& q, const int64_t* starts, uint64_t num_starts) {
  const nbg_go_stmt* st = q.st;
  if (!(q.part && st->steps >= 2 && st->over.size() == 1 && !(st->uses_input && st->steps > 1) &&
        !(getenv("NBG_GO_SLOTS") && atoi(getenv("NBG_GO_SLOTS")) == 0)))
    return 0;
  const uint64_t b = q.E.first_hop_bound(st->over[0], starts, num_starts, q.cap);
  const uint64_t stride = b == UINT64_MAX ? 0 : std::max<uint64_t>(64, (b + 63) / 64 * 64);
  return stride && stride * 4 * 2 <= q.E.npad / 8 ? stride : 0;
}

// ---- agreement: the query runs on every rank or on none.  A statement whose only collectives
// are the hop bitmaps and the statistics (no YIELD DISTINCT owner exchange, no $- / $var roots)
// needs no host round trip for it: a rank whose preparation failed still takes part in those
// collectives, with zero bitmaps and its status word in the statistics, and every rank fails the
// query when it reads them (go_collect).  Other statements agree first (Comm::agree).
// NBG_OK: every rank enqueues the query.  Else the query's code on this rank.
static int32_t go_agree(GoQuery& q, uint64_t hop1_slots, GoPending* p) {
  Engine& E = q.E;
  static const bool force_agree = getenv("NBG_GO_AGREE") && atoi(getenv("NBG_GO_AGREE")) != 0;
  // (YIELD DISTINCT too: its owner exchange runs in go_collect, which every rank leaves at the
  // in-band status before reaching it)
  const bool in_band = q.part && !q.st->uses_input && !force_agree;
  if (in_band) {
    if (q.lrc) {
      int32_t agreed = NBG_OK;
      const hipError_t he = part_empty_query(q.qcomm, q.stream, (int)q.st->steps - 1, E.fb_send, E.fb_recv, E.npad / 8,
                                             hop1_slots * 4, E.fb_gst, E.fb_hgst, q.lrc, &agreed);
      if (he != hipSuccess) {
        q.qcomm->abort();
        return E.fail(NBG_E_DEVICE, "query statistics exchange: " + q.qcomm->last);
      }
      p->finished = true;
      p->failed_rc = q.lrc;
      p->failed_msg = q.lmsg;
      return E.fail(q.lrc, q.lmsg);
    }
  } else if (q.part) {
    int32_t agreed = NBG_OK;
    ++E.host_agreements;
    if (q.qcomm->agree(q.stream, q.lrc, &agreed)) return E.fail(NBG_E_DEVICE, "query agreement: " + q.qcomm->last);
    if (agreed) {
      if (q.lrc) return E.fail(q.lrc, q.lmsg);
      return E.fail(agreed, "the query failed on another rank (code " + std::to_string(agreed) + ")");
    }
  } else if (q.lrc) {
    return E.fail(q.lrc, q.lmsg);
  }
  return NBG_OK;
}

// A tiny query — its walk bound (DevEdgeType::h_w2 / h_w3) keeps every step within one
// workgroup — runs as one launch (ws_go_tiny); NBG_TINY=0 turns it off.  The OVER type of a
// query that qualifies, else nullptr.
static const DevEdgeType* tiny_type(const GoQuery& q, const GoStarts& S, bool device) {
  const nbg_go_stmt* st = q.st;
  const TypeProgram& prog = st->plist[0];
  const uint32_t steps = st->steps;
  static const bool tiny_on = !getenv("NBG_TINY") || atoi(getenv("NBG_TINY")) != 0;
  if (!(tiny_on && !q.part && !device && !st->distinct && !st->uses_input && !st->derived && st->over.size() == 1 &&
        st->ncols > 0 && !st->deferred && !(prog.where_const && !prog.where_const_val) && S.inline_list() &&
        steps <= 3 && prog.nregs <= tiny_max_regs()))
    return nullptr;
  auto it = q.E.snap.types.find(st->over[0]);
  if (it == q.E.snap.types.end()) return nullptr;
  const DevEdgeType* tdt = &it->second;
  if (steps > 1 && !(tdt->h_w2.size() == q.E.snap.nv && tdt->h_w3.size() == q.E.snap.nv)) return nullptr;
  uint64_t bound = 0;
  if (steps == 1) bound = S.types[0].visible;
  else
    for (uint32_t d : S.f0) bound += steps == 2 ? tdt->h_w2[d] : tdt->h_w3[d];
  return bound <= TINY_EDGES ? tdt : nullptr;
}

// Steps 1..N on the workspace's stream: the MARK expansions and the frontier hand-over of every
// step but the last, then the final step's rows.  `he`: what ws_begin_query returned (a failure
// runs no step).
static hipError_t go_steps(GoQuery& q, const GoStarts& S, const RowPlan& plan, const std::vector<uint64_t>& ebound,
                           uint64_t hop1_slots, hipError_t he) {
  Engine& E = q.E;
  const std::vector<int32_t>& over = q.st->over;
  const std::vector<TypeProgram>& plist = q.st->plist;
  const uint32_t steps = q.st->steps;
  Workspace* ws = q.ws;
  uint64_t n_bound = S.n;
  ws_set_mark_claims(ws, over.size() == 1);
  const bool inject = q.part && E.fault(NBG_FAULT_DEVICE);
  for (uint32_t s = 1; he == hipSuccess && s <= steps; ++s) {
    const bool final = s == steps;
    // the next step's first OVER type: the next frontier list carries its edge space
    ExpandArgs next0{};
    const ExpandArgs* np0 = nullptr;
    if (!final) {
      auto it0 = E.snap.types.find(over[0]);
      if (it0 != E.snap.types.end()) {
        next0 = q.args_for(it0->second);
        if (s + 1 == steps && q.index_of(0)) next0.row_ptr = q.index_of(0)->rp;
        np0 = &next0;
      }
    }
    // (before the MARKs, on every rank: one without edges of the type runs none)
    if (s == 1 && !final && hop1_slots) he = ws_set_hop_slots(ws, hop1_slots);
    for (size_t i = 0; he == hipSuccess && i < over.size(); ++i) {
      auto it = E.snap.types.find(over[i]);
      if (it == E.snap.types.end()) continue;
      ExpandArgs a = q.args_for(it->second);
      a.bt_first = s == 1;
      if (!final) {
        he = ws_expand_mark(ws, a, n_bound, it->second.num_edges, (int)s, (int)i, S.inline_of(i, s), np0);
      } else if (q.st->deferred || (plist[i].where_const && !plist[i].where_const_val)) {
        he = ws_scan_only(ws, a, n_bound, (int)s, (int)i);
      } else if (const StmtIndex* ix = q.index_of(i)) {
        const uint32_t* const full = a.row_ptr;
        a.row_ptr = ix->rp;
        a.dst_vid = ix->dst;
        he = ws_expand_final(ws, a, n_bound, ebound[i], (int)s, (int)i, plist[i], plan.region[i], plan.blk_cap[i],
                             nullptr, full);
      } else {
        he = ws_expand_final(ws, a, n_bound, ebound[i], (int)s, (int)i, plist[i], plan.region[i], plan.blk_cap[i],
                             S.inline_of(i, s));
      }
    }
    if (inject) he = hipErrorLaunchFailure;   // NBG_FAULT_DEVICE: a device error between collectives
    if (!final && he == hipSuccess) {
      he = q.part ? ws_exchange(ws, (int)s, np0) : ws_finish_step(ws, (int)s, np0);
      n_bound = E.snap.nv;
    }
  }
  return he;
}

// The end of the query: the global statistics (partitioned) and the end-of-query kernel.
static hipError_t go_end(const GoQuery& q, const RowPlan& plan, bool device) {
  const nbg_go_stmt* st = q.st;
  Workspace* ws = q.ws;
  if (q.part) {
    const hipError_t he = ws_global_stats(ws, (int)st->over.size());
    if (he != hipSuccess) return he;
  }
  // a single engine's result that will be fetched to the host is packed there by the end-of-query
  // kernel when it is small (one host round trip less for it; YIELD DISTINCT compacts the rows
  // after this point, so it fetches them the usual way).  A device result (rows left in HBM) is
  // not: its end kernel is the one-workgroup state copy, a later nbg_rows_fetch copies the rows.
  if (q.part || st->distinct || st->ncols <= 0 || device) return ws_end_query_async(ws);
  SmallPack sp{};
  sp.ntypes = (int)st->over.size();
  sp.ncols = st->ncols;
  for (size_t i = 0; i < st->over.size(); ++i) {
    sp.region[i] = plan.region[i];
    sp.blk_cap[i] = plan.blk_cap[i];
    sp.grid[i] = ws_final_grid_of(ws, (int)i);
  }
  return ws_end_query_async_small(ws, sp);
}

// Enqueue the whole query (every step, the final-step rows and the end-of-query copy) on the
// workspace *wsp (its stream `stream`); no host synchronisation.  *wsp may be null (created here)
// or hold an earlier device result's rows (handed to it first, ws_release).
//
// Partitioned (every rank runs the same call): everything that can fail on one rank alone —
// workspace (re)creation, the input index, the back tracker, the start list's edge space, the
// row buffers — happens BEFORE the query's first collective and is agreed there (Comm::agree,
// one small all-reduce): either every rank enqueues the query or every rank returns the same
// code.  A device error after that point aborts the communicator (the peers' collectives fail).
// pre_rc: a failure the caller already had on this rank (nbg_go_submit's slot stream); it is
// reported through the same agreement as the preparation failures below, so the peers' collective
// sequence for the query still matches.
// sync: the caller waits for this query next (nbg_go_execute): its end kernel wakes the host by
// the mapped flag.  A submitted query is waited for by its event: the other slots' queries hide
// the wake-up, and the event lets the runtime retire finished work (six in flight ran ~1 %
// slower on the flag, profiles/r04_w/x_go_wake_ab*.txt).
// S: the query's start list (nbg_go_piped builds it from device rows; `starts` is then unused).
static int32_t go_launch_list(Engine& E, nbg_go_stmt* st, const GoStarts& S, const int64_t* starts, uint64_t num_starts,
                              bool device, Workspace** wsp, hipStream_t stream, Comm* qcomm, GoPending* p, bool sync,
                              int32_t pre_rc = NBG_OK, const char* pre_msg = nullptr) {
  const bool part = E.partitioned();
  if (part && !qcomm) return E.fail(NBG_E_STATE, "partitioned engine without a communicator");
  GoQuery q{E, st, stream, qcomm, part, E.edge_cap()};
  const std::vector<int32_t>& over = st->over;
  const uint32_t steps = st->steps;
  std::unique_ptr<nbg_rows> rows(new nbg_rows());
  rows->eng = &E;
  rows->ncols = st->ncols;
  rows->on_device = device;
  p->device = device;
  // (partitioned: every rank runs the same collective sequence, even with no local start)
  if (!S.n && !part) {
    p->finished = true;
    p->rows = std::move(rows);
    return NBG_OK;
  }
  if (pre_rc) q.local_fail(pre_rc, pre_msg ? pre_msg : "query set-up failed");
  if (E.fault(NBG_FAULT_ALLOC)) q.local_fail(NBG_E_OUT_OF_MEMORY, "query workspace allocation failed (injected)");
  // The start list keeps duplicates, so its edge space is the one list not bounded by a type's
  // edge count: the device lists carry it in 32 bits, and the workspace's merge-path tile splits
  // must cover it (on a partitioned engine each rank checks its own share).
  if (S.n + S.start_edges >= 0xFFFFFFFFull)   // merge-path items (entries + edges) are 32-bit too
    q.local_fail(NBG_E_UNSUPPORTED, "the start list's edges exceed 2^32-1 (duplicated hub starts)");
  go_workspace(q, S, num_starts, wsp);
  Workspace* ws = q.ws;
  if (ws) ws_set_wake(ws, sync);
  if (ws) ws_backtracker_off(ws);
  if (!q.lrc && st->uses_input) {
    if (!upload_input_index(st)) q.local_fail(NBG_E_OUT_OF_MEMORY, "input index upload");
    if (!q.lrc && steps > 1 && ws_backtracker(ws, &q.bt, &q.bt_in) != hipSuccess)
      q.local_fail(NBG_E_OUT_OF_MEMORY, "backtracker");
  }
  q.now = (int64_t)time(nullptr);
  q.seed = query_rand_seed();
  // final-step row regions: the frontier entering step N is a set (N >= 2) or the start list
  // (N == 1, exact edge count known on the host)
  std::vector<uint64_t> ebound(over.size(), 0);
  for (size_t i = 0; i < over.size(); ++i) {
    auto it = E.snap.types.find(over[i]);
    if (it != E.snap.types.end()) ebound[i] = steps == 1 ? S.types[i].all : it->second.num_edges;
  }
  RowPlan plan = row_regions(steps == 1 ? S.n : E.snap.nv, ebound);
  if (!q.lrc && ws_reserve_rows(ws, plan.cap_rows, st->ncols) != hipSuccess)
    q.local_fail(NBG_E_OUT_OF_MEMORY, "result rows");
  if (!q.lrc && st->derived && ws_reserve_arena(ws, arena_size(st, plan.cap_rows)) != hipSuccess)
    q.local_fail(NBG_E_OUT_OF_MEMORY, "derived-string arena");
  const uint64_t hop1_slots = hop1_slot_stride(q, starts, num_starts);
  if (int32_t rc = go_agree(q, hop1_slots, p)) return rc;
  p->ws = ws;
  rows->ws = ws;
  stmt_index_build(q);
  hipError_t he = S.pipe ? gopipe_list(S.pipe, ws, nullptr) : hipSuccess;
  if (he == hipSuccess)
    he = S.pipe ? ws_begin_query_resident(ws, S.n, &st->plist, st->id)
                : ws_begin_query(ws, S.f0.data(), S.f0.size(), &st->plist, st->id);
  if (const DevEdgeType* tdt = he == hipSuccess ? tiny_type(q, S, device) : nullptr) {
    he = ws_go_tiny(ws, q.args_for(*tdt), S.f0.data(), (uint32_t)S.f0.size(), steps, st->plist[0], st->ncols);
    if (he != hipSuccess) return E.fail(NBG_E_DEVICE, std::string("HIP: ") + hipGetErrorString(he));
    ++E.tiny_queries;
    p->region.assign(1, 0);
    p->blk_cap.assign(1, TINY_EDGES);
    p->rows = std::move(rows);
    return NBG_OK;
  }
  he = go_steps(q, S, plan, ebound, hop1_slots, he);
  if (he == hipSuccess) he = go_end(q, plan, device);
  if (he != hipSuccess) {
    // the peers may already wait in this query's next collective: release them
    if (part) qcomm->abort();
    const std::string cm = part && !qcomm->last.empty() ? " (" + qcomm->last + ")" : "";
    return E.fail(NBG_E_DEVICE, std::string("HIP: ") + hipGetErrorString(he) + cm);
  }
  p->region = std::move(plan.region);
  p->blk_cap = std::move(plan.blk_cap);
  p->rows = std::move(rows);
  return NBG_OK;
}

static int32_t go_launch(Engine& E, nbg_go_stmt* st, const int64_t* starts, uint64_t num_starts, bool device,
                         Workspace** wsp, hipStream_t stream, Comm* qcomm, GoPending* p, bool sync,
                         int32_t pre_rc = NBG_OK, const char* pre_msg = nullptr) {
  if (num_starts && !starts) return E.fail(NBG_E_INVALID_ARGUMENT, "null argument");
  if (hipSetDevice(E.cfg.device) != hipSuccess) return E.fail(NBG_E_DEVICE, "hipSetDevice failed");
  const GoStarts S(E, *st, starts, num_starts, E.edge_cap());
  return go_launch_list(E, st, S, starts, num_starts, device, wsp, stream, qcomm, p, sync, pre_rc, pre_msg);
}

// ----------------------------------------------------------------------------- go_collect's phases
// The text of every derived-string code in a result (nbg_rows::derived): the arena entries the
// query's OP_SOUT stored, and the statement's constants that carry the hash code.  Partitioned
// with YIELD DISTINCT, rows have moved between ranks, so every rank's entries are all-gathered
// (each rank runs this for the same query, in submission order).
static int32_t derived_strings(Engine& E, const nbg_go_stmt* st, Workspace* ws, uint64_t used, bool gather,
                               nbg_rows* rows) {
  std::vector<char> buf;
  std::vector<std::pair<uint64_t, uint64_t>> parts;   // (offset, bytes) per rank in buf
  if (!gather) {
    if (ws_read_arena(ws, used, &buf) != hipSuccess) return E.fail(NBG_E_DEVICE, "derived-string arena read");
    parts.emplace_back(0, used);
  } else {
    Comm* cm = ws_get_comm(ws);
    hipStream_t s = ws_stream(ws);
    std::vector<uint64_t> sizes;
    const uint64_t u = used;
    if (cm->gather_u64(s, &u, 1, &sizes)) return E.fail(NBG_E_DEVICE, "derived strings: " + cm->last);
    uint64_t mx = 8;
    for (uint64_t x : sizes) mx = std::max(mx, x);
    uint64_t cap = 0;
    const char* arena = ws_arena(ws, &cap);
    char *send = nullptr, *recv = nullptr;
    bool ok = hipMalloc((void**)&recv, mx * sizes.size()) == hipSuccess;
    if (ok && cap < mx) ok = hipMalloc((void**)&send, mx) == hipSuccess &&
                             (!used || hipMemcpyAsync(send, arena, used, hipMemcpyDeviceToDevice, s) == hipSuccess);
    // (a rank that cannot allocate cannot take part: the communicator is aborted, as for any
    // device failure between collectives)
    ok = ok && cm->allgather(send ? send : arena, recv, mx, s) == 0;
    buf.resize(mx * sizes.size());
    ok = ok && hipMemcpyAsync(buf.data(), recv, buf.size(), hipMemcpyDeviceToHost, s) == hipSuccess &&
         hipStreamSynchronize(s) == hipSuccess;
    if (send) (void)hipFree(send);
    if (recv) (void)hipFree(recv);
    if (!ok) {
      cm->abort();
      return E.fail(NBG_E_DEVICE, "derived strings all-gather");
    }
    for (size_t q = 0; q < sizes.size(); ++q) parts.emplace_back(q * mx, sizes[q]);
  }
  auto add = [&](int64_t code, std::string text) {
    auto it = rows->derived.find(code);
    if (it == rows->derived.end()) rows->derived.emplace(code, std::move(text));
    else if (it->second != text) return false;   // two strings with one 62-bit hash
    return true;
  };
  for (auto& pr : parts) {
    for (uint64_t o = pr.first; o + 16 <= pr.first + pr.second;) {
      int64_t code;
      uint64_t len;
      memcpy(&code, buf.data() + o, 8);
      memcpy(&len, buf.data() + o + 8, 8);
      if (o + 16 + len > pr.first + pr.second) return E.fail(NBG_E_DEVICE, "derived-string arena entry");
      // (an OP_SMAT entry, code 0, is a nested function's inner string: no result cell holds it)
      if (is_derived_code(code) && !add(code, std::string(buf.data() + o + 16, len)))
        return E.fail(NBG_E_EXECUTION_ERROR, "derived-string hash collision");
      o += 16 + ((len + 7) & ~7ull);
    }
  }
  for (const TypeProgram& tp : st->plist)
    for (size_t y = 0; y < tp.yield_const.size(); ++y)
      if (tp.yield_reg[y] < 0 && tp.yield_kind[y] == VK_STRING && is_derived_code(tp.yield_const[y]) &&
          !add(tp.yield_const[y], tp.yield_const_str[y]))
        return E.fail(NBG_E_EXECUTION_ERROR, "derived-string hash collision");
  return NBG_OK;
}

// statistics of the whole query: this engine's, or summed over all ranks when partitioned
struct GoStats {
  unsigned long long err, n[MAX_STEPS + 2], e[MAX_STEPS + 2], tagbits;
};
static GoStats go_stats(const Engine& E, const nbg_go_stmt* st, Workspace* ws, const QState& q) {
  GoStats g{q.err, {}, {}, q.tagbits};
  if (E.partitioned()) {
    ws_host_gstats(ws, &g.err, g.n, g.e, &g.tagbits);
  } else {
    for (int s = 0; s < MAX_STEPS + 2; ++s) {
      g.n[s] = q.step_n[s];
      g.e[s] = 0;
      for (size_t i = 0; i < st->over.size(); ++i) g.e[s] += q.e_st[s][i];
    }
  }
  return g;
}

// What the query's statistics say of its outcome, the first that applies.
static int32_t go_status(Engine& E, const nbg_go_stmt* st, const QState& q, const GoStats& g) {
  const uint32_t steps = st->steps;
  const bool reached_final = g.n[steps] > 0;
  if (reached_final && st->deferred) return E.fail(st->deferred, st->deferred_msg);
  if (reached_final && g.e[steps] > 0 && !st->dst_unknown.empty()) return E.fail(NBG_E_EXECUTION_ERROR, st->dst_unknown);
  if (g.err >= SPLIT_BAD)
    return E.fail(NBG_E_DEVICE, "internal: a frontier list's merge-path split did not describe its tile");
  if (g.err >= ARENA_OVERFLOW)
    return E.fail(NBG_E_OUT_OF_MEMORY, "the derived strings of the result need " + std::to_string(q.arena_used >> 10) +
                                       " KB, more than the string arena's cap (NBG_STR_ARENA_KB)");
  if (g.err) return E.fail(NBG_E_EXECUTION_ERROR, "WHERE/YIELD evaluation error");
  // a $$ default read for a tag no final destination has: VertexHolder::defaultFor fails
  if ((g.tagbits >> MAX_TAG_BITS) & ~g.tagbits & ((1ull << MAX_TAG_BITS) - 1))
    return E.fail(NBG_E_EXECUTION_ERROR, "Unknown Vertex");
  return NBG_OK;
}

// YIELD DISTINCT on the device: segments deduplicated and compacted in place; partitioned,
// the survivors then travel to the rank their identity hashes to, which deduplicates again
// (every rank takes part: the exchange is collective)
static int32_t go_distinct(Engine& E, Workspace* ws, int ncols, nbg_rows* rows) {
  auto segments = [&](std::vector<std::pair<size_t, size_t>>* where) {
    std::vector<std::array<uint64_t, 3>> segs;
    for (size_t i = 0; i < rows->blocks.size(); ++i) {
      const auto& tb = rows->blocks[i];
      for (size_t b = 0; b < tb.counts.size(); ++b) {
        if (!tb.counts[b]) continue;
        segs.push_back({tb.region + (uint64_t)b * tb.blk_cap, tb.counts[b], (uint64_t)i});
        if (where) where->emplace_back(i, b);
      }
    }
    return segs;
  };
  std::vector<std::pair<size_t, size_t>> where;   // (type, block) of each segment
  std::vector<std::array<uint64_t, 3>> segs = segments(&where);
  std::vector<uint32_t> kept;
  hipError_t de = ws_distinct(ws, segs, ncols, rows->kinds, &kept);
  rows->count = 0;
  for (size_t k = 0; de == hipSuccess && k < segs.size(); ++k) {
    rows->blocks[where[k].first].counts[where[k].second] = kept[k];
    rows->count += kept[k];
  }
  if (E.partitioned()) {
    // the exchange is collective: every rank takes part, a rank whose dedup pass failed with no
    // rows and its status, which travels with the exchange's counts (no agreement of its own)
    std::vector<DistinctBlock> db;
    int32_t gstatus = NBG_OK;
    const int32_t mine = de == hipSuccess ? NBG_OK : NBG_E_DEVICE;
    de = ws_distinct_exchange(ws, mine ? std::vector<std::array<uint64_t, 3>>{} : segments(nullptr), ncols,
                              rows->kinds, &db, mine, &gstatus);
    if (de == hipSuccess && gstatus)
      return E.fail(gstatus, mine ? std::string("YIELD DISTINCT: the dedup pass failed")
                                  : "YIELD DISTINCT failed on another rank (code " + std::to_string(gstatus) + ")");
    rows->count = 0;
    for (size_t i = 0; de == hipSuccess && i < rows->blocks.size() && i < db.size(); ++i) {
      rows->blocks[i].region = db[i].region;
      rows->blocks[i].blk_cap = db[i].blk_cap;
      rows->blocks[i].counts = db[i].counts;
      for (uint32_t c : db[i].counts) rows->count += c;
    }
  }
  if (de != hipSuccess) {
    // a failure inside the owner exchange (after its first collective) leaves the peers in the
    // later collectives of this query: abort the communicator, as for any device failure
    // between collectives, so they fail at once instead of at NBG_COMM_TIMEOUT_S
    if (E.partitioned()) ws_get_comm(ws)->abort();
    return E.fail(NBG_E_DEVICE, std::string("HIP (distinct): ") + hipGetErrorString(de));
  }
  return NBG_OK;
}

// Wait for a launched query and build its result.  The rows are the caller's only when the query
// succeeded: every failure frees them.
static int32_t go_collect(Engine& E, nbg_go_stmt* st, GoPending* p, nbg_rows** out) {
  std::unique_ptr<nbg_rows> rows = std::move(p->rows);
  if (p->failed_rc) return E.fail(p->failed_rc, p->failed_msg);
  if (p->finished) { *out = rows.release(); return NBG_OK; }
  Workspace* ws = p->ws;
  const hipError_t he = ws_end_query_wait(ws);
  if (he != hipSuccess) return E.fail(NBG_E_DEVICE, std::string("HIP: ") + hipGetErrorString(he));
  if (E.partitioned()) {   // a rank whose preparation failed (go_launch, in-band statuses)
    const int32_t code = ws_host_gstatus(ws);
    if (code) return E.fail(code, "the query failed on another rank (code " + std::to_string(code) + ")");
  }
  const QState& q = *ws_host_state(ws);
  const GoStats g = go_stats(E, st, ws, q);
  for (uint32_t s = 1; s <= st->steps; ++s) {
    rows->step_frontier.push_back(g.n[s]);
    rows->step_edges.push_back(g.e[s]);
    rows->scanned += g.e[s];
  }
  st->final_scanned += g.e[st->steps];
  if (int32_t rc = go_status(E, st, q, g)) return rc;
  rows->col_types = st->col_types;
  rows->wclass = st->wclass;
  rows->misaligned = st->misaligned;
  rows->float_col = st->float_col;
  for (size_t i = 0; i < st->over.size(); ++i) {
    rows->kinds.push_back(st->plist[i].yield_kind);
    rows->const_str.push_back(st->plist[i].yield_const_str);
    const unsigned grid = ws_final_grid_of(ws, (int)i);   // 0: the final expansion did not run
    const uint32_t* per_block = ws_host_blk_rows(ws, (int)i);
    nbg_rows::TypeBlocks tb;
    tb.region = p->region[i];
    tb.blk_cap = p->blk_cap[i];
    tb.counts.assign(per_block, per_block + grid);
    uint64_t c = 0;
    for (uint32_t x : tb.counts) c += x;
    rows->count += c;
    rows->blocks.push_back(std::move(tb));
  }
  if (st->distinct && (rows->count || E.partitioned()))
    if (int32_t rc = go_distinct(E, ws, st->ncols, rows.get())) return rc;
  if (st->derived)
    if (int32_t rc = derived_strings(E, st, ws, q.arena_used, E.partitioned() && st->distinct, rows.get())) return rc;
  // the hand-over: host rows are fetched now, device rows keep the workspace
  for (int c = 0; c < st->ncols; ++c) rows->dcols.push_back(ws_row_col(ws, c));
  rows->small_ok = !E.partitioned() && !st->distinct && !p->device;   // (go_launch packed a small result)
  if (!p->device) {
    int32_t rc = materialize_rows(rows.get());
    if (rc) return rc == NBG_E_EXECUTION_ERROR || rc == NBG_E_DEVICE ? rc : E.fail(rc, "row fetch failed");
  } else if (rows->count) {
    E.holders[ws] = rows.get();   // the rows stay valid until nbg_rows_free (ws_release)
  }
  *out = rows.release();
  return NBG_OK;
}

static int32_t go_execute(Engine& E, nbg_go_stmt* st, const int64_t* starts, uint64_t num_starts, bool device,
                          nbg_rows** out) {
  if (!out) return E.fail(NBG_E_INVALID_ARGUMENT, "null argument");
  *out = nullptr;
  GoPending p;
  if (int32_t rc = go_launch(E, st, starts, num_starts, device, &E.ws, E.stream, E.comm.get(), &p, true)) return rc;
  return go_collect(E, st, &p, out);
}

static int32_t go_impl(Engine& E, const nbg_go_request* rq, bool device, nbg_rows** out) {
  std::lock_guard<std::mutex> lg(E.mu);
  nbg_go_stmt* st = nullptr;
  if (int32_t rc = go_prepare(E, rq, &st)) return rc;
  const std::unique_ptr<nbg_go_stmt> own(st);
  return go_execute(E, st, rq->starts, rq->num_starts, device, out);
}

// ----------------------------------------------------------------------------- GO over device rows
// nbg_go_piped: GoExecutor::setupStarts (GoExecutor.cpp:365-399) over a device-resident result.  The
// statement is prepared as nbg_go prepares it; the start list and the input index come from
// gopipe.hip; everything after the start list is go_launch_list / go_collect.  The numbered steps
// are the statuses of include/nbg.h, in their order.
static int32_t go_piped(Engine& E, const nbg_rows* in, const nbg_go_request* rq, bool device, nbg_rows** out) {
  // ---- 1. arguments
  if (in->eng != &E) return E.fail(NBG_E_INVALID_ARGUMENT, "GO FROM $-: the rows belong to another engine");
  if (!in->on_device) return E.fail(NBG_E_INVALID_ARGUMENT, "GO FROM $-: the rows are host-only (not a device result)");
  if (!rq->input_names) return E.fail(NBG_E_INVALID_ARGUMENT, "GO FROM $-: null input column names");
  if (rq->num_input_cols != in->ncols)
    return E.fail(NBG_E_INVALID_ARGUMENT, "GO FROM $-: " + std::to_string(rq->num_input_cols) + " input column names for " +
                                              std::to_string(in->ncols) + " columns");
  for (int32_t c = 0; c < rq->num_input_cols; ++c)
    if (!rq->input_names[c]) return E.fail(NBG_E_INVALID_ARGUMENT, "GO FROM $-: null input column name");
  const int vcol = rq->input_vid_col;
  if (vcol < 0 || vcol >= in->ncols) return E.fail(NBG_E_INVALID_ARGUMENT, "GO FROM $-: the FROM column is out of range");
  if (rq->num_yields < 0 || (rq->num_yields > 0 && (!rq->yields || !rq->yield_lens)))
    return E.fail(NBG_E_INVALID_ARGUMENT, "GO FROM $-: null argument");
  {
    std::string err;
    if (rq->where && rq->where_len && !decode_expr(rq->where, rq->where_len, &err))
      return E.fail(NBG_E_INVALID_ARGUMENT, "WHERE: " + err);
    for (int32_t i = 0; i < rq->num_yields; ++i)
      if (!decode_expr(rq->yields[i], rq->yield_lens[i], &err)) return E.fail(NBG_E_INVALID_ARGUMENT, "YIELD: " + err);
  }
  // ---- 2.
  if (E.partitioned())
    return E.fail(NBG_E_UNSUPPORTED, "GO FROM $- on a partitioned engine (its rows live on several ranks)");
  // ---- 3. prepare() runs before setupStarts: diagnosed for an empty input too
  nbg_go_stmt* stp = nullptr;
  if (int32_t rc = go_prepare(E, rq, &stp, in)) return rc;
  const std::unique_ptr<nbg_go_stmt> own(stp);
  nbg_go_stmt* st = stp;
  if (hipSetDevice(E.cfg.device) != hipSuccess) return E.fail(NBG_E_DEVICE, "hipSetDevice failed");
  const uint32_t cap = E.edge_cap();
  GoPending p;
  auto run = [&](const GoStarts& S) {
    if (int32_t rc = go_launch_list(E, st, S, nullptr, 0, device, &E.ws, E.stream, E.comm.get(), &p, true)) return rc;
    return go_collect(E, st, &p, out);
  };
  // ---- 4. no rows: setupStarts returns before getVIDs, then onEmptyInputs
  if (!in->count) return run(GoStarts(E, *st, nullptr, 0, cap));
  // ---- 5. getVIDs -> RowReader::getVid (RowReader.cpp:569-576): INT and VID columns only
  const int vkind = in->col_kind(vcol);
  const int32_t vtype = vcol < (int)in->col_types.size() && in->col_types[vcol] ? in->col_types[vcol]
                        : vkind == VK_DOUBLE ? NBG_T_DOUBLE : vkind == VK_BOOL ? NBG_T_BOOL
                        : vkind == VK_STRING ? NBG_T_STRING : NBG_T_INT;
  if ((vkind >= 0 && vkind != VK_INT) || (vtype != NBG_T_INT && vtype != NBG_T_VID))
    return E.fail(NBG_E_EXECUTION_ERROR, std::string("Column `") + rq->input_names[vcol] + "' not found");
  // ---- 6. device scope
  if (in->misaligned || in->float_col)
    return E.fail(NBG_E_UNSUPPORTED, "GO FROM $-: the input's row schema re-reads its columns (misaligned or FLOAT)");
  if (vkind < 0) return E.fail(NBG_E_UNSUPPORTED, std::string("GO FROM $-: column `") + rq->input_names[vcol] + "' mixes value kinds");
  uint32_t refs = 0;   // the input columns WHERE / YIELD read (OP_INPUT's aux)
  for (const TypeProgram& tp : st->plist)
    for (const Ins& i : tp.code)
      if (i.op == OP_INPUT && i.aux >= 0 && i.aux < in->ncols) refs |= 1u << i.aux;
  for (int c = 0; c < in->ncols; ++c) {
    if (!((refs >> c) & 1u)) continue;
    const int k = in->col_kind(c);
    if (k < 0) return E.fail(NBG_E_UNSUPPORTED, std::string("GO FROM $-: column `") + rq->input_names[c] + "' mixes value kinds");
    bool outside = !in->derived.empty();
    for (auto& cs : in->const_str) outside = outside || ((int)cs.size() > c && !cs[c].empty());
    if (k == VK_STRING && outside)
      return E.fail(NBG_E_UNSUPPORTED, std::string("GO FROM $-: string column `") + rq->input_names[c] +
                                           "' can hold strings outside the dictionary");
  }
  if (in->count > 0xFFFFFFFFull) return E.fail(NBG_E_UNSUPPORTED, "GO FROM $-: an input of 2^32 rows or more");
  if (!E.snap.d_vids || in->ncols > MAX_YIELDS) return E.fail(NBG_E_UNSUPPORTED, "GO FROM $-: vertex table missing");
  // ---- 7. the join and the counts, one read-back
  auto* m = const_cast<nbg_rows*>(in);
  m->build_segs();
  std::vector<std::pair<uint64_t, uint64_t>> segs;
  for (auto& sg : m->segs)
    if (sg.end > sg.begin) segs.emplace_back(sg.begin, sg.end - sg.begin);
  Workspace* inw = in->owned_ws ? in->owned_ws : in->ws;
  if (!inw) return E.fail(NBG_E_INVALID_ARGUMENT, "GO FROM $-: the rows have no device workspace");
  GpPlan gp;
  gp.vid_col = vcol;
  gp.vids = E.snap.d_vids;
  gp.nv = E.snap.nv;
  gp.distinct = st->distinct;
  gp.index = st->uses_input;
  gp.cap = cap;
  std::vector<int> slot(st->over.size(), -1);   // OVER position -> GpCounts::deg entry
  for (size_t i = 0; i < st->over.size(); ++i) {
    auto it = E.snap.types.find(st->over[i]);
    if (it == E.snap.types.end() || !it->second.row_ptr) continue;
    slot[i] = gp.ntypes;
    gp.row_ptr[gp.ntypes++] = it->second.row_ptr;
  }
  GoPipe* pipe = nullptr;
  GpCounts got{};
  std::string err;
  if (int32_t rc = gopipe_open(inw, E.stream, segs, gp, &E.gp_prof, &pipe, &got, &err)) return E.fail(rc, err);
  const std::unique_ptr<GoPipe, void (*)(GoPipe*)> closer(pipe, gopipe_close);   // (after the query's last wait)
  const uint64_t nlist = st->distinct ? got.unique : got.found;
  if (!nlist) return run(GoStarts(E, *st, nullptr, 0, cap));
  // the input index, owned by this one-shot statement (freed with it)
  if (st->uses_input) {
    const hipError_t he = gopipe_index(pipe, refs, in->ncols, &st->d_in_ids, &st->d_in_col_ptrs);
    bool ok = he == hipSuccess;
    ok = ok && hipMalloc((void**)&st->d_in_cols, std::max<size_t>(st->d_in_col_ptrs.size(), 1) * 8) == hipSuccess &&
         hipMemcpyAsync(st->d_in_cols, st->d_in_col_ptrs.data(), st->d_in_col_ptrs.size() * 8, hipMemcpyHostToDevice,
                        E.stream) == hipSuccess;
    if (!ok) {
      (void)hipGetLastError();
      return E.fail(he == hipSuccess || he == hipErrorOutOfMemory ? NBG_E_OUT_OF_MEMORY : NBG_E_DEVICE, "GO FROM $-: input index");
    }
    st->in_n = got.unique;
  }
  // a short list is read back and takes the host start-list path (the inline list, the tiny path)
  if (nlist <= (uint64_t)INLINE_STARTS) {
    std::vector<uint32_t> dense(nlist);
    if (gopipe_list(pipe, nullptr, dense.data()) != hipSuccess) return E.fail(NBG_E_DEVICE, "GO FROM $-: start list read");
    return run(GoStarts(E, *st, std::move(dense), cap));
  }
  std::vector<uint64_t> all(st->over.size(), 0);
  for (size_t i = 0; i < st->over.size(); ++i)
    if (slot[i] >= 0) all[i] = got.deg[slot[i]];
  return run(GoStarts(*st, pipe, nlist, all));
}

}  // namespace

// ============================================================================= asynchronous GO
// Up to NBG_QUERY_SLOTS queries of one engine in flight: each on its own workspace and HIP
// stream, so the device overlaps one query's latency-bound small launches with another's
// expansion (graphd serves concurrent queries the same way, one executor per query).
struct nbg_go_ticket {
  nbg_go_stmt* st = nullptr;
  int slot = -1;
  GoPending p;
  bool done = false;
  int32_t rc = NBG_OK;
  nbg_rows* result = nullptr;
};

static int query_slots() {
  static const int n = [] {
    const char* v = getenv("NBG_QUERY_SLOTS");
    const int k = v ? atoi(v) : 6;
    return k < 1 ? 1 : (k > 16 ? 16 : k);
  }();
  return n;
}

// complete the oldest submitted ticket (its result stays in the ticket until nbg_go_wait)
static void complete_oldest(Engine& E) {
  auto* t = static_cast<nbg_go_ticket*>(E.inflight.front());
  E.inflight.erase(E.inflight.begin());
  t->rc = go_collect(E, t->st, &t->p, &t->result);
  t->done = true;
  E.slots[t->slot].ticket = nullptr;
}

void nbg::go_drain(Engine& E) {
  while (!E.inflight.empty()) {
    auto* t = static_cast<nbg_go_ticket*>(E.inflight.front());
    complete_oldest(E);
    if (t->result) nbg_rows_free(t->result);
    t->result = nullptr;
    delete t;
  }
}

// ============================================================================= C ABI
extern "C" {

int32_t nbg_go_submit(nbg_go_stmt* st, const int64_t* starts, uint64_t num_starts, int32_t device,
                      nbg_go_ticket** out) {
  if (!st || !st->eng || !out) return NBG_E_INVALID_ARGUMENT;
  Engine& E = *st->eng;
  std::lock_guard<std::mutex> lg(E.mu);
  *out = nullptr;
  if (hipSetDevice(E.cfg.device) != hipSuccess) return E.fail(NBG_E_DEVICE, "hipSetDevice failed");
  if (E.slots.empty()) E.slots.resize(query_slots());
  int slot = -1;
  for (size_t i = 0; i < E.slots.size() && slot < 0; ++i)
    if (!E.slots[i].ticket) slot = (int)i;
  if (slot < 0) {   // every slot busy: finish the oldest query first
    const int s0 = static_cast<nbg_go_ticket*>(E.inflight.front())->slot;
    complete_oldest(E);
    slot = s0;
  }
  Engine::QuerySlot& q = E.slots[slot];
  // A partitioned engine's queries are collectives.  Each slot gets its own communicator (a
  // split of the engine's, made collectively the first time the slot is used: every rank submits
  // the same queries in the same order, so it picks the same slot at the same call), and so its
  // own stream: the ranks issue every communicator's collectives in one order, and queries of
  // different slots overlap on the device.  Without a split (in-process transport, or
  // NBG_SLOT_COMMS=0) the slots share the engine's stream and communicator, one query after
  // another on the device.
  if (E.partitioned() && !q.comm_tried) {
    q.comm_tried = true;
    static const bool split_ok = !getenv("NBG_SLOT_COMMS") || atoi(getenv("NBG_SLOT_COMMS")) != 0;
    if (split_ok) {
      std::string err;
      q.comm.reset(E.comm->split(&err));
      // the split is collective: keep it only if every rank got one (else all share the engine's)
      if (E.comm->kind() != std::string("local")) {
        int32_t agreed = NBG_OK;
        if (E.comm->agree(E.stream, q.comm ? NBG_OK : NBG_E_DEVICE, &agreed))
          return E.fail(NBG_E_DEVICE, "slot communicator agreement: " + E.comm->last);
        if (agreed) q.comm.reset();
      }
    }
  }
  const bool own_stream = !E.partitioned() || q.comm != nullptr;
  Comm* const qcomm = q.comm ? q.comm.get() : E.comm.get();
  hipStream_t qstream = own_stream ? q.stream : E.stream;
  int32_t pre_rc = NBG_OK;
  const bool stream_fault = own_stream && E.fault(NBG_FAULT_STREAM);
  if (own_stream && (!q.stream || stream_fault)) {
    if (stream_fault || hipStreamCreateWithFlags(&q.stream, hipStreamNonBlocking) != hipSuccess) {
      if (!stream_fault) q.stream = nullptr;
      if (!E.partitioned()) return E.fail(NBG_E_DEVICE, "hipStreamCreate failed");
      // the peers run this query's collectives (in band or an agreement, per statement): fail it
      // with them through go_launch, on the engine's stream
      pre_rc = NBG_E_DEVICE;
      qstream = E.stream;
    } else {
      qstream = q.stream;
    }
  }
  auto* t = new nbg_go_ticket();
  t->st = st;
  t->slot = slot;
  int32_t rc = go_launch(E, st, starts, num_starts, device != 0, &q.ws, qstream, qcomm, &t->p, false, pre_rc,
                         "hipStreamCreate failed");
  // an in-band failure keeps its slot like any submitted query (the peers' slot holds theirs);
  // nbg_go_wait returns the code
  if (rc && !t->p.failed_rc) { delete t; return rc; }
  q.ticket = t;
  E.inflight.push_back(t);
  *out = t;
  return NBG_OK;
}

int32_t nbg_go_wait(nbg_go_ticket* t, nbg_rows** out) {
  if (!t || !out) return NBG_E_INVALID_ARGUMENT;
  Engine& E = *t->st->eng;
  std::lock_guard<std::mutex> lg(E.mu);
  *out = nullptr;
  if (!t->done) {
    // complete every older ticket first (their results stay in their tickets)
    while (!E.inflight.empty() && E.inflight.front() != t) complete_oldest(E);
    complete_oldest(E);
  }
  const int32_t rc = t->rc;
  *out = t->result;
  delete t;
  return rc;
}

int32_t nbg_go(nbg_engine* h, const nbg_go_request* req, nbg_rows** out) {
  if (!h) return NBG_E_INVALID_ARGUMENT;
  return go_impl(h->e, req, false, out);
}

int32_t nbg_go_device(nbg_engine* h, const nbg_go_request* req, nbg_rows** out) {
  if (!h) return NBG_E_INVALID_ARGUMENT;
  return go_impl(h->e, req, true, out);
}

int32_t nbg_go_piped(nbg_engine* h, const nbg_rows* in, const nbg_go_request* req, int32_t device, nbg_rows** out) {
  if (!h || !in || !req || !out) return NBG_E_INVALID_ARGUMENT;
  *out = nullptr;
  std::lock_guard<std::mutex> lg(h->e.mu);
  return go_piped(h->e, in, req, device != 0, out);
}

int32_t nbg_go_default_columns(nbg_engine* h, const int32_t* over, int32_t n, int32_t over_all, int32_t* out,
                               int32_t cap) {
  if (!h || n < 0 || (n && !over) || (cap && !out)) return NBG_E_INVALID_ARGUMENT;
  std::vector<int32_t> req(over, over + n);
  if (over_all) req = response_schema_order(req);
  for (int32_t i = 0; i < cap && i < (int32_t)req.size(); ++i) out[i] = req[i];
  return (int32_t)req.size();
}

int32_t nbg_go_prepare(nbg_engine* h, const nbg_go_request* req, nbg_go_stmt** out) {
  if (!h) return NBG_E_INVALID_ARGUMENT;
  Engine& E = h->e;
  std::lock_guard<std::mutex> lg(E.mu);
  const int32_t rc = go_prepare(E, req, out);
  if (rc || (*out)->steps < 2) return rc;
  {   // the filtered-adjacency switches, read per statement (nbg.h)
    nbg_go_stmt* st = *out;
    const char* on = getenv("NBG_STMT_INDEX");
    const char* after = getenv("NBG_STMT_INDEX_AFTER");
    const char* mb = getenv("NBG_STMT_INDEX_MB");
    st->idx_on = !(on && atoi(on) == 0);
    if (after) st->idx_after = std::max(0.0, atof(after));
    if (mb) st->idx_budget = strtoull(mb, nullptr, 10) << 20;
  }
  // GoExecutor::prepare() validates once and execute() then only runs: size the row buffers of
  // the engine's workspace and of every query slot's now (growing a multi-GB buffer inside the
  // first execution cost that query ~0.2 s at RMAT-26).  A failure here is not an error: the
  // query grows (or fails) on its own.
  if (hipSetDevice(E.cfg.device) != hipSuccess) return NBG_OK;
  const uint64_t rows = stmt_row_bound(E, *out);
  auto reserve = [&](Workspace* w) {
    if (w && !E.holders.count(w)) (void)ws_reserve_rows(w, rows, (*out)->ncols);
  };
  reserve(E.ws);
  for (auto& q : E.slots) reserve(q.ws);
  E.row_reserve = std::max(E.row_reserve, rows);
  E.col_reserve = std::max(E.col_reserve, (*out)->ncols);
  return NBG_OK;
}

int32_t nbg_go_execute(nbg_go_stmt* st, const int64_t* starts, uint64_t num_starts, int32_t device, nbg_rows** out) {
  if (!st || !st->eng) return NBG_E_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lg(st->eng->mu);
  return go_execute(*st->eng, st, starts, num_starts, device != 0, out);
}

void nbg_go_stmt_free(nbg_go_stmt* st) { delete st; }

uint64_t nbg_go_stmt_index_bytes(const nbg_go_stmt* st) {
  if (!st || !st->eng) return 0;
  std::lock_guard<std::mutex> lg(st->eng->mu);
  return st->idx.bytes;
}

}  // extern "C"
