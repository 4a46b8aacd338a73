// The stages over device-resident rows at the C ABI (include/nbg.h): nbg_group_by, nbg_order_by,
// nbg_set_op, nbg_yield, nbg_yield_agg, nbg_fetch_vertices, nbg_fetch_edges, nbg_rows_encode and
// nbg_rows_decode.  Each plans its request on the host, as its executor in the reference checks it, and
// hands the plan to its driver (groupby.hip, orderby.hip, setops.hip, yieldrows.hip, yieldagg.hip,
// fetchrows.hip, fetchedges.hip, rowenc.hip, rowdec.hip).
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <set>

#include "nbg_rows.h"
#include "rowdec.h"
#include "rowenc.h"

using namespace nbg;

// ============================================================================= what the stages share
// Small checks and steps, each called where the stage's own executor stands: the order of a
// stage's checks is the reference's, and it decides which status wins.
namespace {

using Segs = std::vector<std::pair<uint64_t, uint64_t>>;   // (first row, rows)

int32_t natural_type_of(VKind k) {
  return k == VK_DOUBLE ? NBG_T_DOUBLE : k == VK_BOOL ? NBG_T_BOOL : k == VK_STRING ? NBG_T_STRING : NBG_T_INT;
}

nbg_rows* new_rows(Engine& E, int ncols) {
  auto* r = new nbg_rows();
  r->eng = &E;
  r->ncols = ncols;
  r->on_device = true;
  r->kinds.emplace_back(ncols, VK_INT);
  r->const_str.emplace_back(ncols, std::string());
  r->col_types.assign(ncols, NBG_T_INT);
  r->wclass.emplace_back(ncols, (uint8_t)W_ID);
  return r;
}

// rows of another engine, then host-only rows, over every input of the stage
int32_t guard_rows(Engine& E, const std::string& label, std::initializer_list<const nbg_rows*> rows) {
  for (const nbg_rows* r : rows)
    if (r->eng != &E) return E.fail(NBG_E_INVALID_ARGUMENT, label + ": the rows belong to another engine");
  for (const nbg_rows* r : rows)
    if (!r->on_device) return E.fail(NBG_E_INVALID_ARGUMENT, label + ": the rows are host-only (not a device result)");
  return NBG_OK;
}

int32_t guard_partitioned(Engine& E, const std::string& label) {
  if (!E.partitioned()) return NBG_OK;
  return E.fail(NBG_E_UNSUPPORTED, label + " on a partitioned engine (its rows live on several ranks)");
}

int32_t copy_input_names(Engine& E, const std::string& label, const char* const* given, int nc,
                         std::vector<std::string>* names) {
  for (int c = 0; c < nc; ++c) {
    if (!given[c]) return E.fail(NBG_E_INVALID_ARGUMENT, label + ": null input column name");
    names->emplace_back(given[c]);
  }
  return NBG_OK;
}

// the device side of a result: its workspace and its non-empty segments, on the engine's device
struct DeviceInput {
  Workspace* w = nullptr;
  Segs segs;
  std::vector<int> types;   // each segment's OVER position (nbg_rows::Seg::type)
};
int32_t device_input(Engine& E, const std::string& label, const nbg_rows* in, DeviceInput* d) {
  if (hipSetDevice(E.cfg.device) != hipSuccess) return E.fail(NBG_E_DEVICE, "hipSetDevice failed");
  auto* m = const_cast<nbg_rows*>(in);
  m->build_segs();
  for (auto& sg : m->segs)
    if (sg.end > sg.begin) {
      d->segs.emplace_back(sg.begin, sg.end - sg.begin);
      d->types.push_back(sg.type);
    }
  d->w = in->owned_ws ? in->owned_ws : in->ws;
  return d->w ? NBG_OK : E.fail(NBG_E_INVALID_ARGUMENT, label + ": the rows have no device workspace");
}

// a driver's output becomes the result: one segment of `n` rows in `w` (the stages' result form)
void adopt_rows(nbg_rows* r, Workspace* w, uint64_t n, int ncols) {
  r->ws = r->owned_ws = w;
  r->count = n;
  nbg_rows::TypeBlocks tb;
  tb.region = 0;
  tb.blk_cap = n;
  tb.counts.assign(1, (uint32_t)n);
  r->blocks.push_back(std::move(tb));
  for (int c = 0; c < ncols; ++c) r->dcols.push_back(ws_row_col(w, c));
}

// What a stage knows about its input's columns, computed once per call.  What follows from it
// (which case is an error, and its text) is each stage's own.
struct InputCols {
  std::vector<uint8_t> mixed;      // the OVER types give the column different kinds (its kind reads VK_INT)
  std::vector<VKind> kind;
  std::vector<int32_t> type;       // NBG_T_*: the result schema's if it names one, else the kind's natural type
  std::vector<std::string> spell;  // what spells the column's string constant outside the dictionary
  std::vector<uint8_t> respelt;    // ... differs between OVER types
  std::vector<uint8_t> spelt;      // ... is not empty for some OVER type
  std::vector<uint8_t> outside;    // the column can hold strings outside the dictionary: spelt, or derived strings
  bool any_mixed = false, any_respelt = false;
  explicit InputCols(const nbg_rows* in)
      : mixed(in->ncols, 0), kind(in->ncols, VK_INT), type(in->ncols, NBG_T_INT), spell(in->ncols), respelt(in->ncols, 0),
        spelt(in->ncols, 0), outside(in->ncols, 0) {
    for (int c = 0; c < in->ncols; ++c) {
      const int k = in->col_kind(c);
      mixed[c] = k < 0;
      kind[c] = k < 0 ? VK_INT : (VKind)k;
      type[c] = c < (int)in->col_types.size() && in->col_types[c] ? in->col_types[c] : natural_type_of(kind[c]);
      bool have = false;
      for (auto& cs : in->const_str) {
        if ((int)cs.size() <= c) continue;
        respelt[c] = respelt[c] || (have && spell[c] != cs[c]);
        spelt[c] = spelt[c] || !cs[c].empty();
        spell[c] = cs[c];
        have = true;
      }
      outside[c] = spelt[c] || !in->derived.empty();
      any_mixed = any_mixed || mixed[c];
      any_respelt = any_respelt || respelt[c];
    }
  }
};

// the environment a stage compiles expressions in; `rows`: a program run per input row (CompileEnv::rows)
CompileEnv stage_env(Engine& E, bool rows) {
  static const std::vector<int32_t> no_over;
  CompileEnv cenv{};
  cenv.etype = 0;
  cenv.over = &no_over;
  cenv.edges = &E.edges;
  cenv.strings = &E.snap.strings;
  cenv.tags = &E.tags;
  if (!rows) return cenv;
  cenv.max_dict_len = E.refresh_max_dict_len();
  cenv.rows = true;
  return cenv;
}

// one YIELD column that is not passed through as it is: its register or constant in the plan, its
// kind, type (Collector::getSchema: the value's own, or a root cast's) and constant spelling in `res`
int32_t compile_yield_column(Engine& E, const std::string& label, const Node& n, const CompileEnv& cenv,
                             const ColTypeEnv& tenv, ProgramBuilder& pb, int y, YrPlan* plan, nbg_rows* res) {
  Compiled c;
  std::string err;
  if (int32_t rc = compile_expr(n, cenv, pb, &c, &err, true)) return E.fail(rc, label + ": " + err);
  plan->yield_reg[y] = c.is_const ? -1 : c.reg;
  plan->yield_const[y] = c.is_const ? c.const_bits : 0;
  res->kinds[0][y] = c.kind;
  res->col_types[y] = n.kind == EK_CAST ? yield_column_type(n, tenv) : natural_type_of(c.kind);
  if (!res->col_types[y]) res->col_types[y] = natural_type_of(c.kind);
  if (c.is_const && c.kind == VK_STRING && (c.const_bits & 1)) res->const_str[0][y] = c.const_str;
  return NBG_OK;
}

// the compiled program into the plan, if the device can run it
int32_t finish_program(Engine& E, const std::string& label, const ProgramBuilder& pb, YrPlan* plan) {
  plan->code = pb.code;
  plan->data = pb.data;
  plan->nregs = std::max(1, pb.max_reg);
  for (const Ins& i : plan->code)
    if (i.op == OP_SOUT || i.op == OP_SMAT) return E.fail(NBG_E_UNSUPPORTED, label + ": an expression that builds a string");
  if ((int)(plan->code.size() + plan->data.size()) > MAX_PROGRAM) return E.fail(NBG_E_UNSUPPORTED, label + ": program too long");
  if (plan->nregs > interp_max_regs())
    return E.fail(NBG_E_UNSUPPORTED, label + ": expression too deep for the device register file (" + std::to_string(plan->nregs) +
                                         " registers, " + std::to_string(interp_max_regs()) + " fit the LDS)");
  return NBG_OK;
}

}  // namespace

// ============================================================================= GROUP BY
// GroupByExecutor (src/graph/GroupByExecutor.cpp:44-178 the checks, :226-322 the grouping,
// :355-391 the result schema) over a device-resident result; the kernels are in groupby.hip.
namespace {

bool gb_only_constants(const Node& n) {   // no prop, input or variable reference anywhere
  switch (n.kind) {
    case EK_PRIMARY: case EK_FUNC: case EK_UNARY: case EK_CAST: case EK_ARITH: case EK_REL: case EK_LOGIC: break;
    default: return false;
  }
  for (auto& k : n.kids)
    if (!k || !gb_only_constants(*k)) return false;
  return true;
}

bool gb_is_agg_name(std::string f) {
  for (char& ch : f) ch = (char)toupper((unsigned char)ch);
  for (const char* a : {"COUNT", "COUNT_DISTINCT", "SUM", "AVG", "MAX", "MIN", "STD", "BIT_AND", "BIT_OR", "BIT_XOR"})
    if (f == a) return true;
  return false;
}

// PrimaryExpression::toString of a constant (what a bare name in GROUP BY is compared to)
std::string gb_primary_string(const Node& n) {
  if (n.kind != EK_PRIMARY) return std::string("\x01");   // (never an alias)
  switch (n.prim.index()) {
    case 0: return std::to_string(std::get<0>(n.prim));
    case 1: return std::to_string(std::get<1>(n.prim));
    case 2: return std::get<2>(n.prim) ? "true" : "false";
    default: return std::get<3>(n.prim);
  }
}

struct GbValue {          // a YIELD operand: an input column or a constant
  int col = -1;
  VKind kind = VK_INT;
  int32_t type = NBG_T_INT;
  int64_t bits = 0;       // constant payload (strings: the dictionary code)
  std::string text;       // constant string
};

}  // namespace

extern "C" {

int32_t nbg_group_by(nbg_engine* h, const nbg_rows* in, const nbg_group_request* rq, nbg_rows** out) {
  if (!h || !in || !rq || !out) return NBG_E_INVALID_ARGUMENT;
  *out = nullptr;
  Engine& E = h->e;
  std::lock_guard<std::mutex> lg(E.mu);
  if (int32_t rc = guard_rows(E, "GROUP BY", {in})) return rc;
  if (int32_t rc = guard_partitioned(E, "GROUP BY")) return rc;
  const int ng = rq->num_groups, ny = rq->num_yields;
  if (!in->count) {   // GroupByExecutor::execute returns before checkAll: no check, no rows
    *out = new_rows(E, std::max(0, std::min(ny, (int)MAX_YIELDS)));
    return NBG_OK;
  }
  if ((ng > 0 && (!rq->group_exprs || !rq->group_lens)) ||
      (ny > 0 && (!rq->yield_exprs || !rq->yield_lens || !rq->yield_funs)) || !rq->input_names)
    return E.fail(NBG_E_INVALID_ARGUMENT, "GROUP BY: null argument");
  if (ng > MAX_YIELDS || ny > MAX_YIELDS)
    return E.fail(NBG_E_UNSUPPORTED, "GROUP BY: more than NBG_MAX_YIELDS group or yield columns");
  std::vector<std::string> names;
  if (int32_t rc = copy_input_names(E, "GROUP BY", rq->input_names, in->ncols, &names)) return rc;
  auto find_col = [&](const std::string& n) {
    auto it = std::find(names.begin(), names.end(), n);
    return it == names.end() ? -1 : (int)(it - names.begin());
  };
  auto decode = [&](const uint8_t* p, uint32_t n, std::unique_ptr<Node>* node) -> int32_t {
    std::string err;
    if (!p || !n) return E.fail(NBG_E_INVALID_ARGUMENT, "GROUP BY: an empty expression");
    *node = decode_expr(p, n, &err);
    return *node ? NBG_OK : E.fail(NBG_E_INVALID_ARGUMENT, "GROUP BY: " + err);
  };
  // ---- prepareYield / prepareGroup / checkAll
  if (ny <= 0) return E.fail(NBG_E_SYNTAX_ERROR, "Yield cols is empty");
  std::vector<std::unique_ptr<Node>> ynodes(ny), gnodes(std::max(ng, 0));
  std::map<std::string, int> aliases;   // alias -> the first `$-.x AS alias` yield
  for (int y = 0; y < ny; ++y) {
    if (int32_t rc = decode(rq->yield_exprs[y], rq->yield_lens[y], &ynodes[y])) return rc;
    const int32_t f = rq->yield_funs[y];
    if (f < NBG_AGG_NONE || f > NBG_AGG_BIT_XOR) return E.fail(NBG_E_INVALID_ARGUMENT, "GROUP BY: unknown function");
    const Node& n = *ynodes[y];
    const bool star = n.kind == EK_PRIMARY && n.prim.index() == 3 && std::get<3>(n.prim) == "*";
    if (star && f != NBG_AGG_COUNT && f != NBG_AGG_COUNT_DISTINCT) return E.fail(NBG_E_SYNTAX_ERROR, "Syntax error: near `*'");
    const char* al = rq->yield_aliases ? rq->yield_aliases[y] : nullptr;
    if (al && n.kind == EK_INPUT) aliases.emplace(al, y);
  }
  if (ng <= 0) return E.fail(NBG_E_SYNTAX_ERROR, "Group cols is empty");
  std::set<int> key_set;          // the `$-` group keys (input columns)
  std::vector<int> key_cols;
  for (int g = 0; g < ng; ++g) {
    if (int32_t rc = decode(rq->group_exprs[g], rq->group_lens[g], &gnodes[g])) return rc;
    const Node& n = *gnodes[g];
    if (n.kind == EK_FUNC && gb_is_agg_name(n.alias))
      return E.fail(NBG_E_SYNTAX_ERROR, "Use invalid group function `" + n.alias + "'");
  }
  for (int g = 0; g < ng; ++g) {
    const Node& n = *gnodes[g];
    if (n.kind == EK_INPUT) {
      const int c = find_col(n.prop);
      if (c < 0) return E.fail(NBG_E_SYNTAX_ERROR, "Group `" + n.prop + "' isn't in output fields");
      if (key_set.insert(c).second) key_cols.push_back(c);
      continue;
    }
    if (n.kind == EK_FUNC) continue;   // (constant-folded below)
    const std::string gname = gb_primary_string(n);
    auto a = aliases.find(gname);
    if (a == aliases.end()) return E.fail(NBG_E_SYNTAX_ERROR, "Group `" + gname + "' isn't in output fields");
    const int c = find_col(ynodes[a->second]->prop);   // (absent: the yield check below answers)
    if (c >= 0 && key_set.insert(c).second) key_cols.push_back(c);
  }
  for (int y = 0; y < ny; ++y) {
    const Node& n = *ynodes[y];
    if (n.kind == EK_INPUT) {
      const int c = find_col(n.prop);
      if (c < 0) return E.fail(NBG_E_SYNTAX_ERROR, "Yield `" + n.prop + "' isn't in output fields");
      if (rq->yield_funs[y] == NBG_AGG_NONE && !key_set.count(c))
        return E.fail(NBG_E_SYNTAX_ERROR, "Yield `" + n.prop + "' isn't in group fields");
    } else if (n.kind == EK_VAR) {
      return E.fail(NBG_E_SYNTAX_ERROR, "Can't support variableExpression");
    }
  }
  // ---- device scope
  if (in->misaligned || in->float_col)
    return E.fail(NBG_E_UNSUPPORTED, "GROUP BY: the input's row schema re-reads its columns (misaligned or FLOAT)");
  const CompileEnv cenv = stage_env(E, false);
  const InputCols cols(in);
  auto constant = [&](const Node& n, GbValue* v) -> int32_t {
    if (!gb_only_constants(n)) return E.fail(NBG_E_UNSUPPORTED, "GROUP BY: an expression that is neither `$-.col' nor constant");
    ProgramBuilder pb;
    Compiled c;
    std::string err;
    const int32_t rc = compile_expr(n, cenv, pb, &c, &err, true);
    if (rc) return E.fail(rc, "GROUP BY: " + err);
    if (c.always_error) return E.fail(NBG_E_EXECUTION_ERROR, "GROUP BY: a constant expression fails to evaluate");
    if (!c.is_const || c.derived) return E.fail(NBG_E_UNSUPPORTED, "GROUP BY: an expression that is not constant");
    v->col = -1;
    v->kind = c.kind;
    v->type = natural_type_of(c.kind);
    v->bits = c.const_bits;
    v->text = c.const_str;
    return NBG_OK;
  };
  auto column = [&](int c, GbValue* v) -> int32_t {
    if (cols.mixed[c]) return E.fail(NBG_E_UNSUPPORTED, "GROUP BY: column `" + names[c] + "' mixes value kinds");
    v->col = c;
    v->kind = cols.kind[c];
    v->type = cols.type[c];
    return NBG_OK;
  };
  for (int g = 0; g < ng; ++g) {   // a function-call key must fold: it adds nothing to the identity
    if (gnodes[g]->kind != EK_FUNC) continue;
    GbValue v;
    if (int32_t rc = constant(*gnodes[g], &v)) return rc;
  }
  GbPlan plan;
  plan.nkeys = (int)key_cols.size();
  for (int k = 0; k < plan.nkeys; ++k) {
    GbValue v;
    if (int32_t rc = column(key_cols[k], &v)) return rc;
    plan.key_col[k] = (int8_t)key_cols[k];
    plan.key_dbl[k] = v.kind == VK_DOUBLE;
  }
  plan.acc[0] = GbAcc{GB_COUNT, 0, -1, 0, 0};
  plan.nacc = 1;
  plan.nout = ny;
  std::unique_ptr<nbg_rows> res(new_rows(E, ny));
  auto slot = [&](GbOp op, const GbValue& v, int ref) {
    plan.acc[plan.nacc] = GbAcc{(uint8_t)op, (uint8_t)(v.kind == VK_DOUBLE), (int8_t)v.col, (uint8_t)ref, v.bits};
    return plan.nacc++;
  };
  for (int y = 0; y < ny; ++y) {
    GbValue v;
    const Node& n = *ynodes[y];
    if (n.kind == EK_INPUT) {
      if (int32_t rc = column(find_col(n.prop), &v)) return rc;
    } else if (int32_t rc = constant(n, &v)) {
      return rc;
    }
    GbOut& o = plan.out[y];
    VKind okind = VK_INT;
    int32_t otype = NBG_T_INT;
    auto emit_const = [&](VKind k, int32_t t, int64_t bits) {
      o = GbOut{GE_CONST, -1, 0, bits};
      okind = k;
      otype = t;
    };
    const bool int_like = v.type == NBG_T_INT || v.type == NBG_T_VID || v.type == NBG_T_TIMESTAMP;
    const bool is_dbl = v.type == NBG_T_DOUBLE;
    const double zero = 0.0;
    int64_t zero_bits;
    memcpy(&zero_bits, &zero, 8);
    switch (rq->yield_funs[y]) {
      case NBG_AGG_NONE:   // Group::apply keeps the row's value: a key cell or the constant
        if (v.col >= 0) {
          o = GbOut{GE_KEY, (int8_t)v.col, 0, 0};
          okind = v.kind;
          otype = v.type;
          if (v.kind == VK_STRING) {   // a string column the result carries over: what spells its codes outside the dictionary
            if (cols.respelt[v.col])
              return E.fail(NBG_E_UNSUPPORTED, "GROUP BY: column `" + names[v.col] + "' spells different constants per OVER type");
            res->const_str[0][y] = cols.spell[v.col];
          }
        } else {
          emit_const(v.kind, v.type, v.bits);
          res->const_str[0][y] = v.text;
        }
        break;
      case NBG_AGG_COUNT:
        o = GbOut{GE_SLOT, -1, 0, 0};
        break;
      case NBG_AGG_COUNT_DISTINCT:
        if (v.col < 0) emit_const(VK_INT, NBG_T_INT, 1);
        else o = GbOut{GE_SLOT, -1, (uint8_t)slot(GB_DISTINCT, v, 0), 0};
        break;
      case NBG_AGG_SUM:
        if (int_like) {
          o = GbOut{GE_SLOT, -1, (uint8_t)slot(GB_SUM_I, v, 0), 0};
          otype = v.type;
        } else if (is_dbl) {
          o = GbOut{GE_SLOT, -1, (uint8_t)slot(GB_SUM_D, v, 0), 0};
          okind = VK_DOUBLE;
          otype = NBG_T_DOUBLE;
        } else {
          emit_const(VK_INT, NBG_T_INT, 0);
        }
        break;
      case NBG_AGG_AVG:
        okind = VK_DOUBLE;
        otype = NBG_T_DOUBLE;
        if (v.type == NBG_T_VID || v.type == NBG_T_TIMESTAMP)
          return E.fail(NBG_E_UNSUPPORTED, "GROUP BY: AVG over a VID or TIMESTAMP column");
        if (int_like) o = GbOut{GE_AVG_I, -1, (uint8_t)slot(GB_SUM_I, v, 0), 0};
        else if (is_dbl) o = GbOut{GE_AVG_D, -1, (uint8_t)slot(GB_SUM_D, v, 0), 0};
        else emit_const(VK_DOUBLE, NBG_T_DOUBLE, zero_bits);
        break;
      case NBG_AGG_MAX: case NBG_AGG_MIN: {
        okind = v.kind;
        otype = v.type;
        if (v.col < 0) {
          emit_const(v.kind, v.type, v.bits);
          res->const_str[0][y] = v.text;
          break;
        }
        if (v.kind == VK_STRING && cols.outside[v.col])
          return E.fail(NBG_E_UNSUPPORTED, "GROUP BY: MAX/MIN over a string column that can hold strings outside the dictionary");
        const GbOp op = rq->yield_funs[y] == NBG_AGG_MAX ? GB_MAX : GB_MIN;
        o = GbOut{(uint8_t)(v.kind == VK_DOUBLE ? GE_ORD_D : GE_ORD_I), -1, (uint8_t)slot(op, v, 0), 0};
        break;
      }
      case NBG_AGG_STD:
        if (v.type == NBG_T_INT || is_dbl) {
          const int s = slot(is_dbl ? GB_SUM_D : GB_SUM_I, v, 0);
          o = GbOut{GE_STD, -1, (uint8_t)slot(GB_SQ, v, s), 0};
          okind = VK_DOUBLE;
          otype = NBG_T_DOUBLE;
        } else {
          emit_const(VK_INT, NBG_T_INT, 0);
        }
        break;
      default: {   // BIT_AND / BIT_OR / BIT_XOR: INT values only
        if (v.type != NBG_T_INT) { emit_const(VK_INT, NBG_T_INT, 0); break; }
        const GbOp op = rq->yield_funs[y] == NBG_AGG_BIT_AND ? GB_AND : rq->yield_funs[y] == NBG_AGG_BIT_OR ? GB_OR : GB_XOR;
        o = GbOut{GE_SLOT, -1, (uint8_t)slot(op, v, 0), 0};
      }
    }
    res->kinds[0][y] = okind;
    res->col_types[y] = otype;
  }
  // ---- the passes
  DeviceInput d;
  if (int32_t rc = device_input(E, "GROUP BY", in, &d)) return rc;
  Workspace* ow = nullptr;
  uint64_t G = 0;
  std::string err;
  if (int32_t rc = ws_group_by(d.w, E.stream, d.segs, plan, &ow, &G, &err)) return E.fail(rc, err);
  res->derived = in->derived;
  adopt_rows(res.get(), ow, G, ny);
  *out = res.release();
  return NBG_OK;
}

// ============================================================================= ORDER BY / LIMIT
// OrderByExecutor (src/graph/OrderByExecutor.cpp:94-155) and LimitExecutor
// (src/graph/LimitExecutor.cpp:18-66) over a device-resident result; the kernels are in orderby.hip.
// (under the engine lock; nbg_set_op's pass-through shortcuts are this with no factors and no LIMIT)
static int32_t order_by_locked(Engine& E, const nbg_rows* in, const nbg_order_request* rq, nbg_rows** out) {
  // LimitExecutor::prepare (:18-28): before anything is executed, whatever the input holds
  if (rq->has_limit && rq->offset < 0)
    return E.fail(NBG_E_SYNTAX_ERROR, "skip `" + std::to_string(rq->offset) + "' is illegal");
  if (rq->has_limit && rq->count < 0)
    return E.fail(NBG_E_SYNTAX_ERROR, "count `" + std::to_string(rq->count) + "' is illegal");
  if (int32_t rc = guard_rows(E, "ORDER BY", {in})) return rc;
  if (int32_t rc = guard_partitioned(E, "ORDER BY")) return rc;
  const int nf = rq->num_factors, nc = in->ncols;
  if (nf < 0) return E.fail(NBG_E_INVALID_ARGUMENT, "ORDER BY: negative factor count");
  // the result carries the input's columns: one kind and one spelling of constants per column
  std::unique_ptr<nbg_rows> res(new_rows(E, nc));
  res->derived = in->derived;
  const InputCols cols(in);
  res->kinds[0] = cols.kind;
  res->col_types = cols.type;
  res->const_str[0] = cols.spell;
  if (!in->count) {   // OrderByExecutor::beforeExecute (:137-139) and LimitExecutor: no rows, no check
    *out = res.release();
    return NBG_OK;
  }
  if (!rq->input_names || (nf > 0 && (!rq->factor_names || !rq->factor_desc)))
    return E.fail(NBG_E_INVALID_ARGUMENT, "ORDER BY: null argument");
  if (nf > MAX_YIELDS) return E.fail(NBG_E_UNSUPPORTED, "ORDER BY: more than NBG_MAX_YIELDS factors");
  if (nc < 1 || nc > MAX_YIELDS) return E.fail(NBG_E_INVALID_ARGUMENT, "ORDER BY: the rows have no columns");
  std::vector<std::string> names;
  if (int32_t rc = copy_input_names(E, "ORDER BY", rq->input_names, nc, &names)) return rc;
  ObPlan plan;
  plan.nf = nf;
  plan.ncols = nc;
  for (int f = 0; f < nf; ++f) {   // getFieldIndex: the first column of that name (:140-152)
    if (!rq->factor_names[f]) return E.fail(NBG_E_INVALID_ARGUMENT, "ORDER BY: null factor name");
    auto it = std::find(names.begin(), names.end(), std::string(rq->factor_names[f]));
    if (it == names.end())
      return E.fail(NBG_E_EXECUTION_ERROR, std::string("Field (") + rq->factor_names[f] + ") not exist in input schema.");
    plan.col[f] = (int8_t)(it - names.begin());
    plan.desc[f] = rq->factor_desc[f] != 0;
  }
  // ---- device scope
  if (in->misaligned || in->float_col)
    return E.fail(NBG_E_UNSUPPORTED, "ORDER BY: the input's row schema re-reads its columns (misaligned or FLOAT)");
  if (cols.any_mixed) return E.fail(NBG_E_UNSUPPORTED, "ORDER BY: a column mixes value kinds between OVER types");
  if (cols.any_respelt) return E.fail(NBG_E_UNSUPPORTED, "ORDER BY: a string column spells different constants per OVER type");
  for (int f = 0; f < nf; ++f) {
    const int c = plan.col[f];
    plan.dbl[f] = cols.kind[c] == VK_DOUBLE;
    // dictionary codes order as their strings do (loader.cpp: the dictionary is sorted by
    // std::string::operator<); a derived code or an out-of-dictionary constant does not
    if (cols.kind[c] == VK_STRING && cols.outside[c])
      return E.fail(NBG_E_UNSUPPORTED, "ORDER BY: factor `" + names[c] + "' can hold strings outside the dictionary");
  }
  // ---- the window (LimitExecutor.cpp:30-66)
  const uint64_t total = in->count;
  plan.has_limit = rq->has_limit != 0;
  plan.lo = 0;
  plan.hi = total;
  if (plan.has_limit) {
    const uint64_t off = (uint64_t)rq->offset, cnt = (uint64_t)rq->count;
    if (cnt == 0 || total <= off) {
      *out = res.release();
      return NBG_OK;
    }
    plan.lo = off;
    plan.hi = cnt > total - off ? total : off + cnt;   // (off + cnt saturates)
  }
  if (plan.hi - plan.lo > 0xFFFFFFFFull)   // (a result segment's row count is 32 bits)
    return E.fail(NBG_E_UNSUPPORTED, "ORDER BY: a result of 2^32 rows or more");
  // ---- the passes
  DeviceInput d;
  if (int32_t rc = device_input(E, "ORDER BY", in, &d)) return rc;
  Workspace* ow = nullptr;
  std::string err;
  if (int32_t rc = ws_order_by(d.w, E.stream, d.segs, plan, &ow, &E.ob_prof, &err)) return E.fail(rc, err);
  adopt_rows(res.get(), ow, plan.hi - plan.lo, nc);
  *out = res.release();
  return NBG_OK;
}

int32_t nbg_order_by(nbg_engine* h, const nbg_rows* in, const nbg_order_request* rq, nbg_rows** out) {
  if (!h || !in || !rq || !out) return NBG_E_INVALID_ARGUMENT;
  *out = nullptr;
  Engine& E = h->e;
  std::lock_guard<std::mutex> lg(E.mu);
  return order_by_locked(E, in, rq, out);
}

// ============================================================================= UNION / INTERSECT / MINUS
// SetExecutor (src/graph/SetExecutor.cpp:98-383) over two device-resident results; the kernels
// are in setops.hip.
int32_t nbg_set_op(nbg_engine* h, const nbg_rows* left, const nbg_rows* right, const nbg_set_request* rq,
                   nbg_rows** out) {
  if (!h || !left || !right || !rq || !out) return NBG_E_INVALID_ARGUMENT;
  *out = nullptr;
  Engine& E = h->e;
  std::lock_guard<std::mutex> lg(E.mu);
  if (rq->op < NBG_SET_UNION || rq->op > NBG_SET_MINUS) return E.fail(NBG_E_INVALID_ARGUMENT, "set operation: unknown operator");
  if (int32_t rc = guard_rows(E, "set operation", {left, right})) return rc;
  if (int32_t rc = guard_partitioned(E, "set operation")) return rc;
  const int nc = left->ncols;
  if (nc != right->ncols) return E.fail(NBG_E_EXECUTION_ERROR, "Field count not match.");
  // ---- the empty-input shortcuts (SetExecutor.cpp:137-141, :163-174, :273-277, :327-337): before
  // any schema check; a side passed on is what ORDER BY without factors and LIMIT makes of it
  const bool uni = rq->op == NBG_SET_UNION;
  auto as_it_is = [&](const nbg_rows* side) {
    std::vector<const char*> names((size_t)std::max(side->ncols, 1), "");
    nbg_order_request pass{};
    pass.input_names = names.data();
    return order_by_locked(E, side, &pass, out);
  };
  if (!left->count || !right->count) {
    if (uni && right->count) return as_it_is(right);
    if ((uni || rq->op == NBG_SET_MINUS) && left->count) return as_it_is(left);
    *out = new_rows(E, nc);   // (both empty, INTERSECT with an empty side, MINUS from nothing)
    return NBG_OK;
  }
  // ---- device scope, and the casts (checkSchema / doCasting, :219-262)
  if (left->misaligned || left->float_col || right->misaligned || right->float_col)
    return E.fail(NBG_E_UNSUPPORTED, "set operation: an input's row schema re-reads its columns (misaligned or FLOAT)");
  if (nc < 1 || nc > MAX_YIELDS) return E.fail(NBG_E_INVALID_ARGUMENT, "set operation: the rows have no columns");
  std::unique_ptr<nbg_rows> res(new_rows(E, nc));
  SoPlan plan;
  plan.op = rq->op;
  plan.distinct = uni && rq->distinct;
  plan.ncols = nc;
  const InputCols lcols(left), rcols(right);
  auto int_like = [](int32_t t) { return t == NBG_T_INT || t == NBG_T_VID || t == NBG_T_TIMESTAMP; };
  for (int c = 0; c < nc; ++c) {
    if (lcols.mixed[c] || rcols.mixed[c])
      return E.fail(NBG_E_UNSUPPORTED, "set operation: a column mixes value kinds between OVER types");
    const int32_t lt = lcols.type[c], rt = rcols.type[c];
    if ((lt == NBG_T_STRING) != (rt == NBG_T_STRING))
      return E.fail(NBG_E_UNSUPPORTED, "set operation: column " + std::to_string(c) + " casts to or from STRING");
    // a constant outside the dictionary has a code private to its result: nothing to compare it by
    if (lt == NBG_T_STRING && (lcols.spelt[c] || rcols.spelt[c]))
      return E.fail(NBG_E_UNSUPPORTED, "set operation: string column " + std::to_string(c) +
                                           " carries a constant outside the dictionary");
    res->kinds[0][c] = lcols.kind[c];
    res->col_types[c] = lt;
    plan.dbl[c] = lt == NBG_T_DOUBLE;
    uint8_t cast = SO_KEEP;
    if (lt != rt) {
      if (int_like(lt)) cast = rt == NBG_T_DOUBLE ? SO_D2I : rt == NBG_T_BOOL ? SO_B2I : SO_KEEP;
      else if (lt == NBG_T_DOUBLE) cast = rt == NBG_T_BOOL ? SO_B2D : SO_I2D;
      else if (lt == NBG_T_BOOL) cast = rt == NBG_T_DOUBLE ? SO_D2B : SO_I2B;
    }
    plan.cast[c] = cast;
  }
  // the derived strings of both inputs (their codes are content hashes, the same in every result)
  res->derived = left->derived;
  for (auto& kv : right->derived) {
    auto ins = res->derived.emplace(kv.first, kv.second);
    if (!ins.second && ins.first->second != kv.second) return E.fail(NBG_E_EXECUTION_ERROR, "derived-string hash collision");
  }
  // ---- the passes
  DeviceInput l, r;
  if (int32_t rc = device_input(E, "set operation", left, &l)) return rc;
  if (int32_t rc = device_input(E, "set operation", right, &r)) return rc;
  Workspace* ow = nullptr;
  uint64_t n = 0;
  std::string err;
  if (int32_t rc = ws_set_op(l.w, r.w, E.stream, l.segs, r.segs, plan, &ow, &n, &E.so_prof, &err)) return E.fail(rc, err);
  if (ow) adopt_rows(res.get(), ow, n, nc);
  *out = res.release();
  return NBG_OK;
}

// ============================================================================= YIELD ... WHERE
// YieldExecutor::executeInputs (src/graph/YieldExecutor.cpp:178-282) over a device-resident result;
// the kernels are in yieldrows.hip and, beside the interpreter, kernels.hip.
namespace {

// what a WHERE / YIELD tree references (ExpressionContext's has*Prop and variables())
struct YrRefs {
  bool graph = false;                    // $^, $$ or an edge property
  bool input = false;
  std::set<std::string> vars;
  std::vector<std::string> props;        // $- / $var column names, in evaluation order
};
void yr_refs(const Node& n, YrRefs* r) {
  switch (n.kind) {
    case EK_SRCPROP: case EK_DSTPROP: case EK_ALIAS: case EK_RANK: case EK_DST: case EK_SRCID: case EK_TYPE:
      r->graph = true;
      break;
    case EK_INPUT:
      r->input = true;
      r->props.push_back(n.prop);
      break;
    case EK_VAR:
      r->vars.insert(n.alias);
      r->props.push_back(n.prop);
      break;
    default: break;
  }
  for (auto& k : n.kids)
    if (k) yr_refs(*k, r);
}

// Statuses 1 to 6, which nbg_yield and nbg_yield_agg check alike (`agg_call': the latter, whose
// request must name a function)
struct YieldFront {
  std::vector<std::string> names;
  std::unique_ptr<Node> where;
  std::vector<std::unique_ptr<Node>> yields;   // after `$-.*' / `$var.*' expansion
  std::vector<int32_t> funs;
  YrRefs refs;
  bool agg = false;    // some function
  bool done = false;   // status 5: *out holds the zero-row result
  int find_col(const std::string& n) const {   // getFieldIndex: the first column of that name
    auto it = std::find(names.begin(), names.end(), n);
    return it == names.end() ? -1 : (int)(it - names.begin());
  }
};

int32_t yield_front(Engine& E, const nbg_rows* in, const nbg_yield_request* rq, bool agg_call, YieldFront* F,
                    nbg_rows** out) {
  // ---- 1. arguments
  if (rq->num_yields < 1) return E.fail(NBG_E_INVALID_ARGUMENT, "YIELD: no YIELD column");
  if (!rq->input_names || !rq->yield_exprs || !rq->yield_lens) return E.fail(NBG_E_INVALID_ARGUMENT, "YIELD: null argument");
  if (agg_call && !rq->yield_funs) return E.fail(NBG_E_INVALID_ARGUMENT, "YIELD: null argument");
  if (int32_t rc = guard_rows(E, "YIELD", {in})) return rc;
  const int nc = in->ncols;
  std::vector<std::string>& names = F->names;
  if (int32_t rc = copy_input_names(E, "YIELD", rq->input_names, nc, &names)) return rc;
  std::string err;
  if (rq->where && rq->where_len) {
    F->where = decode_expr(rq->where, rq->where_len, &err);
    if (!F->where) return E.fail(NBG_E_INVALID_ARGUMENT, "YIELD: WHERE: " + err);
  }
  std::vector<std::unique_ptr<Node>> given;
  for (int y = 0; y < rq->num_yields; ++y) {
    if (!rq->yield_exprs[y] || !rq->yield_lens[y]) return E.fail(NBG_E_INVALID_ARGUMENT, "YIELD: an empty expression");
    given.push_back(decode_expr(rq->yield_exprs[y], rq->yield_lens[y], &err));
    if (!given.back()) return E.fail(NBG_E_INVALID_ARGUMENT, "YIELD: " + err);
    if (rq->yield_funs && (rq->yield_funs[y] < NBG_AGG_NONE || rq->yield_funs[y] > NBG_AGG_BIT_XOR))
      return E.fail(NBG_E_INVALID_ARGUMENT, "YIELD: unknown function");
    F->agg = F->agg || (rq->yield_funs && rq->yield_funs[y] != NBG_AGG_NONE);
  }
  if (agg_call && !F->agg) return E.fail(NBG_E_INVALID_ARGUMENT, "YIELD: no aggregate function (the request is nbg_yield's)");
  // ---- 2.
  if (int32_t rc = guard_partitioned(E, "YIELD")) return rc;
  // ---- `$-.*' / `$var.*' (YieldClauseWrapper::prepare): every input column, in order
  std::vector<std::unique_ptr<Node>>& yields = F->yields;
  std::vector<int32_t>& funs = F->funs;
  YrRefs& refs = F->refs;
  if (F->where) yr_refs(*F->where, &refs);
  for (int y = 0; y < rq->num_yields; ++y) {
    Node& n = *given[y];
    const int32_t f = rq->yield_funs ? rq->yield_funs[y] : NBG_AGG_NONE;
    if ((n.kind == EK_INPUT || n.kind == EK_VAR) && n.prop == "*") {
      if (n.kind == EK_INPUT) refs.input = true;
      else refs.vars.insert(n.alias);
      for (int c = 0; c < nc; ++c) {
        auto col = std::make_unique<Node>();
        col->kind = n.kind;
        col->alias = n.alias;
        col->prop = names[c];
        yields.push_back(std::move(col));
        funs.push_back(f);
      }
      continue;
    }
    yr_refs(n, &refs);
    yields.push_back(std::move(given[y]));
    funs.push_back(f);
  }
  const int ny = (int)yields.size();
  // ---- 3. checkAggFun (:33-58), syntaxCheck (:116-122)
  if (F->agg)
    for (int y = 0; y < ny; ++y)
      if ((yields[y]->kind == EK_INPUT || yields[y]->kind == EK_VAR) && funs[y] == NBG_AGG_NONE)
        return E.fail(NBG_E_SYNTAX_ERROR,
                      "Input columns without aggregation are not supported in YIELD statement without GROUP BY, near `" +
                          yields[y]->prop + "'");
  if (refs.graph) return E.fail(NBG_E_SYNTAX_ERROR, "Only support input and variable in yield sentence.");
  // ---- 4. (:124-135)
  if (refs.input && !refs.vars.empty()) return E.fail(NBG_E_EXECUTION_ERROR, "Not support both input and variable.");
  if (refs.vars.size() > 1) return E.fail(NBG_E_EXECUTION_ERROR, "Only one variable allowed to use.");
  // ---- 5. no rows: one column per YIELD
  if (!in->count) {
    *out = new_rows(E, std::min(ny, (int)MAX_YIELDS));
    F->done = true;
    return NBG_OK;
  }
  // ---- 6. getOutputSchema (:298-316): getFieldIndex, the first column of that name
  for (const std::string& p : refs.props)
    if (F->find_col(p) < 0)
      return E.fail(NBG_E_EXECUTION_ERROR,
                    "column `" + p + "' not exist in " + (refs.vars.empty() ? "input." : "variable."));
  return NBG_OK;
}

// The WHERE into the program: asBool of its value in plan->where_reg, or, when it folds to a
// constant, whether that is false (no code).  Its registers are dead once its value is read.
int32_t compile_where(Engine& E, const Node& where, const CompileEnv& cenv, ProgramBuilder& pb, YrPlan* plan,
                      bool* where_false) {
  Compiled c;
  std::string err;
  if (int32_t rc = compile_expr(where, cenv, pb, &c, &err)) return E.fail(rc, "YIELD: " + err);
  if (c.is_const) {
    bool tv;
    switch (c.kind) {   // Expression::asBool
      case VK_STRING: tv = c.const_str.empty(); break;
      case VK_DOUBLE: { double d; memcpy(&d, &c.const_bits, 8); tv = d != 0.0; break; }
      default: tv = c.const_bits != 0;
    }
    *where_false = !tv;
    pb.code.clear();
  } else {
    const int r = c.reg;
    if (c.kind == VK_INT) pb.code.push_back(Ins{OP_TRUTHY_I, (uint8_t)r, (uint8_t)r, 0, 0, 0});
    else if (c.kind == VK_DOUBLE) pb.code.push_back(Ins{OP_TRUTHY_F, (uint8_t)r, (uint8_t)r, 0, 0, 0});
    else if (c.kind == VK_STRING)
      pb.code.push_back(Ins{OP_TRUTHY_S, (uint8_t)r, (uint8_t)r, 0, 0, string_code(E.snap.strings, "")});
    plan->where_len = (int)pb.code.size();
    plan->where_reg = r;
  }
  pb.next_reg = 0;
  return NBG_OK;
}

}  // namespace

int32_t nbg_yield(nbg_engine* h, const nbg_rows* in, const nbg_yield_request* rq, nbg_rows** out) {
  if (!h || !in || !rq || !out) return NBG_E_INVALID_ARGUMENT;
  *out = nullptr;
  Engine& E = h->e;
  std::lock_guard<std::mutex> lg(E.mu);
  // ---- 1. to 6.
  YieldFront F;
  if (int32_t rc = yield_front(E, in, rq, false, &F, out)) return rc;
  if (F.done) return NBG_OK;
  const int nc = in->ncols, ny = (int)F.yields.size();
  const std::vector<std::string>& names = F.names;
  const std::unique_ptr<Node>& where = F.where;
  const std::vector<std::unique_ptr<Node>>& yields = F.yields;
  const bool agg = F.agg;
  auto find_col = [&](const std::string& n) { return F.find_col(n); };
  std::string err;
  // ---- 7. device scope
  if (agg) return E.fail(NBG_E_UNSUPPORTED, "YIELD: aggregate functions without GROUP BY");
  if (in->misaligned || in->float_col)
    return E.fail(NBG_E_UNSUPPORTED, "YIELD: the input's row schema re-reads its columns (misaligned or FLOAT)");
  if (ny > MAX_YIELDS) return E.fail(NBG_E_UNSUPPORTED, "YIELD: more than NBG_MAX_YIELDS columns");
  if (nc < 1 || nc > MAX_YIELDS) return E.fail(NBG_E_INVALID_ARGUMENT, "YIELD: the rows have no columns");
  if (in->count > 0xFFFFFFFFull) return E.fail(NBG_E_UNSUPPORTED, "YIELD: an input of 2^32 rows or more");
  const InputCols cols(in);
  const std::vector<VKind>& kinds = cols.kind;
  // a use: `bare' is a YIELD column that is exactly the input column
  auto check_use = [&](int c, bool bare) -> int32_t {
    if (cols.mixed[c]) return E.fail(NBG_E_UNSUPPORTED, "YIELD: column `" + names[c] + "' mixes value kinds");
    if (kinds[c] != VK_STRING) return NBG_OK;
    if (!bare && cols.outside[c])
      return E.fail(NBG_E_UNSUPPORTED, "YIELD: column `" + names[c] + "' can hold strings outside the dictionary");
    if (bare && cols.respelt[c])
      return E.fail(NBG_E_UNSUPPORTED, "YIELD: column `" + names[c] + "' spells different constants per OVER type");
    return NBG_OK;
  };
  {
    YrRefs wr;
    if (where) yr_refs(*where, &wr);
    for (const std::string& p : wr.props)
      if (int32_t rc = check_use(find_col(p), false)) return rc;
    for (int y = 0; y < ny; ++y) {
      const bool bare = yields[y]->kind == EK_INPUT || yields[y]->kind == EK_VAR;
      YrRefs yr;
      yr_refs(*yields[y], &yr);
      for (const std::string& p : yr.props)
        if (int32_t rc = check_use(find_col(p), bare)) return rc;
    }
  }
  // ---- compile: WHERE first, then the YIELDs, one program for every row
  CompileEnv cenv = stage_env(E, true);
  cenv.input_names = &names;
  cenv.input_kinds = &kinds;
  ProgramBuilder pb;
  YrPlan plan;
  plan.ncols = ny;
  bool where_false = false;
  if (where)
    if (int32_t rc = compile_where(E, *where, cenv, pb, &plan, &where_false)) return rc;
  std::unique_ptr<nbg_rows> res(new_rows(E, ny));
  res->derived = in->derived;
  ColTypeEnv tenv;
  tenv.input_names = &names;
  tenv.input_kinds = &kinds;
  std::set<int32_t> direct;   // input columns passed through without the interpreter
  for (int y = 0; y < ny; ++y) {
    if (yields[y]->kind == EK_INPUT || yields[y]->kind == EK_VAR) {   // a bare column: copied as it is
      const int col = find_col(yields[y]->prop);
      plan.yield_reg[y] = -2 - col;
      direct.insert(col);
      res->kinds[0][y] = kinds[col];
      res->col_types[y] = natural_type_of(kinds[col]);
      if (kinds[col] == VK_STRING) res->const_str[0][y] = cols.spell[col];
      continue;
    }
    if (int32_t rc = compile_yield_column(E, "YIELD", *yields[y], cenv, tenv, pb, y, &plan, res.get())) return rc;
  }
  if (int32_t rc = finish_program(E, "YIELD", pb, &plan)) return rc;
  if (where_false) {   // a constant-false WHERE: no row, no launch
    *out = res.release();
    return NBG_OK;
  }
  {
    std::set<int32_t> wc, yc = direct;
    for (int pc = 0; pc < (int)plan.code.size(); ++pc)
      if (plan.code[pc].op == OP_COL) (pc < plan.where_len ? wc : yc).insert(plan.code[pc].aux);
    plan.where_cols = (int)wc.size();
    plan.yield_cols = (int)yc.size();
  }
  // ---- 8. the passes
  DeviceInput d;
  if (int32_t rc = device_input(E, "YIELD", in, &d)) return rc;
  plan.str = E.dev_strings();
  plan.now_sec = (int64_t)time(nullptr);
  plan.rand_seed = query_rand_seed();
  Workspace* ow = nullptr;
  uint64_t n = 0;
  if (int32_t rc = ws_yield_rows(d.w, E.stream, d.segs, plan, &ow, &n, &E.yr_prof, &err)) return E.fail(rc, err);
  if (ow) adopt_rows(res.get(), ow, n, ny);
  *out = res.release();
  return NBG_OK;
}

// ============================================================================= YIELD with aggregates
// YieldExecutor::executeInputs with checkAggFun's functions and no GROUP BY
// (src/graph/YieldExecutor.cpp:33-58, :178-282; AggregateFunction.h) over a device-resident result;
// the kernels are in yieldagg.hip and, beside the interpreter, kernels.hip.
namespace {

struct YaValue {          // a function's argument: a register, an input column as it is, or a constant
  int src = -1;           // YaSlot::src
  int col = -1;           // the input column of a bare `$-.col'
  VKind kind = VK_INT;
  int32_t type = NBG_T_INT;   // Collector::getSchema: the kind's own type, or a root cast's
  int64_t bits = 0;
  std::string text;       // a constant string
  bool is_const = false;
  bool fails = false;     // a constant expression that fails to evaluate (OP_ERR on every row)
};

}  // namespace

int32_t nbg_yield_agg(nbg_engine* h, const nbg_rows* in, const nbg_yield_request* rq, nbg_rows** out) {
  if (!h || !in || !rq || !out) return NBG_E_INVALID_ARGUMENT;
  *out = nullptr;
  Engine& E = h->e;
  std::lock_guard<std::mutex> lg(E.mu);
  // ---- 1. to 6.
  YieldFront F;
  if (int32_t rc = yield_front(E, in, rq, true, &F, out)) return rc;
  if (F.done) return NBG_OK;
  const int nc = in->ncols, ny = (int)F.yields.size();
  const std::vector<std::string>& names = F.names;
  std::string err;
  // ---- 7. device scope
  if (in->misaligned || in->float_col)
    return E.fail(NBG_E_UNSUPPORTED, "YIELD: the input's row schema re-reads its columns (misaligned or FLOAT)");
  if (ny > MAX_YIELDS) return E.fail(NBG_E_UNSUPPORTED, "YIELD: more than NBG_MAX_YIELDS columns");
  if (nc < 1 || nc > MAX_YIELDS) return E.fail(NBG_E_INVALID_ARGUMENT, "YIELD: the rows have no columns");
  if (in->count > 0xFFFFFFFFull) return E.fail(NBG_E_UNSUPPORTED, "YIELD: an input of 2^32 rows or more");
  const InputCols cols(in);
  const std::vector<VKind>& kinds = cols.kind;
  auto bare = [](const Node& n) { return n.kind == EK_INPUT || n.kind == EK_VAR; };
  // a use: every function reads a bare column's cells as they are; what a string column may then
  // feed is each function's own check below
  auto check_use = [&](int c, bool is_bare) -> int32_t {
    if (cols.mixed[c]) return E.fail(NBG_E_UNSUPPORTED, "YIELD: column `" + names[c] + "' mixes value kinds");
    if (kinds[c] == VK_STRING && !is_bare && cols.outside[c])
      return E.fail(NBG_E_UNSUPPORTED, "YIELD: column `" + names[c] + "' can hold strings outside the dictionary");
    return NBG_OK;
  };
  {
    YrRefs wr;
    if (F.where) yr_refs(*F.where, &wr);
    for (const std::string& p : wr.props)
      if (int32_t rc = check_use(F.find_col(p), false)) return rc;
    for (int y = 0; y < ny; ++y) {
      YrRefs yr;
      yr_refs(*F.yields[y], &yr);
      for (const std::string& p : yr.props)
        if (int32_t rc = check_use(F.find_col(p), bare(*F.yields[y]))) return rc;
    }
  }
  // ---- compile: the WHERE, then one register per distinct argument expression
  CompileEnv cenv = stage_env(E, true);
  cenv.input_names = &names;
  cenv.input_kinds = &kinds;
  ColTypeEnv tenv;
  tenv.input_names = &names;
  tenv.input_kinds = &kinds;
  ProgramBuilder pb;
  YaPlan plan;
  plan.nout = ny;
  if (F.where)
    if (int32_t rc = compile_where(E, *F.where, cenv, pb, &plan.y, &plan.none)) return rc;
  // an argument's identity: its wire bytes (a column `$-.*' expanded to: the column)
  auto encode = [](const Node& n, auto&& self, std::string* k) -> void {
    k->push_back((char)n.kind);
    k->push_back((char)n.op);
    k->append(n.alias).push_back('\0');
    k->append(n.prop).push_back('\0');
    k->push_back((char)n.prim.index());
    switch (n.prim.index()) {
      case 0: k->append((const char*)&std::get<0>(n.prim), 8); break;
      case 1: k->append((const char*)&std::get<1>(n.prim), 8); break;
      case 2: k->push_back(std::get<2>(n.prim)); break;
      default: k->append(std::get<3>(n.prim)).push_back('\0');
    }
    k->push_back((char)n.kids.size());
    for (auto& kid : n.kids)
      if (kid) self(*kid, self, k);
  };
  std::map<std::string, YaValue> args;
  std::map<std::pair<std::string, int>, int> slots;   // (argument, YaOp) -> slot
  std::set<int32_t> direct;                            // input columns read without the interpreter
  auto argument = [&](const Node& n, std::string* key, YaValue* v) -> int32_t {
    if (bare(n)) *key = "\x01" + std::to_string(F.find_col(n.prop));
    else encode(n, encode, key);
    auto it = args.find(*key);
    if (it != args.end()) {
      *v = it->second;
      return NBG_OK;
    }
    if (bare(n)) {
      v->col = F.find_col(n.prop);
      v->src = -2 - v->col;
      v->kind = kinds[v->col];
      v->type = natural_type_of(v->kind);
    } else {
      Compiled c;
      if (int32_t rc = compile_expr(n, cenv, pb, &c, &err, true)) return E.fail(rc, "YIELD: " + err);
      v->is_const = c.is_const;
      v->fails = c.always_error;
      v->src = c.is_const ? -1 : c.reg;
      v->kind = c.kind;
      v->bits = c.is_const ? c.const_bits : 0;
      if (c.is_const && c.kind == VK_STRING) v->text = c.const_str;
      v->type = n.kind == EK_CAST ? yield_column_type(n, tenv) : 0;
      if (!v->type) v->type = natural_type_of(c.kind);
    }
    args.emplace(*key, *v);
    return NBG_OK;
  };
  auto slot = [&](const std::string& key, YaOp op, const YaValue& v, int ref) {
    auto ins = slots.emplace(std::make_pair(key, (int)op), plan.nslots);
    if (!ins.second) return ins.first->second;
    plan.slot[plan.nslots] = YaSlot{(uint8_t)op, (uint8_t)(v.kind == VK_DOUBLE), (uint8_t)ref, v.src, v.bits};
    if (v.col >= 0) direct.insert(v.col);
    return plan.nslots++;
  };
  std::unique_ptr<nbg_rows> res(new_rows(E, ny));
  res->derived = in->derived;
  std::vector<uint8_t> is_avg(ny, 0);
  bool needs_rows = false;   // a MAX, a MIN or a function-less column: status 9 when no row is kept
  const double zero = 0.0;
  int64_t zero_bits;
  memcpy(&zero_bits, &zero, 8);
  for (int y = 0; y < ny; ++y) {
    const Node& n = *F.yields[y];
    const int32_t fun = F.funs[y];
    std::string key;
    YaValue v;
    if (int32_t rc = argument(n, &key, &v)) return rc;
    YaOut& o = plan.out[y];
    VKind okind = VK_INT;
    int32_t otype = NBG_T_INT;
    auto emit_const = [&](VKind k, int32_t t, int64_t bits) {
      o = YaOut{YE_CONST, 0, bits};
      okind = k;
      otype = t;
    };
    // a string the functions compare by its code: a bare column inside the dictionary, or a constant
    auto string_by_code = [&](const char* what) -> int32_t {
      if (v.kind != VK_STRING || v.is_const) return NBG_OK;
      if (v.col < 0) return E.fail(NBG_E_UNSUPPORTED, std::string("YIELD: ") + what + " over a string expression");
      if (cols.outside[v.col])
        return E.fail(NBG_E_UNSUPPORTED, std::string("YIELD: ") + what + " over a string column that can hold strings outside the dictionary");
      return NBG_OK;
    };
    const bool int_like = v.type == NBG_T_INT || v.type == NBG_T_VID || v.type == NBG_T_TIMESTAMP;
    const bool is_dbl = v.type == NBG_T_DOUBLE;
    switch (fun) {
      case NBG_AGG_NONE:   // Group::apply keeps the last row's value: here a constant's
        if (v.fails) {
          emit_const(VK_INT, NBG_T_INT, 0);   // a constant that fails to evaluate: every kept row's error
        } else if (!v.is_const) {
          return E.fail(NBG_E_UNSUPPORTED, "YIELD: a column without a function that is not constant");
        } else {
          emit_const(v.kind, v.type, v.bits);
          if (v.kind == VK_STRING && (v.bits & 1)) res->const_str[0][y] = v.text;
        }
        needs_rows = true;
        break;
      case NBG_AGG_COUNT:
        o = YaOut{YE_COUNT, 0, 0};
        break;
      case NBG_AGG_COUNT_DISTINCT: {
        if (v.is_const) { emit_const(VK_INT, NBG_T_INT, 1); break; }
        if (int32_t rc = string_by_code("COUNT_DISTINCT")) return rc;
        emit_const(VK_INT, NBG_T_INT, 0);   // (the driver stores the count)
        YaDistinct d;
        d.out = y;
        d.dbl = v.kind == VK_DOUBLE;
        d.y.ncols = 1;
        ProgramBuilder dpb;
        bool unused = false;
        if (F.where && !plan.none)
          if (int32_t rc = compile_where(E, *F.where, cenv, dpb, &d.y, &unused)) return rc;
        if (v.col >= 0) {
          d.y.yield_reg[0] = -2 - v.col;
        } else {
          Compiled c;
          if (int32_t rc = compile_expr(n, cenv, dpb, &c, &err, true)) return E.fail(rc, "YIELD: " + err);
          d.y.yield_reg[0] = c.reg;
        }
        if (int32_t rc = finish_program(E, "YIELD", dpb, &d.y)) return rc;
        plan.distinct.push_back(std::move(d));
        break;
      }
      case NBG_AGG_SUM:
        if (int_like) {
          o = YaOut{YE_SLOT, (uint8_t)slot(key, YA_SUM_I, v, 0), 0};
          otype = v.type;
        } else if (is_dbl) {
          o = YaOut{YE_SLOT, (uint8_t)slot(key, YA_SUM_D, v, 0), 0};
          okind = VK_DOUBLE;
          otype = NBG_T_DOUBLE;
        }
        break;
      case NBG_AGG_AVG:
        okind = VK_DOUBLE;
        otype = NBG_T_DOUBLE;
        is_avg[y] = 1;
        if (v.type == NBG_T_TIMESTAMP) return E.fail(NBG_E_UNSUPPORTED, "YIELD: AVG over a TIMESTAMP-typed argument");
        if (int_like) o = YaOut{YE_AVG_I, (uint8_t)slot(key, YA_SUM_I, v, 0), 0};
        else if (is_dbl) o = YaOut{YE_AVG_D, (uint8_t)slot(key, YA_SUM_D, v, 0), 0};
        else o = YaOut{YE_AVG_0, 0, 0};
        break;
      case NBG_AGG_MAX: case NBG_AGG_MIN: {
        needs_rows = true;
        if (v.is_const) {
          emit_const(v.kind, v.type, v.bits);
          if (v.kind == VK_STRING && (v.bits & 1)) res->const_str[0][y] = v.text;
          break;
        }
        if (int32_t rc = string_by_code("MAX/MIN")) return rc;
        okind = v.kind;
        otype = v.type;
        const YaOp op = fun == NBG_AGG_MAX ? YA_MAX : YA_MIN;
        o = YaOut{(uint8_t)(v.kind == VK_DOUBLE ? YE_ORD_D : YE_ORD_I), (uint8_t)slot(key, op, v, 0), 0};
        break;
      }
      case NBG_AGG_STD:
        if (v.type == NBG_T_INT || is_dbl) {
          const int s = slot(key, is_dbl ? YA_SUM_D : YA_SUM_I, v, 0);
          o = YaOut{YE_STD, (uint8_t)slot(key, YA_SQ, v, s), 0};
          okind = VK_DOUBLE;
          otype = NBG_T_DOUBLE;
          plan.has_sq = true;
        }
        break;
      default: {   // BIT_AND / BIT_OR / BIT_XOR: INT-typed values only
        if (v.type != NBG_T_INT) break;
        const YaOp op = fun == NBG_AGG_BIT_AND ? YA_AND : fun == NBG_AGG_BIT_OR ? YA_OR : YA_XOR;
        o = YaOut{YE_SLOT, (uint8_t)slot(key, op, v, 0), 0};
      }
    }
    res->kinds[0][y] = okind;
    res->col_types[y] = otype;
  }
  if (int32_t rc = finish_program(E, "YIELD", pb, &plan.y)) return rc;
  if (plan.y.nregs + plan.nslots > interp_max_regs())
    return E.fail(NBG_E_UNSUPPORTED, "YIELD: " + std::to_string(plan.y.nregs) + " registers and " + std::to_string(plan.nslots) +
                                         " accumulators are over the register limit (" + std::to_string(interp_max_regs()) +
                                         " fit the LDS)");
  {
    std::set<int32_t> wc, ac = direct;
    for (int pc = 0; pc < (int)plan.y.code.size(); ++pc)
      if (plan.y.code[pc].op == OP_COL) (pc < plan.y.where_len ? wc : ac).insert(plan.y.code[pc].aux);
    plan.y.where_cols = (int)wc.size();
    plan.arg_cols = (int)ac.size();
  }
  // ---- 8. the passes
  DeviceInput d;
  if (int32_t rc = device_input(E, "YIELD", in, &d)) return rc;
  plan.y.str = E.dev_strings();
  plan.y.now_sec = (int64_t)time(nullptr);
  plan.y.rand_seed = query_rand_seed();
  for (YaDistinct& cd : plan.distinct) {
    cd.y.where_cols = plan.y.where_cols;
    cd.y.yield_cols = 1;
    cd.y.str = plan.y.str;
    cd.y.now_sec = plan.y.now_sec;
    cd.y.rand_seed = plan.y.rand_seed;
  }
  Workspace* ow = nullptr;
  uint64_t kept = 0;
  if (int32_t rc = ws_yield_agg(d.w, E.stream, d.segs, plan, &ow, &kept, &E.ya_prof, &E.yr_prof, &E.so_prof, &err)) return E.fail(rc, err);
  RowsWs row;
  row.w = ow;
  // ---- 9. no row kept: a fresh function object's getResult; MAX, MIN and Group::apply hold an
  // empty ColumnValue, which InterimResult::getResultWriter refuses (InterimResult.cpp:602-640)
  if (!kept) {
    if (needs_rows) return E.fail(NBG_E_EXECUTION_ERROR, "Not Support: 0");
    for (int y = 0; y < ny; ++y) {
      res->kinds[0][y] = is_avg[y] ? VK_DOUBLE : VK_INT;
      res->col_types[y] = is_avg[y] ? NBG_T_DOUBLE : NBG_T_INT;
    }
  }
  adopt_rows(res.get(), row.release(), 1, ny);
  *out = res.release();
  return NBG_OK;
}

// ============================================================================= FETCH PROP ON <tag>
// FetchVerticesExecutor / FetchExecutor (src/graph/FetchVerticesExecutor.cpp:19-311,
// src/graph/FetchExecutor.cpp:14-131) over a device-resident result; the kernels are in
// fetchrows.hip and, beside the interpreter, kernels.hip.
namespace {

// what a YIELD tree of a FETCH references (ExpressionContext's has*Prop and aliasProps())
struct FvRefs {
  bool graph = false;   // $^ / $$
  bool input = false;   // $- / $var
  std::vector<std::pair<std::string, std::string>> alias;   // (alias, prop), in evaluation order
};
void fv_refs(const Node& n, FvRefs* r) {
  switch (n.kind) {
    case EK_SRCPROP: case EK_DSTPROP: r->graph = true; break;
    case EK_INPUT: case EK_VAR: r->input = true; break;
    case EK_ALIAS: case EK_RANK: case EK_DST: case EK_SRCID: case EK_TYPE: r->alias.emplace_back(n.alias, n.prop); break;
    default: break;
  }
  for (auto& k : n.kids)
    if (k) fv_refs(*k, r);
}

}  // namespace

int32_t nbg_fetch_vertices(nbg_engine* h, const nbg_rows* in, const nbg_fetch_request* rq, nbg_rows** out) {
  if (!h || !rq || !out) return NBG_E_INVALID_ARGUMENT;
  *out = nullptr;
  Engine& E = h->e;
  std::lock_guard<std::mutex> lg(E.mu);
  // ---- 1. arguments
  if (rq->num_yields < 0 || (rq->num_yields > 0 && (!rq->yield_exprs || !rq->yield_lens)))
    return E.fail(NBG_E_INVALID_ARGUMENT, "FETCH: null argument");
  if (in) {
    if (!rq->input_names || !rq->vid_col) return E.fail(NBG_E_INVALID_ARGUMENT, "FETCH: null argument");
    if (int32_t rc = guard_rows(E, "FETCH", {in})) return rc;
  } else if (!rq->vids && rq->num_vids) {
    return E.fail(NBG_E_INVALID_ARGUMENT, "FETCH: null vid list");
  }
  if (!E.finalized) return E.fail(NBG_E_STATE, "engine not finalized");
  const int nc = in ? in->ncols : 1;
  std::vector<std::string> names;
  if (!in) names.emplace_back("id");
  else if (int32_t rc = copy_input_names(E, "FETCH", rq->input_names, nc, &names)) return rc;
  const std::string vid_col = in ? rq->vid_col : "id";
  std::string err;
  std::vector<std::unique_ptr<Node>> yields;
  for (int y = 0; y < rq->num_yields; ++y) {
    if (!rq->yield_exprs[y] || !rq->yield_lens[y]) return E.fail(NBG_E_INVALID_ARGUMENT, "FETCH: an empty expression");
    yields.push_back(decode_expr(rq->yield_exprs[y], rq->yield_lens[y], &err));
    if (!yields.back()) return E.fail(NBG_E_INVALID_ARGUMENT, "FETCH: " + err);
  }
  // ---- 2.
  if (int32_t rc = guard_partitioned(E, "FETCH")) return rc;
  // ---- 3. prepareClauses (:39-50), prepareVids (:79-81)
  auto tit = E.tags.find(rq->tag_id);
  const Schema* tsc = tit == E.tags.end() ? nullptr : tit->second.latest();
  if (!tsc) return E.fail(NBG_E_EXECUTION_ERROR, "tag " + std::to_string(rq->tag_id) + " schema not exist.");
  const std::string& tag_name = tit->second.name;
  if (in && vid_col == "*") return E.fail(NBG_E_EXECUTION_ERROR, "Cant not use `*' to reference a vertex id column.");
  // ---- no YIELD clause: every column of the latest schema, in order (FetchExecutor::setupColumns, :73-90)
  if (!rq->num_yields)
    for (const Column& col : tsc->cols) {
      auto n = std::make_unique<Node>();
      n->kind = EK_ALIAS;
      n->alias = tag_name;
      n->prop = col.name;
      yields.push_back(std::move(n));
    }
  const int ny = (int)yields.size();
  // ---- 4. prepareYield (FetchExecutor.cpp:50-68), before setupVids: diagnosed for an empty input too
  FvRefs refs;
  for (auto& y : yields) fv_refs(*y, &refs);
  if (refs.graph) return E.fail(NBG_E_SYNTAX_ERROR, "tag.prop and edgetype.prop are supported in fetch sentence.");
  if (refs.input) return E.fail(NBG_E_SYNTAX_ERROR, "`$-' and `$variable' not supported in fetch yet.");
  for (auto& ap : refs.alias)
    if (ap.first != tag_name)
      return E.fail(NBG_E_SYNTAX_ERROR,
                    "Near [" + ap.first + "." + ap.second + "], tag or edge should be declared in statement first.");
  // ---- 5. no rows (onEmptyInputs, FetchExecutor.cpp:99-107): one column per YIELD
  const uint64_t nin = in ? in->count : rq->num_vids;
  if (!nin) {
    *out = new_rows(E, std::min(ny, (int)MAX_YIELDS));
    return NBG_OK;
  }
  // ---- 6. getVIDs -> RowReader::getVid (InterimResult.cpp:29-72, RowReader.cpp:569-576): INT and VID
  // columns only; getPropNames (:142-153, :110-115); the storage request names a prop the schema lacks
  int vcol = 0;
  bool vid_mixed = false;
  if (in) {
    auto it = std::find(names.begin(), names.end(), vid_col);
    vcol = it == names.end() ? -1 : (int)(it - names.begin());
    const InputCols cols(in);
    vid_mixed = vcol >= 0 && cols.mixed[vcol];
    if (vcol < 0 || cols.kind[vcol] != VK_INT || (cols.type[vcol] != NBG_T_INT && cols.type[vcol] != NBG_T_VID))
      return E.fail(NBG_E_EXECUTION_ERROR, "Column `" + vid_col + "' not found");
  }
  if (refs.alias.empty()) return E.fail(NBG_E_EXECUTION_ERROR, "No props declared.");
  for (auto& ap : refs.alias)
    if (tsc->find(ap.second) < 0) return E.fail(NBG_E_EXECUTION_ERROR, "Get props failed");
  // ---- 7. device scope
  if (in && (in->misaligned || in->float_col))
    return E.fail(NBG_E_UNSUPPORTED, "FETCH: the input's row schema re-reads its columns (misaligned or FLOAT)");
  if (vid_mixed) return E.fail(NBG_E_UNSUPPORTED, "FETCH: column `" + vid_col + "' mixes value kinds");
  if (ny > MAX_YIELDS) return E.fail(NBG_E_UNSUPPORTED, "FETCH: more than NBG_MAX_YIELDS columns");
  if (nc < 1 || nc > MAX_YIELDS) return E.fail(NBG_E_INVALID_ARGUMENT, "FETCH: the rows have no columns");
  if (nin > 0xFFFFFFFFull) return E.fail(NBG_E_UNSUPPORTED, "FETCH: an input of 2^32 rows or more");
  auto dit = E.snap.tags.find(rq->tag_id);
  if (dit == E.snap.tags.end() || !dit->second.decoded || !E.snap.d_tcols || !E.snap.d_tpres || !E.snap.d_vids)
    return E.fail(NBG_E_UNSUPPORTED, "FETCH: tag tables missing");
  const DevTag& dtag = dit->second;
  // ---- compile: the YIELDs, one program for every found row
  CompileEnv cenv = stage_env(E, true);
  cenv.dtags = &E.snap.tags;
  cenv.fetch_tag = &tag_name;
  ProgramBuilder pb;
  FvPlan plan;
  plan.y.ncols = ny;
  plan.vid_col = vcol;
  plan.pres = dtag.decoded;
  std::unique_ptr<nbg_rows> res(new_rows(E, ny));
  ColTypeEnv tenv;
  std::set<int32_t> tcols_read;
  for (int y = 0; y < ny; ++y) {
    const Node& n = *yields[y];
    if (n.kind == EK_ALIAS) {   // a bare `tag.prop': the found vertex's column as it is
      const int col = tsc->find(n.prop);
      if (col >= (int)dtag.kind.size()) return E.fail(NBG_E_UNSUPPORTED, "FETCH: tag tables missing");
      plan.y.yield_reg[y] = -2 - (dtag.col_base + col);
      tcols_read.insert(dtag.col_base + col);
      res->kinds[0][y] = dtag.kind[col];
      res->col_types[y] = tsc->cols[col].type;   // FetchExecutor::prepareYield, :37-42
      if (res->col_types[y] == NBG_T_FLOAT) return E.fail(NBG_E_UNSUPPORTED, "FETCH: a bare FLOAT prop (a FLOAT result column)");
      continue;
    }
    if (int32_t rc = compile_yield_column(E, "FETCH", n, cenv, tenv, pb, y, &plan.y, res.get())) return rc;   // :43-47
  }
  if (int32_t rc = finish_program(E, "FETCH", pb, &plan.y)) return rc;
  for (const Ins& i : plan.y.code)
    if (i.op == OP_TAGS_E) tcols_read.insert(i.aux & 0xFFFF);
  plan.tag_cols = (int)tcols_read.size();
  // ---- 8. the passes
  DeviceInput d;
  if (in) {
    if (int32_t rc = device_input(E, "FETCH", in, &d)) return rc;
  } else {   // the literal vids: ws_fetch_vertices uploads them into a temporary one-column result
    if (hipSetDevice(E.cfg.device) != hipSuccess) return E.fail(NBG_E_DEVICE, "hipSetDevice failed");
    d.segs.emplace_back(0, nin);
  }
  plan.y.str = E.dev_strings();
  plan.y.now_sec = (int64_t)time(nullptr);
  plan.y.rand_seed = query_rand_seed();
  plan.vids = E.snap.d_vids;
  plan.nv = E.snap.nv;
  plan.visible = E.snap.d_visible;
  plan.tcols = E.snap.d_tcols;
  plan.tpres = E.snap.d_tpres;
  // (a knob of tools/fetch_probe.py alone, like NBG_SP_*: not part of the interface.  Read per call,
  // so the probe can A/B both searches in one process; a getenv beside milliseconds of kernels)
  if (const char* s = getenv("NBG_FETCH_SEARCH")) plan.search = !strcmp(s, "two-level") ? 2 : 0;
  Workspace* ow = nullptr;
  uint64_t n = 0;
  if (int32_t rc = ws_fetch_vertices(d.w, in ? nullptr : rq->vids, E.stream, d.segs, plan, &ow, &n, &E.fv_prof, &err)) return E.fail(rc, err);
  // ---- YIELD DISTINCT (processResult's uniqResult, :159, :221-228): one row per distinct output
  // row, through nbg_set_op's row table: the UNION DISTINCT of the result's two halves
  if (ow && rq->distinct && n > 1) {
    RowsWs first;   // the result before DISTINCT
    first.w = ow;
    SoPlan sp;
    sp.op = NBG_SET_UNION;
    sp.distinct = 1;
    sp.ncols = ny;
    for (int c = 0; c < ny; ++c) sp.dbl[c] = res->kinds[0][c] == VK_DOUBLE;   // (-0.0 == 0.0, as nbg_set_op)
    const uint64_t half = n / 2;
    ow = nullptr;
    if (int32_t rc = ws_set_op(first.w, first.w, E.stream, {{0, half}}, {{half, n - half}}, sp, &ow, &n, &E.so_prof, &err))
      return E.fail(rc, err);
  }
  if (ow) adopt_rows(res.get(), ow, n, ny);
  *out = res.release();
  return NBG_OK;
}

// ============================================================================= FETCH PROP ON <edge>
// FetchEdgesExecutor / FetchExecutor (src/graph/FetchEdgesExecutor.cpp:17-384,
// src/graph/FetchExecutor.cpp:14-131) over a device-resident result; the kernels are in
// fetchedges.hip and, beside the interpreter, kernels.hip.
int32_t nbg_fetch_edges(nbg_engine* h, const nbg_rows* in, const nbg_fetch_edges_request* rq, nbg_rows** out) {
  if (!h || !rq || !out) return NBG_E_INVALID_ARGUMENT;
  *out = nullptr;
  Engine& E = h->e;
  std::lock_guard<std::mutex> lg(E.mu);
  // ---- 1. arguments
  if (rq->num_yields < 0 || (rq->num_yields > 0 && (!rq->yield_exprs || !rq->yield_lens)))
    return E.fail(NBG_E_INVALID_ARGUMENT, "FETCH: null argument");
  if (in) {
    if (!rq->input_names || !rq->src_col || !rq->dst_col) return E.fail(NBG_E_INVALID_ARGUMENT, "FETCH: null argument");
    if (int32_t rc = guard_rows(E, "FETCH", {in})) return rc;
  } else if ((!rq->srcs || !rq->dsts) && rq->num_keys) {
    return E.fail(NBG_E_INVALID_ARGUMENT, "FETCH: null key list");
  }
  if (!E.finalized) return E.fail(NBG_E_STATE, "engine not finalized");
  const int nc = in ? in->ncols : 3;
  std::vector<std::string> names;
  if (!in) names = {"src", "dst", "rank"};
  else if (int32_t rc = copy_input_names(E, "FETCH", rq->input_names, nc, &names)) return rc;
  // the key columns, in the order setupEdgeKeysFromRef reads them
  std::vector<std::string> key_cols = in ? std::vector<std::string>{rq->src_col, rq->dst_col} : std::vector<std::string>{"src", "dst", "rank"};
  if (in && rq->rank_col) key_cols.emplace_back(rq->rank_col);
  std::string err;
  std::vector<std::unique_ptr<Node>> yields;
  for (int y = 0; y < rq->num_yields; ++y) {
    if (!rq->yield_exprs[y] || !rq->yield_lens[y]) return E.fail(NBG_E_INVALID_ARGUMENT, "FETCH: an empty expression");
    yields.push_back(decode_expr(rq->yield_exprs[y], rq->yield_lens[y], &err));
    if (!yields.back()) return E.fail(NBG_E_INVALID_ARGUMENT, "FETCH: " + err);
  }
  // ---- 2.
  if (int32_t rc = guard_partitioned(E, "FETCH")) return rc;
  // ---- 3. prepareClauses (:36-47), prepareEdgeKeys (:83-88)
  const int32_t type = rq->edge_type;
  auto eit = type > 0 ? E.edges.find(type) : E.edges.end();
  const Schema* esc = eit == E.edges.end() ? nullptr : eit->second.latest();
  if (!esc) return E.fail(NBG_E_EXECUTION_ERROR, "edge type " + std::to_string(type) + ": edge schema not exist.");
  const std::string& edge_name = eit->second.name;
  if (in)
    for (const std::string& kc : key_cols)
      if (kc == "*") return E.fail(NBG_E_EXECUTION_ERROR, "Can not use `*' to reference a vertex id column.");
  // ---- no YIELD clause: every column of the latest schema, in order (FetchExecutor::setupColumns, :73-90)
  if (!rq->num_yields)
    for (const Column& col : esc->cols) {
      auto n = std::make_unique<Node>();
      n->kind = EK_ALIAS;
      n->alias = edge_name;
      n->prop = col.name;
      yields.push_back(std::move(n));
    }
  const int ny = (int)yields.size();
  // ---- 4. prepareYield (FetchExecutor.cpp:50-68), before setupEdgeKeys: diagnosed for an empty input too
  FvRefs refs;
  for (auto& y : yields) fv_refs(*y, &refs);
  if (refs.graph) return E.fail(NBG_E_SYNTAX_ERROR, "tag.prop and edgetype.prop are supported in fetch sentence.");
  if (refs.input) return E.fail(NBG_E_SYNTAX_ERROR, "`$-' and `$variable' not supported in fetch yet.");
  for (auto& ap : refs.alias)
    if (ap.first != edge_name)
      return E.fail(NBG_E_SYNTAX_ERROR,
                    "Near [" + ap.first + "." + ap.second + "], tag or edge should be declared in statement first.");
  // ---- 5. no rows (onEmptyInputs, FetchExecutor.cpp:99-107): one column per YIELD
  const uint64_t nin = in ? in->count : rq->num_keys;
  if (!nin) {
    *out = new_rows(E, std::min(ny, (int)MAX_YIELDS));
    return NBG_OK;
  }
  // ---- 6. getVIDs -> RowReader::getVid per key column (:158-176): INT and VID columns only;
  // getPropNames (:270-274); the storage request names a prop the schema lacks (:280-283)
  int kcol[3] = {0, 1, in ? -1 : 2};
  bool key_mixed = false;
  std::string mixed_name;
  if (in) {
    const InputCols cols(in);
    for (size_t k = 0; k < key_cols.size(); ++k) {
      auto it = std::find(names.begin(), names.end(), key_cols[k]);
      const int c = it == names.end() ? -1 : (int)(it - names.begin());
      if (c < 0 || cols.kind[c] != VK_INT || (cols.type[c] != NBG_T_INT && cols.type[c] != NBG_T_VID))
        return E.fail(NBG_E_EXECUTION_ERROR, "Column `" + key_cols[k] + "' not found");
      if (cols.mixed[c] && !key_mixed) {
        key_mixed = true;
        mixed_name = key_cols[k];
      }
      kcol[k] = c;
    }
  }
  auto key_prop = [](const std::string& p) { return p == "_src" || p == "_dst" || p == "_rank" || p == "_type"; };
  if (refs.alias.empty()) return E.fail(NBG_E_EXECUTION_ERROR, "No props declared.");
  for (auto& ap : refs.alias)
    if (!key_prop(ap.second) && esc->find(ap.second) < 0) return E.fail(NBG_E_EXECUTION_ERROR, "Get props failed");
  // ---- 7. device scope
  if (in && (in->misaligned || in->float_col))
    return E.fail(NBG_E_UNSUPPORTED, "FETCH: the input's row schema re-reads its columns (misaligned or FLOAT)");
  if (key_mixed) return E.fail(NBG_E_UNSUPPORTED, "FETCH: column `" + mixed_name + "' mixes value kinds");
  if (ny > MAX_YIELDS) return E.fail(NBG_E_UNSUPPORTED, "FETCH: more than NBG_MAX_YIELDS columns");
  if (nc < 1 || nc > MAX_YIELDS) return E.fail(NBG_E_INVALID_ARGUMENT, "FETCH: the rows have no columns");
  if (nin > 0xFFFFFFFFull) return E.fail(NBG_E_UNSUPPORTED, "FETCH: an input of 2^32 rows or more");
  auto dit = E.snap.types.find(type);
  if (dit == E.snap.types.end() || !dit->second.row_ptr || !dit->second.dst_vid || !dit->second.d_props || !E.snap.d_vids)
    return E.fail(NBG_E_UNSUPPORTED, "FETCH: the edge type has no device CSR");
  const DevEdgeType& dt = dit->second;
  // ---- compile: the YIELDs in the per-edge mode of a GO over this one type, one program for every found row
  const std::vector<int32_t> over{type};
  CompileEnv cenv{type, &over, &E.edges, &E.snap.strings, dt.valid != nullptr, dt.rank != nullptr};
  cenv.tags = &E.tags;
  cenv.max_dict_len = E.refresh_max_dict_len();
  ProgramBuilder pb;
  FePlan plan;
  plan.y.ncols = ny;
  plan.src_col = kcol[0];
  plan.dst_col = kcol[1];
  plan.rank_col = kcol[2];
  std::unique_ptr<nbg_rows> res(new_rows(E, ny));
  ColTypeEnv tenv;
  std::set<int32_t> pcols_read;
  for (int y = 0; y < ny; ++y) {
    const Node& n = *yields[y];
    const int col = n.kind == EK_ALIAS ? esc->find(n.prop) : -1;
    if (col >= 0) {   // a bare `edge.prop': the found edge's column as it is
      if (col >= (int)dt.props.size() || col >= (int)dt.prop_kind.size())
        return E.fail(NBG_E_UNSUPPORTED, "FETCH: the edge type has no device CSR");
      plan.y.yield_reg[y] = -2 - col;
      pcols_read.insert(col);
      res->kinds[0][y] = dt.prop_kind[col];
      res->col_types[y] = esc->cols[col].type;   // FetchExecutor::prepareYield, :37-42
      if (res->col_types[y] == NBG_T_FLOAT) return E.fail(NBG_E_UNSUPPORTED, "FETCH: a bare FLOAT prop (a FLOAT result column)");
      continue;
    }
    if (int32_t rc = compile_yield_column(E, "FETCH", n, cenv, tenv, pb, y, &plan.y, res.get())) return rc;   // :43-47
  }
  if (int32_t rc = finish_program(E, "FETCH", pb, &plan.y)) return rc;
  bool reads_dst = false, reads_rank = false;
  for (const Ins& i : plan.y.code) {
    if (i.op == OP_COL || i.op == OP_COLV) pcols_read.insert(i.aux);
    plan.need_src = plan.need_src || i.op == OP_SRC;
    reads_dst = reads_dst || i.op == OP_DST;
    reads_rank = reads_rank || (i.op == OP_RANK && dt.rank);
  }
  plan.prop_cols = (int)pcols_read.size() + reads_dst + reads_rank;
  // ---- 8. the passes
  DeviceInput d;
  if (in) {
    if (int32_t rc = device_input(E, "FETCH", in, &d)) return rc;
  } else {   // the literal keys: ws_fetch_edges uploads them into a temporary three-column result
    if (hipSetDevice(E.cfg.device) != hipSuccess) return E.fail(NBG_E_DEVICE, "hipSetDevice failed");
    d.segs.emplace_back(0, nin);
  }
  plan.y.str = E.dev_strings();
  plan.y.now_sec = (int64_t)time(nullptr);
  plan.y.rand_seed = query_rand_seed();
  plan.vids = E.snap.d_vids;
  plan.nv = E.snap.nv;
  plan.visible = E.snap.d_visible;
  plan.row_ptr = dt.row_ptr;
  plan.dst_vid = dt.dst_vid;
  plan.rank = dt.rank;
  plan.valid = dt.valid;
  plan.props = dt.d_props;
  Workspace* ow = nullptr;
  uint64_t n = 0;
  if (int32_t rc = ws_fetch_edges(d.w, in ? nullptr : rq->srcs, rq->dsts, rq->ranks, E.stream, d.segs, plan, &ow, &n, &E.fe_prof, &err))
    return E.fail(rc, err);
  // ---- YIELD DISTINCT (processResult's uniqResult, :322, :371-375): one row per distinct output
  // row, through nbg_set_op's row table: the UNION DISTINCT of the result's two halves
  if (ow && rq->distinct && n > 1) {
    RowsWs first;   // the result before DISTINCT
    first.w = ow;
    SoPlan sp;
    sp.op = NBG_SET_UNION;
    sp.distinct = 1;
    sp.ncols = ny;
    for (int c = 0; c < ny; ++c) sp.dbl[c] = res->kinds[0][c] == VK_DOUBLE;   // (-0.0 == 0.0, as nbg_set_op)
    const uint64_t half = n / 2;
    ow = nullptr;
    if (int32_t rc = ws_set_op(first.w, first.w, E.stream, {{0, half}}, {{half, n - half}}, sp, &ow, &n, &E.so_prof, &err))
      return E.fail(rc, err);
  }
  if (ow) adopt_rows(res.get(), ow, n, ny);
  *out = res.release();
  return NBG_OK;
}

// ============================================================================= RowSet encoding
// What GoExecutor::setupInterimResult (GoExecutor.cpp:707-779) and InterimResult (InterimResult.cpp:
// 602-640) make of a result: the schema's field types and the RowSetWriter bytes of every row; the
// kernels are in rowenc.hip.
int32_t nbg_rows_col_type(const nbg_rows* r, int32_t col) {
  if (!r || col < 0 || col >= r->ncols) return -1;
  return InputCols(r).type[col];
}

int32_t nbg_rows_encode(nbg_engine* h, const nbg_rows* in, nbg_rowset** out) {
  if (!h || !in || !out) return NBG_E_INVALID_ARGUMENT;
  *out = nullptr;
  Engine& E = h->e;
  std::lock_guard<std::mutex> lg(E.mu);
  // ---- 1., 2.
  if (int32_t rc = guard_rows(E, "rows encode", {in})) return rc;
  if (int32_t rc = guard_partitioned(E, "rows encode")) return rc;
  const int nc = in->ncols;
  const InputCols cols(in);
  auto res = std::make_unique<nbg_rowset>();
  res->eng = &E;
  res->types = cols.type;
  // ---- 3.
  if (!in->count) {
    *out = res.release();
    return NBG_OK;
  }
  // ---- 4. device scope
  if (in->misaligned || in->float_col)
    return E.fail(NBG_E_UNSUPPORTED, "rows encode: the input's row schema re-reads its columns (misaligned or FLOAT)");
  if (nc < 1 || nc > MAX_YIELDS) return E.fail(NBG_E_INVALID_ARGUMENT, "rows encode: the rows have no columns");
  if (cols.any_mixed) return E.fail(NBG_E_UNSUPPORTED, "rows encode: a column mixes value kinds between OVER types");
  RePlan plan;
  plan.ncols = nc;
  std::vector<uint8_t> is_string(nc, 0);
  uint64_t widest = 1 + 2 * 8;   // the header byte and two block offsets
  for (int c = 0; c < nc; ++c) {
    const int32_t t = cols.type[c];
    if (t == NBG_T_FLOAT) return E.fail(NBG_E_UNSUPPORTED, "rows encode: a FLOAT column");
    // (the cell is written by its type: a kind the type's reader would not take back is no aligned result)
    const VKind reads = t == NBG_T_BOOL ? VK_BOOL : t == NBG_T_DOUBLE ? VK_DOUBLE : t == NBG_T_STRING ? VK_STRING : VK_INT;
    if (cols.kind[c] != reads)
      return E.fail(NBG_E_UNSUPPORTED, "rows encode: column " + std::to_string(c) + " holds another kind than its type reads");
    plan.type[c] = (uint8_t)t;
    is_string[c] = t == NBG_T_STRING;
    if (is_string[c] && !in->derived.empty())
      return E.fail(NBG_E_UNSUPPORTED, "rows encode: string column " + std::to_string(c) +
                                           " can hold strings outside the dictionary (derived strings)");
    uint64_t cell = 10;
    if (is_string[c]) {
      cell = E.refresh_max_dict_len();
      for (auto& cs : in->const_str)
        if (c < (int)cs.size()) cell = std::max<uint64_t>(cell, cs[c].size());
      cell += 5;
    }
    widest += cell;
  }
  if (in->count > 0xFFFFFFFFull) return E.fail(NBG_E_UNSUPPORTED, "rows encode: an input of 2^32 rows or more");
  if (widest + 10 > 0xFFFFFFFFull)   // (a row's length is a 32-bit word between the passes)
    return E.fail(NBG_E_UNSUPPORTED, "rows encode: a row could encode to 4 GiB or more");
  // ---- the segments in fetch order, each chunk's OVER position, the constants outside the dictionary
  DeviceInput d;
  if (int32_t rc = device_input(E, "rows encode", in, &d)) return rc;
  for (int t : d.types)
    if (t < 0 || t >= (int)in->const_str.size() || t > 255)
      return E.fail(NBG_E_DEVICE, "rows encode: a segment of an unknown OVER position");
  plan.chunk_type = re_chunk_types(d.segs, d.types, OB_CHUNK);
  ReConsts consts = re_const_table(in->const_str, is_string, nc);
  if (!consts.fits) return E.fail(NBG_E_UNSUPPORTED, "rows encode: 4 GiB or more of string constants");
  plan.koff = std::move(consts.off);
  plan.kbytes = std::move(consts.bytes);
  plan.str = E.dev_strings();
  // ---- 5. the passes
  auto grow = [](void* ctx, uint64_t bytes) -> void* {
    auto* rs = static_cast<nbg_rowset*>(ctx);
    rs->data = static_cast<uint8_t*>(rs->eng->pinned_get((size_t)bytes, &rs->cap));
    return rs->data;
  };
  std::string err;
  const int32_t rc = ws_rows_encode(d.w, E.stream, d.segs, plan, grow, res.get(), &res->len, &E.re_prof, &err);
  if (rc) {
    if (res->data) E.pinned_put(res->data, res->cap);
    return E.fail(rc, err);
  }
  res->rows = in->count;
  *out = res.release();
  return NBG_OK;
}

const uint8_t* nbg_rowset_data(const nbg_rowset* rs) { return rs ? rs->data : nullptr; }
uint64_t nbg_rowset_len(const nbg_rowset* rs) { return rs ? rs->len : 0; }
int64_t nbg_rowset_rows(const nbg_rowset* rs) { return rs ? (int64_t)rs->rows : 0; }
int32_t nbg_rowset_num_cols(const nbg_rowset* rs) { return rs ? (int32_t)rs->types.size() : 0; }
int32_t nbg_rowset_col_type(const nbg_rowset* rs, int32_t col) {
  return rs && col >= 0 && col < (int32_t)rs->types.size() ? rs->types[col] : -1;
}
void nbg_rowset_free(nbg_rowset* rs) {
  if (!rs) return;
  if (rs->eng && rs->data) rs->eng->pinned_put(rs->data, rs->cap);
  delete rs;
}

// ============================================================================= RowSet decoding
// The way back in: what InterimResult::getRows / buildIndex read with a RowReader per row
// (InterimResult.cpp:74-140, 158-250; RowReader.cpp:213-258; RowSetReader.cpp) becomes an ordinary
// device-resident result.  The walk and the cell reader are in rowdec.h, the kernel in rowdec.hip.
int32_t nbg_rows_decode(nbg_engine* h, const nbg_rowset_view* rs, nbg_rows** out) {
  if (!h || !rs || !out) return NBG_E_INVALID_ARGUMENT;
  *out = nullptr;
  Engine& E = h->e;
  std::lock_guard<std::mutex> lg(E.mu);
  // ---- 1. arguments
  if (!rs->col_types) return E.fail(NBG_E_INVALID_ARGUMENT, "rows decode: null argument");
  if (rs->num_cols < 1) return E.fail(NBG_E_INVALID_ARGUMENT, "rows decode: a schema without fields");
  const int nc = rs->num_cols;
  for (int c = 0; c < nc; ++c)
    if (rs->col_types[c] < NBG_T_BOOL || rs->col_types[c] > NBG_T_TIMESTAMP)
      return E.fail(NBG_E_INVALID_ARGUMENT, "rows decode: field " + std::to_string(c) + " has no NBG_T_* type");
  if (rs->len && !rs->data) return E.fail(NBG_E_INVALID_ARGUMENT, "rows decode: null data");
  if (!E.finalized) return E.fail(NBG_E_STATE, "engine not finalized");
  // ---- 2.
  if (int32_t rc = guard_partitioned(E, "rows decode")) return rc;
  std::unique_ptr<nbg_rows> res(new_rows(E, nc));
  for (int c = 0; c < nc; ++c) {
    res->col_types[c] = rs->col_types[c];
    res->kinds[0][c] = kindOfType(rs->col_types[c]);
  }
  // ---- 3.
  if (!rs->len) {
    *out = res.release();
    return NBG_OK;
  }
  // ---- 4. device scope: the schema, then what only the walk can tell
  if (nc > MAX_YIELDS) return E.fail(NBG_E_UNSUPPORTED, "rows decode: more than NBG_MAX_YIELDS fields");
  RdPlan plan;
  plan.ncols = nc;
  for (int c = 0; c < nc; ++c) {
    if (rs->col_types[c] == NBG_T_FLOAT)
      return E.fail(NBG_E_UNSUPPORTED, "rows decode: a FLOAT field (the aligned result has no FLOAT column)");
    plan.type[c] = (uint8_t)rs->col_types[c];
  }
  const auto t0 = std::chrono::steady_clock::now();
  const RdIndex ix = rd_walk(rs->data, rs->len, nc);
  if (E.rd_prof.on) {
    E.rd_prof.launches[RD_K_WALK]++;
    E.rd_prof.ms[RD_K_WALK] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    E.rd_prof.bytes[RD_K_WALK] += (double)rs->len;
  }
  if (ix.status == RD_WALK_ROWS) return E.fail(NBG_E_UNSUPPORTED, "rows decode: an input of 2^32 rows or more");
  if (ix.status == RD_WALK_CHUNK)
    return E.fail(NBG_E_UNSUPPORTED, "rows decode: a chunk of 2,048 rows whose bytes reach 4 GiB");
  // ---- 5. malformed bytes
  if (rd_walk_malformed(ix.status)) {
    const char* what = ix.status == RD_WALK_PREFIX     ? "a length prefix over 10 bytes or running past the end"
                       : ix.status == RD_WALK_PAST_END ? "a row running past the end"
                       : ix.status == RD_WALK_EMPTY_ROW ? "a row of length 0 (no header byte)"
                                                        : "a row shorter than its own header";
    return E.fail(NBG_E_INVALID_ARGUMENT, std::string("rows decode: ") + what + " (row " + std::to_string(ix.bad_row) +
                                              ", byte " + std::to_string(ix.bad_at) + ")");
  }
  // ---- the pass
  if (hipSetDevice(E.cfg.device) != hipSuccess) return E.fail(NBG_E_DEVICE, "hipSetDevice failed");
  plan.str = E.dev_strings();
  size_t cap = 0;
  void* block = E.pinned_get((size_t)rd_block_bytes(rs->len, ix.chunk_start.size(), ix.rows), &cap);
  if (!block) return E.fail(NBG_E_OUT_OF_MEMORY, "rows decode: pinned host memory for the row bytes");
  Workspace* ow = nullptr;
  RdRecord rec;
  std::string err;
  const int32_t rc = ws_rows_decode(E.stream, rs->data, rs->len, ix.chunk_start.data(), ix.chunk_start.size(), ix.row_off.data(),
                                    ix.rows, block, plan, &ow, &rec, &E.rd_prof, &err);
  E.pinned_put(block, cap);
  if (rc) return E.fail(rc, err);
  RowsWs hold;   // (destroyed unless the result adopts it)
  hold.w = ow;
  // ---- 6., 7.
  if (rec.malformed)
    return E.fail(NBG_E_INVALID_ARGUMENT, "rows decode: " + std::to_string(rec.malformed) +
                                              " row(s) whose cells would read past the row's end; the first is row " +
                                              std::to_string(rec.first >> 6) + ", column " + std::to_string(rec.first & 63));
  if (rec.missing)
    return E.fail(NBG_E_UNSUPPORTED, "rows decode: " + std::to_string(rec.missing) +
                                         " STRING cell(s) whose bytes are not in the snapshot's dictionary");
  adopt_rows(res.get(), hold.release(), ix.rows, nc);
  *out = res.release();
  return NBG_OK;
}

}  // extern "C"
