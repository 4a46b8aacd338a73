// nebula_amd — piped YIELD with aggregate functions and no GROUP BY over a device-resident result
// (gfx950, wave64).  YieldExecutor::executeInputs with checkAggFun's functions
// (src/graph/YieldExecutor.cpp:33-58, :178-282; AggregateFunction.h) over the row segments earlier
// stages leave in HBM: a streaming reduction, no table and no atomics.
//   k_ya_reduce   (kernels.hip, beside the interpreter) the WHERE and the arguments per row; per
//                 chunk one partial per accumulator slot and the kept count, plain stores
//   k_ya_finish   one workgroup folds every slot's partials in a fixed order of the chunk index,
//                 writes the means a STD measures from and, on the last pass, the result row
//   k_ya_reduce   again for STD: the squared distances from the now known means; k_ya_finish again
// The partials are per chunk and the fold's order depends on the chunk count alone, so a result
// does not depend on the grid or on scheduling.  COUNT_DISTINCT materialises its argument over the
// kept rows (ws_yield_rows) and counts the rows of its UNION DISTINCT (ws_set_op).  The host waits
// once, for the kept count and the error word.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "aggops.h"
#include "stage.h"
#include "ws.h"

namespace nbg {

const char* const kYaKernelNames[YA_KINDS] = {"k_ya_reduce", "k_ya_finish"};

namespace {

struct YaFinArgs {
  const uint64_t* partial;   // [nslots][nchunks]
  const uint32_t* ccount;    // [nchunks]
  uint32_t nchunks;
  const YaSlot* slot;
  int nslots;
  int pass;                  // as k_ya_reduce's
  int last;                  // the result row is written
  uint64_t* tot;             // [nslots]: every slot's fold
  double* mean;              // [nslots]: pass 0 writes the mean of each YA_SQ slot
  YrState* st;               // total: the kept count
  const YaOut* out;
  int nout;
  int64_t* cells;            // column c's cell at cells[c * stride]
  uint64_t stride;
};

// thread t folds the chunks [t * per, (t + 1) * per) in order, then the workgroup's fold
// (ya_block_reduce): an order the chunk count alone decides
__global__ void __launch_bounds__(BLOCK) k_ya_finish(YaFinArgs f) {
  __shared__ uint64_t wp[WAVES];
  const uint32_t per = (f.nchunks + BLOCK - 1) / BLOCK;
  const uint64_t first = (uint64_t)threadIdx.x * per;
  const uint32_t lo = first < f.nchunks ? (uint32_t)first : f.nchunks;
  const uint32_t hi = first + per < f.nchunks ? (uint32_t)(first + per) : f.nchunks;
  if (f.pass == 0) {
    uint64_t c = 0;
    for (uint32_t i = lo; i < hi; ++i) c += f.ccount[i];
    c = ya_block_reduce(YA_SUM_I, c, wp);
    if (threadIdx.x == 0) f.st->total = c;
  }
  for (int s = 0; s < f.nslots; ++s) {
    const uint8_t op = f.slot[s].op;
    if (!ya_in_pass(op, f.pass)) continue;
    uint64_t v = ya_identity(op);
    for (uint32_t i = lo; i < hi; ++i) v = ya_combine(op, v, f.partial[(size_t)s * f.nchunks + i]);
    v = ya_block_reduce(op, v, wp);
    if (threadIdx.x == 0) f.tot[s] = v;
  }
  __syncthreads();   // (thread 0's stores, read below by the others)
  const uint64_t n = f.st->total;
  if (f.pass == 0 && (int)threadIdx.x < f.nslots && f.slot[threadIdx.x].op == YA_SQ)
    f.mean[threadIdx.x] = ya_avg(f.tot[f.slot[threadIdx.x].ref], f.slot[threadIdx.x].dbl, n);
  if (!f.last || (int)threadIdx.x >= f.nout) return;
  const YaOut o = f.out[threadIdx.x];
  const bool avg = o.emit == YE_AVG_I || o.emit == YE_AVG_D || o.emit == YE_AVG_0;
  const double nan = __ddiv_rn(0.0, 0.0);   // no row kept: AVG is 0.0 / 0, everything else 0
  uint64_t cell = avg ? (uint64_t)__double_as_longlong(nan) : 0ull;
  if (n) {
    const uint64_t t = f.tot[o.slot];
    switch (o.emit) {
      case YE_CONST: cell = (uint64_t)o.bits; break;
      case YE_COUNT: cell = n; break;
      case YE_SLOT: cell = t; break;
      case YE_ORD_I: cell = ord_unimage(t, 0); break;
      case YE_ORD_D: cell = ord_unimage(t, 1); break;
      case YE_AVG_I: cell = (uint64_t)__double_as_longlong(ya_avg(t, false, n)); break;
      case YE_AVG_D: cell = (uint64_t)__double_as_longlong(ya_avg(t, true, n)); break;
      case YE_AVG_0: cell = 0ull; break;
      default: cell = (uint64_t)__double_as_longlong(__dsqrt_rn(__ddiv_rn(__longlong_as_double((long long)t), (double)n)));
    }
  }
  f.cells[threadIdx.x * f.stride] = (int64_t)cell;
}

}  // namespace

int32_t ws_yield_agg(Workspace* inw, hipStream_t stream, const std::vector<std::pair<uint64_t, uint64_t>>& segs,
                     const YaPlan& plan, Workspace** outw, uint64_t* kept, StageProf<YA_KINDS>* prof,
                     StageProf<YR_KINDS>* yr_prof, StageProf<SO_KINDS>* so_prof, std::string* err) {
  *outw = nullptr;
  *kept = 0;
  StageStatus cs("YIELD");
  const YrPlan& yp = plan.y;
  uint64_t n = 0;
  for (auto& sg : segs) n += sg.second;
  if (plan.nout < 1 || plan.nout > MAX_YIELDS || plan.nslots < 0 || plan.nslots > YA_MAX_SLOTS || !n || n > 0xFFFFFFFFull ||
      yp.code.size() + yp.data.size() > (size_t)MAX_PROGRAM || yp.where_len < 0 || (size_t)yp.where_len > yp.code.size() ||
      (yp.where_reg >= 0) != (yp.where_len > 0) || yp.where_reg >= yp.nregs) {
    if (err) *err = "YIELD: empty input or plan";
    return NBG_E_INVALID_ARGUMENT;
  }
  for (int s = 0; s < plan.nslots; ++s)
    if (plan.slot[s].src >= yp.nregs || (plan.slot[s].op == YA_SQ && plan.slot[s].ref >= plan.nslots)) {
      if (err) *err = "YIELD: a slot outside the plan";
      return NBG_E_INVALID_ARGUMENT;
    }
  if (yp.nregs + plan.nslots > interp_max_regs()) {
    if (err)
      *err = "YIELD: " + std::to_string(yp.nregs) + " registers and " + std::to_string(plan.nslots) +
             " accumulators are over the register limit (" + std::to_string(interp_max_regs()) + " fit the LDS)";
    return NBG_E_UNSUPPORTED;
  }

  RowsWs res;
  StageScratch sc;   // (declared before the timer: the timer's events are resolved first)
  StageTimer<YA_KINDS> tm{prof, stream, {}, nullptr};
  StageChunks ch;
  YaArgs a{};
  YrState* st = nullptr;
  YaSlot* d_slot = nullptr;
  YaOut* d_out = nullptr;
  uint64_t* tot = nullptr;
  double* mean = nullptr;
  uint32_t* ccount = nullptr;
  const int ns = plan.nslots;
  if (cs.failed(sc.alloc((void**)&d_slot, ns * sizeof(YaSlot)), "slots") || cs.failed(sc.alloc((void**)&d_out, plan.nout * sizeof(YaOut)), "emit rules") ||
      cs.failed(sc.alloc((void**)&tot, ns * 8), "totals") || cs.failed(sc.alloc((void**)&mean, ns * 8), "means") ||
      (ns && cs.failed(hipMemcpyAsync(d_slot, plan.slot, ns * sizeof(YaSlot), hipMemcpyHostToDevice, stream), "slot upload")) ||
      cs.failed(hipMemcpyAsync(d_out, plan.out, plan.nout * sizeof(YaOut), hipMemcpyHostToDevice, stream), "emit upload") ||
      cs.failed(hipMemsetAsync(tot, 0, ns ? ns * 8 : 8, stream), "totals clear") ||
      ch.upload(cs, sc, stream, segs, 0, plan.none ? 0 : n) || yr_setup(cs, sc, stream, yp, ch, inw, &a.y, &st) ||
      cs.failed(sc.alloc((void**)&a.partial, (size_t)ns * ch.n * 8), "partials") ||
      cs.failed(sc.alloc((void**)&ccount, (size_t)ch.n * 4), "chunk counts") || cs.failed(res.reserve(stream, 1, plan.nout), "result row"))
    return cs.code(err);
  a.y.ccount = ccount;
  a.slot = d_slot;
  a.nslots = ns;
  a.nregs = yp.nregs;
  a.mean = mean;
  YaFinArgs f{a.partial, ccount, ch.n, d_slot, ns, 0, 0, tot, mean, st, d_out, plan.nout, ws_row_col(res.w, 0), 0};
  f.stride = plan.nout > 1 ? (uint64_t)(ws_row_col(res.w, 1) - ws_row_col(res.w, 0)) : 0;
  const int read_cols = yp.where_cols + plan.arg_cols;
  for (int pass = 0; pass < (plan.has_sq ? 2 : 1); ++pass) {
    a.pass = f.pass = pass;
    f.last = pass == (plan.has_sq ? 1 : 0);
    tm.begin();
    hipError_t he = launch_ya_reduce(a, ch.grid, stream);
    tm.end(YA_K_REDUCE, (double)(plan.none ? 0 : n) * 8.0 * read_cols + (double)ch.n * (8.0 * ns + 4.0));
    if (cs.failed(he, "k_ya_reduce")) return cs.code(err);
    tm.begin();
    hipLaunchKernelGGL(k_ya_finish, dim3(1), dim3(BLOCK), 0, stream, f);
    he = hipGetLastError();
    tm.end(YA_K_FINISH, (double)ch.n * (8.0 * ns + 4.0));
    if (cs.failed(he, "k_ya_finish")) return cs.code(err);
  }
  YrState got{};
  if (cs.failed(hipMemcpyAsync(&got, st, sizeof(YrState), hipMemcpyDeviceToHost, stream), "kept rows read") ||
      cs.failed(hipStreamSynchronize(stream), "reduction"))
    return cs.code(err);
  if (got.err) {
    if (err) *err = "YIELD: an evaluation error in the WHERE clause or in an argument of a kept row";
    return NBG_E_EXECUTION_ERROR;
  }
  if (got.total > n) {
    if (err) *err = "YIELD: " + std::to_string(got.total) + " rows kept of " + std::to_string(n);
    return NBG_E_DEVICE;
  }
  // ---- COUNT_DISTINCT: the argument of the kept rows as a one-column result, then the rows of the
  // UNION DISTINCT of its two halves (nbg_fetch_vertices' DISTINCT)
  std::vector<int64_t> counts(plan.distinct.size(), 0);   // (outlives the uploads below)
  for (size_t k = 0; got.total && k < plan.distinct.size(); ++k) {
    const YaDistinct& d = plan.distinct[k];
    RowsWs vals;
    uint64_t m = 0;
    if (int32_t rc = ws_yield_rows(inw, stream, segs, d.y, &vals.w, &m, yr_prof, err)) return rc;
    if (vals.w && m > 1) {
      SoPlan sp;
      sp.op = NBG_SET_UNION;
      sp.distinct = 1;
      sp.ncols = 1;
      sp.dbl[0] = d.dbl;
      RowsWs uniq;
      const uint64_t half = m / 2;
      if (int32_t rc = ws_set_op(vals.w, vals.w, stream, {{0, half}}, {{half, m - half}}, sp, &uniq.w, &m, so_prof, err)) return rc;
    }
    counts[k] = (int64_t)m;
    if (cs.failed(hipMemcpyAsync(ws_row_col(res.w, d.out), &counts[k], 8, hipMemcpyHostToDevice, stream), "distinct count"))
      return cs.code(err);
  }
  if (got.total && !plan.distinct.empty() && cs.failed(hipStreamSynchronize(stream), "distinct counts")) return cs.code(err);
  *outw = res.release();
  *kept = got.total;
  return NBG_OK;
}

}  // namespace nbg
