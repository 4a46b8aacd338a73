// nebula_amd — piped YIELD ... WHERE over a device-resident result (gfx950, wave64).
// YieldExecutor::executeInputs (src/graph/YieldExecutor.cpp:178-282) over the row segments earlier
// stages leave in HBM.  One program (WHERE first, then the YIELDs), compiled in CompileEnv's rows
// mode, runs per row through the GO interpreter; the kernels that call it sit beside it in
// kernels.hip (launch_yr_filter, launch_yr_emit):
//   k_yr_filter   the WHERE per row: one keep byte per logical row, one count per chunk
//   k_yr_scan     exclusive scan of the chunk counts into chunk bases and the total (one workgroup)
//   k_yr_emit     the YIELDs of the kept rows, stored at chunk base + rank within the chunk, so the
//                 result keeps the input's fetch order
// Without a WHERE the first two are skipped and a row's slot is its logical index.  The input is
// walked through the chunk list of stage.h, one workgroup per chunk.  No kernel waits on another
// workgroup: every dependency is a kernel boundary on one stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "stage.h"
#include "ws.h"

namespace nbg {

const char* const kYrKernelNames[YR_KINDS] = {"k_yr_filter", "k_yr_scan", "k_yr_emit"};

namespace {

// base[k] = sum of count[0..k), st->total = the sum of all; each thread scans a contiguous slice
__global__ void __launch_bounds__(BLOCK) k_yr_scan(const uint32_t* __restrict__ count, uint32_t n,
                                                   uint32_t* __restrict__ base, YrState* __restrict__ st) {
  __shared__ uint32_t lds[WAVES];
  const uint32_t per = (n + BLOCK - 1) / BLOCK;
  const uint64_t first = (uint64_t)threadIdx.x * per;
  const uint32_t lo = first < n ? (uint32_t)first : n;
  const uint32_t hi = first + per < n ? (uint32_t)(first + per) : n;
  uint32_t sum = 0;
  for (uint32_t i = lo; i < hi; ++i) sum += count[i];
  uint32_t total = 0;
  uint32_t run = block_excl_scan(sum, &total, lds);
  for (uint32_t i = lo; i < hi; ++i) {
    base[i] = run;
    run += count[i];
  }
  if (threadIdx.x == 0) st->total = total;
}

}  // namespace

hipError_t launch_yr_scan(const uint32_t* count, uint32_t n, uint32_t* base, YrState* st, hipStream_t s) {
  hipLaunchKernelGGL(k_yr_scan, dim3(1), dim3(BLOCK), 0, s, count, n, base, st);
  return hipGetLastError();
}

int32_t ws_yield_rows(Workspace* inw, hipStream_t stream, const std::vector<std::pair<uint64_t, uint64_t>>& segs,
                      const YrPlan& plan, Workspace** outw, uint64_t* rows, StageProf<YR_KINDS>* prof, std::string* err) {
  *outw = nullptr;
  *rows = 0;
  StageStatus cs("YIELD");
  uint64_t n = 0;
  for (auto& sg : segs) n += sg.second;
  if (plan.ncols < 1 || plan.ncols > MAX_YIELDS || !n || n > 0xFFFFFFFFull || plan.code.size() + plan.data.size() > (size_t)MAX_PROGRAM ||
      plan.where_len < 0 || (size_t)plan.where_len > plan.code.size() || (plan.where_reg >= 0) != (plan.where_len > 0) ||
      plan.where_reg >= plan.nregs) {
    if (err) *err = "YIELD: empty input or plan";
    return NBG_E_INVALID_ARGUMENT;
  }

  RowsWs res;
  StageScratch sc;   // (declared before the timer: the timer's events are resolved first)
  StageTimer<YR_KINDS> tm{prof, stream, {}, nullptr};
  StageChunks ch;
  YrArgs a{};
  YrState* st = nullptr;
  if (ch.upload(cs, sc, stream, segs, 0, n) || yr_setup(cs, sc, stream, plan, ch, inw, &a, &st)) return cs.code(err);

  uint64_t nout = n;
  YrState got{};
  if (plan.where_reg >= 0) {
    uint32_t* ccount = nullptr;
    uint32_t* cbase = nullptr;
    if (cs.failed(sc.alloc((void**)&a.keep, n), "keep flags") || cs.failed(sc.alloc((void**)&ccount, (size_t)ch.n * 4), "chunk counts") ||
        cs.failed(sc.alloc((void**)&cbase, (size_t)ch.n * 4), "chunk bases"))
      return cs.code(err);
    a.ccount = ccount;
    a.cbase = cbase;
    tm.begin();
    hipError_t he = launch_yr_filter(a, plan.nregs, ch.grid, stream);
    tm.end(YR_K_FILTER, (double)n * (8.0 * plan.where_cols + 1.0));
    if (cs.failed(he, "k_yr_filter")) return cs.code(err);
    tm.begin();
    he = launch_yr_scan(ccount, ch.n, cbase, st, stream);
    tm.end(YR_K_SCAN, (double)ch.n * 8.0);
    if (cs.failed(he, "k_yr_scan") ||
        cs.failed(hipMemcpyAsync(&got, st, sizeof(YrState), hipMemcpyDeviceToHost, stream), "kept rows read") ||
        cs.failed(hipStreamSynchronize(stream), "filter"))
      return cs.code(err);
    if (got.err) {
      if (err) *err = "YIELD: an evaluation error in the WHERE clause";
      return NBG_E_EXECUTION_ERROR;
    }
    nout = got.total;
    if (nout > n) {
      if (err) *err = "YIELD: " + std::to_string(nout) + " rows kept of " + std::to_string(n);
      return NBG_E_DEVICE;
    }
    if (!nout) return NBG_OK;
  }

  if (cs.failed(res.reserve(stream, nout, plan.ncols), "result rows")) return cs.code(err);
  for (int c = 0; c < plan.ncols; ++c) a.out[c] = ws_row_col(res.w, c);
  a.cap = nout;
  tm.begin();
  const hipError_t he = launch_yr_emit(a, plan.nregs, ch.grid, stream);
  tm.end(YR_K_EMIT, (double)n * (a.keep ? 1.0 : 0.0) + (double)nout * 8.0 * (plan.yield_cols + plan.ncols));
  if (cs.failed(he, "k_yr_emit") || cs.failed(hipMemcpyAsync(&got, st, sizeof(YrState), hipMemcpyDeviceToHost, stream), "error word read") ||
      cs.failed(hipStreamSynchronize(stream), "emission"))
    return cs.code(err);
  if (got.err) {
    if (err) *err = "YIELD: an evaluation error in a YIELD column";
    return NBG_E_EXECUTION_ERROR;
  }
  *outw = res.release();
  *rows = nout;
  return NBG_OK;
}

}  // namespace nbg
