// nebula_amd — piped FETCH PROP ON <edge> over a device-resident result (gfx950, wave64).
// FetchEdgesExecutor (src/graph/FetchEdgesExecutor.cpp:17-384) over the row segments earlier
// stages leave in HBM: the (src, dst[, rank]) columns are joined to the edges of the type's
// out-CSR, and the YIELDs of the found rows are evaluated with the found edge as "the lane's
// edge", so `edge.prop`, `_dst`, `_src` and `_rank` are the interpreter's per-edge loads.  The
// kernels sit beside the interpreter in kernels.hip (launch_fe_resolve, launch_fe_emit):
//   k_fe_resolve  per row: the src cell searched in Snapshot::d_vids (sorted, signed) and checked
//                 for visibility, then (rank, dst) searched in the source's CSR row (sorted in the
//                 key's byte order); an edge index, the source's dense id where _src is read and
//                 a keep byte per logical row, one count per chunk
//   k_yr_scan     (yieldrows.hip, as it is) chunk counts into chunk bases and the total
//   k_fe_emit     the YIELDs of the found rows at chunk base + rank within the chunk, so the
//                 result keeps the input's fetch order
// The input is walked through the chunk list of stage.h, one workgroup per chunk.  No kernel waits
// on another workgroup: every dependency is a kernel boundary on one stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "stage.h"
#include "ws.h"

namespace nbg {

const char* const kFeKernelNames[FE_KINDS] = {"k_fe_resolve", "k_fe_emit"};

int32_t ws_fetch_edges(Workspace* inw, const int64_t* host_src, const int64_t* host_dst, const int64_t* host_rank,
                       hipStream_t stream, const std::vector<std::pair<uint64_t, uint64_t>>& segs, const FePlan& plan,
                       Workspace** outw, uint64_t* rows, StageProf<FE_KINDS>* prof, std::string* err) {
  *outw = nullptr;
  *rows = 0;
  StageStatus cs("FETCH");
  const YrPlan& yp = plan.y;
  uint64_t n = 0;
  for (auto& sg : segs) n += sg.second;
  auto col_ok = [](int c) { return c >= 0 && c < MAX_YIELDS; };
  if (yp.ncols < 1 || yp.ncols > MAX_YIELDS || !n || n > 0xFFFFFFFFull || yp.code.size() + yp.data.size() > (size_t)MAX_PROGRAM ||
      yp.where_len != 0 || yp.where_reg >= 0 || !col_ok(plan.src_col) || !col_ok(plan.dst_col) ||
      (plan.rank_col != -1 && !col_ok(plan.rank_col)) || !plan.vids || !plan.row_ptr || !plan.dst_vid || !plan.props ||
      plan.nv >= (uint64_t)NO_ROW) {
    if (err) *err = "FETCH: empty input or plan";
    return NBG_E_INVALID_ARGUMENT;
  }

  RowsWs res, lit;
  if (!inw) {   // literal keys: a temporary three-column result (src, dst, rank) on the same path
    if (!host_src || !host_dst || segs.size() != 1 || segs[0].first != 0 || plan.src_col != 0 || plan.dst_col != 1 ||
        plan.rank_col != 2) {
      if (err) *err = "FETCH: no input";
      return NBG_E_INVALID_ARGUMENT;
    }
    if (cs.failed(lit.reserve(stream, n, 3), "key rows") ||
        cs.failed(hipMemcpyAsync(ws_row_col(lit.w, 0), host_src, n * 8, hipMemcpyHostToDevice, stream), "src upload") ||
        cs.failed(hipMemcpyAsync(ws_row_col(lit.w, 1), host_dst, n * 8, hipMemcpyHostToDevice, stream), "dst upload") ||
        cs.failed(host_rank ? hipMemcpyAsync(ws_row_col(lit.w, 2), host_rank, n * 8, hipMemcpyHostToDevice, stream)
                            : hipMemsetAsync(ws_row_col(lit.w, 2), 0, n * 8, stream),
                  "rank upload") ||
        cs.failed(hipStreamSynchronize(stream), "key upload"))
      return cs.code(err);
    inw = lit.w;
  }

  StageScratch sc;   // (declared before the timer: the timer's events are resolved first)
  StageTimer<FE_KINDS> tm{prof, stream, {}, nullptr};
  StageChunks ch;
  FeArgs f{};
  YrArgs& a = f.y;
  YrState* st = nullptr;
  uint32_t* ccount = nullptr;
  uint32_t* cbase = nullptr;
  if (ch.upload(cs, sc, stream, segs, 0, n) || cs.failed(sc.alloc((void**)&a.keep, n), "keep flags") ||
      cs.failed(sc.alloc((void**)&f.eidx, n * 4), "edge indices") ||
      (plan.need_src && cs.failed(sc.alloc((void**)&f.dense, n * 4), "dense ids")) ||
      cs.failed(sc.alloc((void**)&ccount, (size_t)ch.n * 4), "chunk counts") ||
      cs.failed(sc.alloc((void**)&cbase, (size_t)ch.n * 4), "chunk bases") || yr_setup(cs, sc, stream, yp, ch, inw, &a, &st))
    return cs.code(err);
  a.ccount = ccount;
  a.cbase = cbase;
  f.src_col = plan.src_col;
  f.dst_col = plan.dst_col;
  f.rank_col = plan.rank_col;
  f.vids = plan.vids;
  f.nv = plan.nv;
  f.visible = plan.visible;
  f.row_ptr = plan.row_ptr;
  f.dst_vid = plan.dst_vid;
  f.rank = plan.rank;
  f.valid = plan.valid;
  f.props = plan.props;
  const double key_cells = plan.rank_col >= 0 ? 3.0 : 2.0, idx_bytes = plan.need_src ? 8.0 : 4.0;

  // ---- the join, the ranks
  tm.begin();
  hipError_t he = launch_fe_resolve(f, ch.grid, stream);
  tm.end(FE_K_RESOLVE, (double)n * (8.0 * key_cells + idx_bytes + 1.0));
  if (cs.failed(he, "k_fe_resolve")) return cs.code(err);
  he = launch_yr_scan(ccount, ch.n, cbase, st, stream);
  YrState got{};
  if (cs.failed(he, "k_yr_scan") || cs.failed(hipMemcpyAsync(&got, st, sizeof(YrState), hipMemcpyDeviceToHost, stream), "found rows read") ||
      cs.failed(hipStreamSynchronize(stream), "join"))
    return cs.code(err);
  const uint64_t nout = got.total;
  if (nout > n) {
    if (err) *err = "FETCH: " + std::to_string(nout) + " rows found of " + std::to_string(n);
    return NBG_E_DEVICE;
  }
  if (!nout) return NBG_OK;

  // ---- the YIELDs of the found rows
  if (cs.failed(res.reserve(stream, nout, yp.ncols), "result rows")) return cs.code(err);
  for (int c = 0; c < yp.ncols; ++c) a.out[c] = ws_row_col(res.w, c);
  a.cap = nout;
  tm.begin();
  he = launch_fe_emit(f, yp.nregs, ch.grid, stream);
  tm.end(FE_K_EMIT, (double)n * 1.0 + (double)nout * (idx_bytes + 8.0 * (plan.prop_cols + yp.ncols)));
  if (cs.failed(he, "k_fe_emit") || cs.failed(hipMemcpyAsync(&got, st, sizeof(YrState), hipMemcpyDeviceToHost, stream), "error word read") ||
      cs.failed(hipStreamSynchronize(stream), "emission"))
    return cs.code(err);
  if (got.err) {
    if (err) *err = "FETCH: an evaluation error in a YIELD column";
    return NBG_E_EXECUTION_ERROR;
  }
  *outw = res.release();
  *rows = nout;
  return NBG_OK;
}

}  // namespace nbg
