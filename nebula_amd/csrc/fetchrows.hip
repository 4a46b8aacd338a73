// nebula_amd — piped FETCH PROP ON <tag> over a device-resident result (gfx950, wave64).
// FetchVerticesExecutor (src/graph/FetchVerticesExecutor.cpp:19-311) over the row segments earlier
// stages leave in HBM: the vid column is joined to the snapshot's dense vertex ids, and the YIELDs
// of the found rows are evaluated with the row's vertex as "the lane's vertex", so `tag.prop` is
// the interpreter's tag-column load (OP_TAGS_E).  The kernels sit beside the interpreter in
// kernels.hip (launch_fv_resolve, launch_fv_emit):
//   k_fv_resolve  per row: the vid cell searched in Snapshot::d_vids (sorted, signed), presence of
//                 the tag and visibility of the vertex; a dense id and a keep byte per logical row,
//                 one count per chunk
//   k_yr_scan     (yieldrows.hip, as it is) chunk counts into chunk bases and the total
//   k_fv_emit     the YIELDs of the found rows at chunk base + rank within the chunk, so the
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

const char* const kFvKernelNames[FV_KINDS] = {"k_fv_resolve", "k_fv_emit"};

int32_t ws_fetch_vertices(Workspace* inw, const int64_t* host_vids, hipStream_t stream, const std::vector<std::pair<uint64_t, uint64_t>>& segs,
                          const FvPlan& plan, Workspace** outw, uint64_t* rows, StageProf<FV_KINDS>* prof, std::string* err) {
  *outw = nullptr;
  *rows = 0;
  StageStatus cs("FETCH");
  const YrPlan& yp = plan.y;
  uint64_t n = 0;
  for (auto& sg : segs) n += sg.second;
  if (yp.ncols < 1 || yp.ncols > MAX_YIELDS || !n || n > 0xFFFFFFFFull || yp.code.size() + yp.data.size() > (size_t)MAX_PROGRAM ||
      yp.where_len != 0 || yp.where_reg >= 0 || plan.vid_col < 0 || plan.vid_col >= MAX_YIELDS || !plan.vids || !plan.tcols ||
      !plan.tpres || !plan.pres || plan.nv >= (uint64_t)NO_ROW) {
    if (err) *err = "FETCH: empty input or plan";
    return NBG_E_INVALID_ARGUMENT;
  }

  RowsWs res, lit;
  if (!inw) {   // a literal vid list: a temporary one-column result on the same path
    if (!host_vids || segs.size() != 1 || segs[0].first != 0) {
      if (err) *err = "FETCH: no input";
      return NBG_E_INVALID_ARGUMENT;
    }
    if (cs.failed(lit.reserve(stream, n, 1), "vid rows") ||
        cs.failed(hipMemcpyAsync(ws_row_col(lit.w, 0), host_vids, n * 8, hipMemcpyHostToDevice, stream), "vid upload") ||
        cs.failed(hipStreamSynchronize(stream), "vid upload"))
      return cs.code(err);
    inw = lit.w;
  }

  StageScratch sc;   // (declared before the timer: the timer's events are resolved first)
  StageTimer<FV_KINDS> tm{prof, stream, {}, nullptr};
  StageChunks ch;
  FvArgs f{};
  YrArgs& a = f.y;
  YrState* st = nullptr;
  uint32_t* ccount = nullptr;
  uint32_t* cbase = nullptr;
  if (ch.upload(cs, sc, stream, segs, 0, n) || cs.failed(sc.alloc((void**)&a.keep, n), "keep flags") ||
      cs.failed(sc.alloc((void**)&f.dense, n * 4), "dense ids") || cs.failed(sc.alloc((void**)&ccount, (size_t)ch.n * 4), "chunk counts") ||
      cs.failed(sc.alloc((void**)&cbase, (size_t)ch.n * 4), "chunk bases") || yr_setup(cs, sc, stream, yp, ch, inw, &a, &st))
    return cs.code(err);
  a.ccount = ccount;
  a.cbase = cbase;
  f.vid_col = plan.vid_col;
  f.vids = plan.vids;
  f.nv = plan.nv;
  f.pres = plan.pres;
  f.visible = plan.visible;
  f.tcols = plan.tcols;
  f.tpres = plan.tpres;
  // the plain search ships: the two-level form measured slower; it stays selectable
  // for the probe, from 2 * FV_PIVOTS vertices on (the pivots must be distinct entries)
  f.two_level = plan.search == 2 && plan.nv >= 2ull * FV_PIVOTS;

  // ---- the join, the ranks
  tm.begin();
  hipError_t he = launch_fv_resolve(f, ch.grid, stream);
  tm.end(FV_K_RESOLVE, (double)n * (8.0 + 4.0 + 1.0));
  if (cs.failed(he, "k_fv_resolve")) return cs.code(err);
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
  he = launch_fv_emit(f, yp.nregs, ch.grid, stream);
  tm.end(FV_K_EMIT, (double)n * 1.0 + (double)nout * (4.0 + 8.0 * (plan.tag_cols + yp.ncols)));
  if (cs.failed(he, "k_fv_emit") || cs.failed(hipMemcpyAsync(&got, st, sizeof(YrState), hipMemcpyDeviceToHost, stream), "error word read") ||
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
