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
                          const FvPlan& plan, Workspace** outw, uint64_t* rows, FvProf* prof, std::string* err) {
  *outw = nullptr;
  *rows = 0;
  hipError_t he = hipSuccess;
  const char* what = "";
  auto failed = [&](hipError_t e, const char* w) {
    he = e;
    what = w;
    return e != hipSuccess;
  };
  auto code = [&]() -> int32_t {
    if (err) *err = std::string("FETCH: ") + what + ": " + hipGetErrorString(he);
    return he == hipErrorOutOfMemory ? NBG_E_OUT_OF_MEMORY : NBG_E_DEVICE;
  };
  const YrPlan& yp = plan.y;
  uint64_t n = 0;
  for (auto& sg : segs) n += sg.second;
  if (yp.ncols < 1 || yp.ncols > MAX_YIELDS || !n || n > 0xFFFFFFFFull || yp.code.size() + yp.data.size() > (size_t)MAX_PROGRAM ||
      yp.where_len != 0 || yp.where_reg >= 0 || plan.vid_col < 0 || plan.vid_col >= MAX_YIELDS || !plan.vids || !plan.tcols ||
      !plan.tpres || !plan.pres || plan.nv >= (uint64_t)NO_ROW) {
    if (err) *err = "FETCH: empty input or plan";
    return NBG_E_INVALID_ARGUMENT;
  }

  // the result: a workspace holding nothing but its rows (what the row accessors read)
  struct WsGuard {
    Workspace* w = nullptr;
    ~WsGuard() { if (w) ws_destroy(w); }
  } res, lit;
  auto new_rows = [&](WsGuard& g, uint64_t nrows, int ncols) {
    g.w = new Workspace();
    g.w->stream = stream;
    hipError_t e = hipMalloc((void**)&g.w->d_row_cols, MAX_YIELDS * sizeof(int64_t*));
    if (e == hipSuccess) e = ws_reserve_rows(g.w, nrows, ncols);
    if (e != hipSuccess) (void)hipGetLastError();
    return e;
  };
  if (!inw) {   // a literal vid list: a temporary one-column result on the same path
    if (!host_vids || segs.size() != 1 || segs[0].first != 0) {
      if (err) *err = "FETCH: no input";
      return NBG_E_INVALID_ARGUMENT;
    }
    if (failed(new_rows(lit, n, 1), "vid rows") ||
        failed(hipMemcpyAsync(ws_row_col(lit.w, 0), host_vids, n * 8, hipMemcpyHostToDevice, stream), "vid upload") ||
        failed(hipStreamSynchronize(stream), "vid upload"))
      return code();
    inw = lit.w;
  }

  StageScratch sc;   // (declared before the timer: the timer's events are resolved first)
  StageTimer<FvProf> tm{prof, stream, {}, nullptr};
  const std::vector<uint64_t> chunks = stage_chunks(segs, 0, n);
  const uint32_t nchunks = (uint32_t)(chunks.size() / 3);
  const unsigned grid = std::min<unsigned>(std::max<uint32_t>(nchunks, 1), STAGE_GRID);
  std::vector<Ins> image(yp.code);
  image.insert(image.end(), yp.data.begin(), yp.data.end());
  uint64_t* d_chunks = nullptr;
  Ins* d_prog = nullptr;
  YrState* st = nullptr;
  uint32_t* ccount = nullptr;
  uint32_t* cbase = nullptr;
  FvArgs f{};
  // (a pageable source is staged by the runtime before the call returns)
  if (failed(sc.alloc((void**)&d_chunks, chunks.size() * 8), "chunk list") ||
      failed(sc.alloc((void**)&d_prog, image.size() * sizeof(Ins)), "program") ||
      failed(sc.alloc((void**)&st, sizeof(YrState)), "state") || failed(sc.alloc((void**)&f.y.keep, n), "keep flags") ||
      failed(sc.alloc((void**)&f.dense, n * 4), "dense ids") || failed(sc.alloc((void**)&ccount, (size_t)nchunks * 4), "chunk counts") ||
      failed(sc.alloc((void**)&cbase, (size_t)nchunks * 4), "chunk bases") ||
      failed(hipMemcpyAsync(d_chunks, chunks.data(), chunks.size() * 8, hipMemcpyHostToDevice, stream), "chunk upload") ||
      (!image.empty() &&
       failed(hipMemcpyAsync(d_prog, image.data(), image.size() * sizeof(Ins), hipMemcpyHostToDevice, stream), "program upload")) ||
      failed(hipMemsetAsync(st, 0, sizeof(YrState), stream), "state clear") || failed(hipStreamSynchronize(stream), "uploads"))
    return code();

  YrArgs& a = f.y;
  a.chunk = d_chunks;
  a.nchunks = nchunks;
  a.cols = (const int64_t* const*)inw->d_row_cols;
  a.prog = d_prog;
  a.code_len = (int)yp.code.size();
  a.where_len = 0;
  a.where_reg = -1;
  a.ccount = ccount;
  a.cbase = cbase;
  a.err = &st->err;
  a.ncols = yp.ncols;
  for (int c = 0; c < yp.ncols; ++c) {
    a.yield_reg[c] = yp.yield_reg[c];
    a.yield_const[c] = yp.yield_const[c];
  }
  a.str = yp.str;
  a.now_sec = yp.now_sec;
  a.rand_seed = yp.rand_seed;
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
  he = launch_fv_resolve(f, grid, stream);
  tm.end(FV_K_RESOLVE, (double)n * (8.0 + 4.0 + 1.0));
  if (failed(he, "k_fv_resolve")) return code();
  he = launch_yr_scan(ccount, nchunks, cbase, st, stream);
  YrState got{};
  if (failed(he, "k_yr_scan") || failed(hipMemcpyAsync(&got, st, sizeof(YrState), hipMemcpyDeviceToHost, stream), "found rows read") ||
      failed(hipStreamSynchronize(stream), "join"))
    return code();
  const uint64_t nout = got.total;
  if (nout > n) {
    if (err) *err = "FETCH: " + std::to_string(nout) + " rows found of " + std::to_string(n);
    return NBG_E_DEVICE;
  }
  if (!nout) return NBG_OK;

  // ---- the YIELDs of the found rows
  if (failed(new_rows(res, nout, yp.ncols), "result rows")) return code();
  for (int c = 0; c < yp.ncols; ++c) a.out[c] = ws_row_col(res.w, c);
  a.cap = nout;
  tm.begin();
  he = launch_fv_emit(f, yp.nregs, grid, stream);
  tm.end(FV_K_EMIT, (double)n * 1.0 + (double)nout * (4.0 + 8.0 * (plan.tag_cols + yp.ncols)));
  if (failed(he, "k_fv_emit") || failed(hipMemcpyAsync(&got, st, sizeof(YrState), hipMemcpyDeviceToHost, stream), "error word read") ||
      failed(hipStreamSynchronize(stream), "emission"))
    return code();
  if (got.err) {
    if (err) *err = "FETCH: an evaluation error in a YIELD column";
    return NBG_E_EXECUTION_ERROR;
  }
  *outw = res.w;
  res.w = nullptr;
  *rows = nout;
  return NBG_OK;
}

}  // namespace nbg
