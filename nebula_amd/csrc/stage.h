// nebula_amd — the frame of a driver of a stage over device-resident rows (groupby.hip, orderby.hip,
// setops.hip, yieldrows.hip, yieldagg.hip, fetchrows.hip, fetchedges.hip, gopipe.hip, rowenc.hip, rowdec.hip): the status of its HIP calls, its result workspace
// (RowsWs, nbg_internal.h), the scratch of one call, the event pairs nbg_profile puts around each
// launch, the chunk list that spreads an input's segments over the device, and the YrPlan setup
// YIELD and FETCH share.  A driver declares its scratch before its timer: the timer's events are
// resolved first.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "ws.h"

namespace nbg {

constexpr unsigned STAGE_GRID = 2048;   // 8 workgroups per CU; the chunks beyond are grid-strided

__device__ __forceinline__ uint32_t lane_rank(unsigned long long bal) {   // set bits below this lane
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
}

// the vid -> dense id join (k_fv_resolve, k_fe_resolve, k_gp_resolve): the first entry of
// vids[lo, hi) not below `vid` (signed order)
__device__ __forceinline__ uint64_t fv_lower_bound(const int64_t* __restrict__ vids, uint64_t lo, uint64_t hi, int64_t vid) {
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (vids[mid] < vid) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// what a driver's HIP calls came to: `failed` records and tests one, `code` reports the last
struct StageStatus {
  const char* prefix;   // "order by", "YIELD", ...: what the message opens with
  hipError_t he = hipSuccess;
  const char* what = "";
  explicit StageStatus(const char* p) : prefix(p) {}
  bool failed(hipError_t e, const char* w) {
    he = e;
    what = w;
    return e != hipSuccess;
  }
  int32_t code(std::string* err) const {
    if (err) *err = std::string(prefix) + ": " + what + ": " + hipGetErrorString(he);
    return he == hipErrorOutOfMemory ? NBG_E_OUT_OF_MEMORY : NBG_E_DEVICE;
  }
};

// the result: a workspace holding nothing but its rows (what the row accessors read)
inline hipError_t RowsWs::reserve(hipStream_t stream, uint64_t rows, int ncols) {
  w = new Workspace();
  w->stream = stream;
  hipError_t e = hipMalloc((void**)&w->d_row_cols, MAX_YIELDS * sizeof(int64_t*));
  if (e == hipSuccess) e = ws_reserve_rows(w, rows, ncols);
  if (e != hipSuccess) (void)hipGetLastError();
  return e;
}

// scratch of one call, released when it returns
struct StageScratch {
  std::vector<void*> ptrs;
  hipError_t alloc(void** p, size_t bytes) {
    *p = nullptr;
    const hipError_t e = hipMalloc(p, bytes ? bytes : 8);
    if (e == hipSuccess) ptrs.push_back(*p);
    else (void)hipGetLastError();
    return e;
  }
  ~StageScratch() {
    for (void* p : ptrs) (void)hipFree(p);
  }
};

// an event pair around each launch while nbg_profile is on, resolved after the call's last wait;
// a StageProf of the stage's kinds
template <int KINDS>
struct StageTimer {
  StageProf<KINDS>* prof;
  hipStream_t stream;
  struct Rec { int kind; hipEvent_t a, b; double bytes; };
  std::vector<Rec> recs;
  hipEvent_t open = nullptr;
  bool on() const { return prof && prof->on; }
  void begin() {
    if (!on()) return;
    if (hipEventCreate(&open) != hipSuccess) { open = nullptr; return; }
    (void)hipEventRecord(open, stream);
  }
  void end(int kind, double bytes) {
    if (!open) return;
    hipEvent_t b = nullptr;
    if (hipEventCreate(&b) == hipSuccess) {
      (void)hipEventRecord(b, stream);
      recs.push_back({kind, open, b, bytes});
    } else {
      (void)hipEventDestroy(open);
    }
    open = nullptr;
  }
  ~StageTimer() {
    for (auto& r : recs) {
      float ms = 0.f;
      if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
        prof->launches[r.kind]++;
        prof->ms[r.kind] += ms;
        prof->bytes[r.kind] += r.bytes;
      }
      (void)hipEventDestroy(r.a);
      (void)hipEventDestroy(r.b);
    }
    if (open) (void)hipEventDestroy(open);
  }
};

// the rows of `segs` inside logical rows [lo, hi), cut into chunks of at most OB_CHUNK rows:
// chunk[3k..3k+2] = (first physical row, rows, the first row's logical index minus lo)
inline std::vector<uint64_t> stage_chunks(const std::vector<std::pair<uint64_t, uint64_t>>& segs, uint64_t lo,
                                          uint64_t hi) {
  std::vector<uint64_t> out;
  uint64_t at = 0;
  for (auto& sg : segs) {
    const uint64_t s0 = std::max(at, lo), s1 = std::min(at + sg.second, hi);
    for (uint64_t p = s0; p < s1; p += OB_CHUNK)
      out.insert(out.end(), {sg.first + (p - at), std::min<uint64_t>(OB_CHUNK, s1 - p), p - lo});
    at += sg.second;
  }
  return out;
}

// stage_chunks on the device.  The host copy lives as long as the object, so the upload needs no
// wait of its own.
struct StageChunks {
  std::vector<uint64_t> host;
  uint64_t* dev = nullptr;
  uint32_t n = 0;
  unsigned grid = 1;   // one workgroup per chunk, at most STAGE_GRID
  bool upload(StageStatus& st, StageScratch& sc, hipStream_t stream,
              const std::vector<std::pair<uint64_t, uint64_t>>& segs, uint64_t lo, uint64_t hi) {
    host = stage_chunks(segs, lo, hi);
    n = (uint32_t)(host.size() / 3);
    grid = std::min<unsigned>(std::max<uint32_t>(n, 1), STAGE_GRID);
    return st.failed(sc.alloc((void**)&dev, host.size() * 8), "chunk list") ||
           st.failed(hipMemcpyAsync(dev, host.data(), host.size() * 8, hipMemcpyHostToDevice, stream), "chunk upload");
  }
};

// What YIELD and FETCH make of a YrPlan before their first launch: the program image on the device
// (code, then data), a cleared YrState, and the members of YrArgs the plan, the chunks and the
// input decide.  Waits for the uploads (the image is a local).
inline bool yr_setup(StageStatus& st, StageScratch& sc, hipStream_t stream, const YrPlan& plan, const StageChunks& ch,
                     const Workspace* inw, YrArgs* a, YrState** state) {
  std::vector<Ins> image(plan.code);
  image.insert(image.end(), plan.data.begin(), plan.data.end());
  Ins* d_prog = nullptr;
  if (st.failed(sc.alloc((void**)&d_prog, image.size() * sizeof(Ins)), "program") ||
      st.failed(sc.alloc((void**)state, sizeof(YrState)), "state") ||
      (!image.empty() &&
       st.failed(hipMemcpyAsync(d_prog, image.data(), image.size() * sizeof(Ins), hipMemcpyHostToDevice, stream), "program upload")) ||
      st.failed(hipMemsetAsync(*state, 0, sizeof(YrState), stream), "state clear") ||
      st.failed(hipStreamSynchronize(stream), "uploads"))
    return true;
  a->chunk = ch.dev;
  a->nchunks = ch.n;
  a->cols = (const int64_t* const*)inw->d_row_cols;
  a->prog = d_prog;
  a->code_len = (int)plan.code.size();
  a->where_len = plan.where_len;
  a->where_reg = plan.where_reg;
  a->err = &(*state)->err;
  a->ncols = plan.ncols;
  for (int c = 0; c < plan.ncols; ++c) {
    a->yield_reg[c] = plan.yield_reg[c];
    a->yield_const[c] = plan.yield_const[c];
  }
  a->str = plan.str;
  a->now_sec = plan.now_sec;
  a->rand_seed = plan.rand_seed;
  return false;
}

}  // namespace nbg
