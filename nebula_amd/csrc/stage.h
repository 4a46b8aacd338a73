// nebula_amd — what the stages over device-resident rows share (orderby.hip, setops.hip): the
// chunk list that spreads an input's segments over the device, the scratch of one call, and the
// event pairs nbg_profile puts around each launch.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "ws.h"

namespace nbg {

constexpr unsigned STAGE_GRID = 2048;   // 8 workgroups per CU; the chunks beyond are grid-strided

__device__ __forceinline__ uint32_t lane_rank(unsigned long long bal) {   // set bits below this lane
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
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
// Prof: { bool on; uint64_t launches[]; double ms[]; double bytes[]; }
template <class Prof>
struct StageTimer {
  Prof* prof;
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

}  // namespace nbg
