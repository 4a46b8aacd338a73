// The filtered adjacency of one (prepared GO statement, OVER type): the CSR rows restricted to the
// edges that pass the statement's WHERE `col <cmp> const`, built once so that the statement's
// final steps copy rows instead of re-reading the WHERE column and the failing edges' _dst on
// every execution (go.cpp go_launch substitutes it; the snapshot is immutable after finalize).
//   pos = exclusive scan of the pass flags (the flags are computed inside the scan's input
//         iterator and again by the scatter: no flag array), E + 1 entries, pos[E] = passing edges
//   rp'[v] = pos[row_ptr[v]]            (nv + 1 entries)
//   dst'[pos[j]] = dst_vid[j]           for passing j: the original order within each row
// The only temporaries are pos and the scan's scratch, released before returning.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <rocprim/rocprim.hpp>

#include "nbg_internal.h"

namespace nbg {
namespace {

constexpr int BT = 256;

unsigned grid_for(uint64_t n) {
  const uint64_t g = (n + BT - 1) / BT;
  return (unsigned)std::min<uint64_t>(std::max<uint64_t>(g, 1), 1u << 16);
}

#define GRID_STRIDE(i, n) \
  for (uint64_t i = (uint64_t)blockIdx.x * BT + threadIdx.x; i < (n); i += (uint64_t)gridDim.x * BT)

// pass = (lo <= x <= hi) != neg, as FastProg carries the WHERE; edge index n (one past the last)
// counts as failing, so a scan over n + 1 items ends with the number of passing edges
template <typename T>
struct Pass {
  const T* col;
  int64_t lo, hi;
  bool neg;
  uint64_t n;
  __device__ __forceinline__ uint32_t operator()(uint64_t j) const {
    if (j >= n) return 0u;
    const int64_t v = (int64_t)col[j];
    return (((v >= lo) & (v <= hi)) != neg) ? 1u : 0u;
  }
};

template <typename T>
__global__ void __launch_bounds__(BT) k_idx_scatter(Pass<T> pass, const uint32_t* __restrict__ pos,
                                                    const int64_t* __restrict__ dst, int64_t* __restrict__ out) {
  GRID_STRIDE(j, pass.n)
    if (pass(j)) out[pos[j]] = dst[j];
}

__global__ void __launch_bounds__(BT) k_idx_rows(const uint32_t* __restrict__ row_ptr, const uint32_t* __restrict__ pos,
                                                 uint32_t* __restrict__ rp, uint64_t nv) {
  GRID_STRIDE(v, nv + 1) rp[v] = pos[row_ptr[v]];
}

struct Temps {
  uint32_t* pos = nullptr;
  void* scan = nullptr;
  ~Temps() {
    if (pos) (void)hipFree(pos);
    if (scan) (void)hipFree(scan);
  }
};

template <typename T>
bool build_as(const StmtIndexSpec& sp, uint64_t budget, hipStream_t s, StmtIndex* out) {
  const uint64_t E = sp.edges, nv = sp.nv;
  const Pass<T> pass{static_cast<const T*>(sp.wcol), sp.lo, sp.hi, sp.where_neg != 0, E};
  auto flags = rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint64_t>(0), pass);
  size_t scan_bytes = 0;
  Temps t;
  if (rocprim::exclusive_scan(nullptr, scan_bytes, flags, t.pos, 0u, E + 1, rocprim::plus<uint32_t>(), s) != hipSuccess)
    return false;
  const uint64_t rp_bytes = (nv + 1) * 4, temp_bytes = (E + 1) * 4 + scan_bytes;
  if (rp_bytes + temp_bytes > budget) return false;
  StmtIndex ix;
  bool ok = hipMalloc((void**)&t.pos, (E + 1) * 4) == hipSuccess &&
            hipMalloc(&t.scan, std::max<size_t>(scan_bytes, 1)) == hipSuccess &&
            hipMalloc((void**)&ix.rp, rp_bytes) == hipSuccess;
  ok = ok && rocprim::exclusive_scan(t.scan, scan_bytes, flags, t.pos, 0u, E + 1, rocprim::plus<uint32_t>(), s) ==
                 hipSuccess;
  uint32_t total = 0;
  ok = ok && hipMemcpyAsync(&total, t.pos + E, 4, hipMemcpyDeviceToHost, s) == hipSuccess &&
       hipStreamSynchronize(s) == hipSuccess;
  // (at least one element: the final step reads element 0 for a tile without edges)
  const uint64_t dst_bytes = std::max<uint64_t>(total, 1) * 8;
  ok = ok && rp_bytes + dst_bytes + temp_bytes <= budget && hipMalloc((void**)&ix.dst, dst_bytes) == hipSuccess;
  if (ok) {
    if (!total) ok = hipMemsetAsync(ix.dst, 0, 8, s) == hipSuccess;
    hipLaunchKernelGGL(k_idx_rows, dim3(grid_for(nv + 1)), dim3(BT), 0, s, sp.row_ptr, t.pos, ix.rp, nv);
    if (total) hipLaunchKernelGGL(k_idx_scatter<T>, dim3(grid_for(E)), dim3(BT), 0, s, pass, t.pos, sp.dst_vid, ix.dst);
    ok = ok && hipGetLastError() == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
  }
  if (!ok) {
    (void)hipGetLastError();   // a failed allocation means "no index", never a query error
    stmtidx_free(&ix);
    return false;
  }
  ix.rows = total;
  ix.bytes = rp_bytes + dst_bytes;
  *out = ix;
  return true;
}

}  // namespace

void stmtidx_free(StmtIndex* ix) {
  if (ix->rp) (void)hipFree(ix->rp);
  if (ix->dst) (void)hipFree(ix->dst);
  *ix = StmtIndex{};
}

bool stmtidx_build(const StmtIndexSpec& sp, uint64_t budget_bytes, hipStream_t s, StmtIndex* out, double* ms) {
  *out = StmtIndex{};
  if (!sp.row_ptr || !sp.dst_vid || !sp.wcol || !sp.edges || sp.edges >= 0xFFFFFFFFull) return false;
  // ... and never above half of the free device memory (other statements, result rows)
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return false;
  const uint64_t budget = std::min<uint64_t>(budget_bytes, free_b / 2);
  if (hipStreamSynchronize(s) != hipSuccess) return false;
  const auto t0 = std::chrono::steady_clock::now();
  bool ok = false;
  switch (sp.wbytes) {
    case 1: ok = build_as<int8_t>(sp, budget, s, out); break;
    case 2: ok = build_as<int16_t>(sp, budget, s, out); break;
    case 4: ok = build_as<int32_t>(sp, budget, s, out); break;
    case 8: ok = build_as<int64_t>(sp, budget, s, out); break;
    default: break;
  }
  if (ms) *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return ok;
}

}  // namespace nbg
