// nebula_amd — ORDER BY and LIMIT over a device-resident result (gfx950, wave64).
// OrderByExecutor (src/graph/OrderByExecutor.cpp:94-155) and LimitExecutor
// (src/graph/LimitExecutor.cpp:30-66) over the row segments a GO leaves in HBM (rows.hip).  Every
// factor becomes an order-preserving 64-bit image (ordimg.h; -0.0 folded into 0.0, complemented
// for DESC); a row's key is the tuple of its images.
//   full order        k_ob_iota      the rows' physical indices in segment order (the permutation)
//                     k_ob_image     one factor's images of the permutation's rows
//                     rocprim::radix_sort_pairs (image, row): stable, so LSD passes from the last
//                                    factor to the first leave the rows ordered by the whole tuple
//   first-K selection k_ob_hist      per digit (MSB first, 8 bits): LDS histogram of the first
//                                    factor's images matching the prefix so far, flushed with one
//                                    atomic per non-empty bin
//                     k_ob_pick      one workgroup: the digit holding the K-th smallest image
//                     k_ob_compact   rows at or below the K-th image -> the candidates: each wave
//                                    places its rows by ballot / mbcnt, the slots of a whole
//                                    chunk reserved with one atomic; they go through the full
//                                    order above
//   result            k_ob_gather    output row j <- input row perm[lo + j], every column
//   LIMIT only        k_ob_copy      the segment slices covering the window
// No kernel waits on another workgroup: every dependency is a kernel boundary on one stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <rocprim/rocprim.hpp>
#include <string>
#include <vector>

#include "ordimg.h"
#include "stage.h"
#include "ws.h"

namespace nbg {

const char* const kObKernelNames[OB_KINDS] = {"k_ob_iota", "k_ob_hist", "k_ob_pick", "k_ob_compact",
                                              "k_ob_image", "ob_radix_sort", "k_ob_gather", "k_ob_copy"};

namespace {

constexpr uint32_t OB_DBL = 1u, OB_DESC = 2u;
constexpr unsigned OB_GRID = STAGE_GRID;

// a factor cell's sort image
__device__ __forceinline__ uint64_t ob_image(int64_t v, uint32_t flags) {
  uint64_t u = (uint64_t)v;
  if ((flags & OB_DBL) && u == SIGN64) u = 0;   // -0.0 == 0.0 (ColumnValue::operator==)
  u = ord_image(u, (uint8_t)(flags & OB_DBL));
  return (flags & OB_DESC) ? ~u : u;
}

__device__ __forceinline__ uint32_t ob_lane_rank(unsigned long long bal) { return lane_rank(bal); }

// the selection's state: one copy in HBM, advanced by k_ob_pick between the histogram passes
struct ObSel {
  unsigned long long prefix;      // the digits chosen so far (the K-th image when all 8 are)
  unsigned long long k;           // rank of the K-th image among the rows matching the prefix
  unsigned long long below;       // rows whose image is below every image matching the prefix
  unsigned long long equal;       // rows matching the prefix
  unsigned long long ncand;       // k_ob_compact's slot counter
  unsigned long long hist[256];
};

// chunk[3k..3k+2] = (first physical row, rows (<= OB_CHUNK), logical index of the first row)
__global__ void __launch_bounds__(BLOCK) k_ob_iota(const uint64_t* __restrict__ chunk, uint32_t nchunks,
                                                   uint64_t* __restrict__ perm) {
  for (uint32_t k = blockIdx.x; k < nchunks; k += gridDim.x) {
    const uint64_t b = chunk[3 * k], len = chunk[3 * k + 1], lo = chunk[3 * k + 2];
    for (uint64_t i = threadIdx.x; i < len; i += BLOCK) perm[lo + i] = b + i;
  }
}

__global__ void __launch_bounds__(BLOCK) k_ob_hist(const uint64_t* __restrict__ chunk, uint32_t nchunks,
                                                   const int64_t* __restrict__ col, uint32_t flags, int shift,
                                                   ObSel* __restrict__ st) {
  __shared__ unsigned int lh[256];
  static_assert(BLOCK == 256, "one bin per thread");
  const int lane = threadIdx.x & 63;
  lh[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t prefix = st->prefix;
  const uint64_t hmask = shift >= 56 ? 0ull : ~0ull << (shift + 8);   // the digits above this one
  for (uint32_t k = blockIdx.x; k < nchunks; k += gridDim.x) {
    const uint64_t b = chunk[3 * k], len = chunk[3 * k + 1];
    for (uint64_t c0 = 0; c0 < len; c0 += BLOCK) {
      const uint64_t i = c0 + threadIdx.x;
      const bool valid = i < len;
      const uint64_t img = valid ? ob_image(col[b + i], flags) : 0ull;
      const bool match = valid && ((img ^ prefix) & hmask) == 0;
      const uint32_t digit = (uint32_t)(img >> shift) & 255u;
      // a wave whose matching rows share one digit (a tied factor, the upper digits of small
      // values) adds once; lanes on one LDS address would otherwise serialise
      const unsigned long long bal = __ballot(match);
      if (bal) {
        const int leader = __ffsll(bal) - 1;
        const uint32_t ld = (uint32_t)__shfl((int)digit, leader);
        if (__ballot(match && digit == ld) == bal) {
          if (lane == leader) atomicAdd(&lh[ld], (unsigned int)__popcll(bal));
        } else if (match) {
          atomicAdd(&lh[digit], 1u);
        }
      }
    }
  }
  __syncthreads();
  const unsigned int mine = lh[threadIdx.x];
  if (mine) atomicAdd(&st->hist[threadIdx.x], (unsigned long long)mine);
}

// one workgroup: the digit whose bin holds rank k, then the histogram cleared for the next pass
__global__ void __launch_bounds__(256) k_ob_pick(ObSel* __restrict__ st, int shift) {
  __shared__ unsigned long long h[256];
  h[threadIdx.x] = st->hist[threadIdx.x];
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long k = st->k;
    unsigned long long cum = 0;
    int d = 0;
    for (; d < 255; ++d) {
      if (k < cum + h[d]) break;
      cum += h[d];
    }
    st->prefix |= (unsigned long long)d << shift;
    st->k = k - cum;
    st->below += cum;
    st->equal = h[d];
  }
  st->hist[threadIdx.x] = 0;
}

__global__ void __launch_bounds__(BLOCK) k_ob_compact(const uint64_t* __restrict__ chunk, uint32_t nchunks,
                                                      const int64_t* __restrict__ col, uint32_t flags,
                                                      ObSel* __restrict__ st, uint64_t* __restrict__ cand,
                                                      uint64_t cap) {
  // Two walks over a chunk (the second one hits the cache): the waves' ballot counts per step,
  // one reservation for the whole chunk — a counter every wave adds to would serialise the pass
  // when many rows tie at the K-th image — then each wave's rows at its offset, in row order.
  constexpr int STEPS = (int)(OB_CHUNK / BLOCK);
  __shared__ uint32_t woff[STEPS * WAVES];
  __shared__ unsigned long long sbase;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t kth = st->prefix;
  for (uint32_t k = blockIdx.x; k < nchunks; k += gridDim.x) {
    const uint64_t b = chunk[3 * k], len = chunk[3 * k + 1];   // len <= OB_CHUNK
    const int steps = (int)((len < OB_CHUNK ? len : OB_CHUNK) + BLOCK - 1) / BLOCK;   // <= STEPS
    for (int s = 0; s < steps; ++s) {
      const uint64_t i = (uint64_t)s * BLOCK + threadIdx.x;
      const bool take = i < len && ob_image(col[b + (i < len ? i : 0)], flags) <= kth;
      const unsigned long long bal = __ballot(take);
      if (lane == 0) woff[s * WAVES + wave] = (uint32_t)__popcll(bal);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t total = 0;
      for (int j = 0; j < steps * WAVES; ++j) {
        const uint32_t c = woff[j];
        woff[j] = total;
        total += c;
      }
      sbase = total ? atomicAdd(&st->ncand, (unsigned long long)total) : 0ull;
    }
    __syncthreads();
    const uint64_t base = sbase;
    for (int s = 0; s < steps; ++s) {
      const uint64_t i = (uint64_t)s * BLOCK + threadIdx.x;
      const bool take = i < len && ob_image(col[b + (i < len ? i : 0)], flags) <= kth;
      const unsigned long long bal = __ballot(take);
      const uint64_t slot = base + woff[s * WAVES + wave] + ob_lane_rank(bal);
      if (take && slot < cap) cand[slot] = b + i;
    }
    __syncthreads();   // (woff and sbase are rewritten for the next chunk)
  }
}

__global__ void __launch_bounds__(BLOCK) k_ob_image(const uint64_t* __restrict__ perm, uint64_t n,
                                                    const int64_t* __restrict__ col, uint32_t flags,
                                                    uint64_t* __restrict__ keys) {
  for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BLOCK)
    keys[i] = ob_image(col[perm[i]], flags);
}

__global__ void __launch_bounds__(BLOCK) k_ob_gather(const uint64_t* __restrict__ perm, uint64_t n,
                                                     int64_t* const* __restrict__ cols, int ncols,
                                                     int64_t* const* __restrict__ ocols) {
  for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BLOCK) {
    const uint64_t row = perm[i];
    for (int c = 0; c < ncols; ++c) ocols[c][i] = cols[c][row];
  }
}

__global__ void __launch_bounds__(BLOCK) k_ob_copy(const uint64_t* __restrict__ chunk, uint32_t nchunks,
                                                   int64_t* const* __restrict__ cols, int ncols,
                                                   int64_t* const* __restrict__ ocols) {
  for (uint32_t k = blockIdx.x; k < nchunks; k += gridDim.x) {
    const uint64_t b = chunk[3 * k], len = chunk[3 * k + 1], lo = chunk[3 * k + 2];
    for (int c = 0; c < ncols; ++c) {
      const int64_t* __restrict__ src = cols[c] + b;
      int64_t* __restrict__ dst = ocols[c] + lo;
      for (uint64_t i = threadIdx.x; i < len; i += BLOCK) dst[i] = src[i];
    }
  }
}

unsigned ob_flat_grid(uint64_t n) { return (unsigned)std::min<uint64_t>(std::max<uint64_t>(cdiv(n, BLOCK), 1), OB_GRID); }

}  // namespace

int32_t ws_order_by(Workspace* inw, hipStream_t stream, const std::vector<std::pair<uint64_t, uint64_t>>& segs,
                    const ObPlan& plan, Workspace** outw, StageProf<OB_KINDS>* prof, std::string* err) {
  *outw = nullptr;
  StageStatus cs("order by");
  uint64_t total = 0;
  for (auto& sg : segs) total += sg.second;
  if (plan.lo >= plan.hi || plan.hi > total || plan.nf < 0 || plan.nf > MAX_YIELDS || plan.ncols < 1 ||
      plan.ncols > MAX_YIELDS) {
    if (err) *err = "order by: empty window or plan";
    return NBG_E_INVALID_ARGUMENT;
  }
  const uint64_t nout = plan.hi - plan.lo;
  int64_t* const* cols = inw->d_row_cols;

  RowsWs res;
  if (cs.failed(res.reserve(stream, nout, plan.ncols), "result rows")) return cs.code(err);
  int64_t* const* ocols = (int64_t* const*)res.w->d_row_cols;

  StageScratch sc;      // (declared before the timer: the timer's events are resolved first)
  StageTimer<OB_KINDS> tm{prof, stream, {}, nullptr};
  // the chunks the kernels walk: the window's slices (LIMIT only), else every row
  StageChunks ch;
  if (ch.upload(cs, sc, stream, segs, plan.nf ? 0 : plan.lo, plan.nf ? total : plan.hi)) return cs.code(err);

  if (!plan.nf) {
    tm.begin();
    hipLaunchKernelGGL(k_ob_copy, dim3(ch.grid), dim3(BLOCK), 0, stream, ch.dev, ch.n, cols, plan.ncols, ocols);
    tm.end(OB_K_COPY, (double)nout * plan.ncols * 16.0);
    if (cs.failed(hipGetLastError(), "k_ob_copy") || cs.failed(hipStreamSynchronize(stream), "copy")) return cs.code(err);
    *outw = res.w;
    res.w = nullptr;
    return NBG_OK;
  }

  auto flags_of = [&](int f) { return (plan.dbl[f] ? OB_DBL : 0u) | (plan.desc[f] ? OB_DESC : 0u); };
  std::vector<const int64_t*> hcols(plan.ncols);   // the columns' bases (the kernels here read one column each)
  if (cs.failed(hipMemcpyAsync(hcols.data(), cols, plan.ncols * sizeof(int64_t*), hipMemcpyDeviceToHost, stream), "column bases") ||
      cs.failed(hipStreamSynchronize(stream), "column bases"))
    return cs.code(err);
  // ---- the rows to sort: every row, or the candidates of the first-K selection
  uint64_t n = total;
  uint64_t* rows_a = nullptr;
  const bool select = plan.has_limit && plan.hi <= total / OB_SELECT_RATIO;
  if (select) {
    const int64_t* col0 = hcols[plan.col[0]];
    ObSel* st = nullptr;
    ObSel init{};
    init.k = plan.hi - 1;   // the K-th smallest image, 0-based
    if (cs.failed(sc.alloc((void**)&st, sizeof(ObSel)), "selection state") ||
        cs.failed(hipMemcpyAsync(st, &init, sizeof(ObSel), hipMemcpyHostToDevice, stream), "selection state upload"))
      return cs.code(err);
    for (int shift = 56; shift >= 0; shift -= 8) {
      tm.begin();
      hipLaunchKernelGGL(k_ob_hist, dim3(ch.grid), dim3(BLOCK), 0, stream, ch.dev, ch.n, col0, flags_of(0), shift, st);
      tm.end(OB_K_HIST, (double)total * 8.0);
      if (cs.failed(hipGetLastError(), "k_ob_hist")) return cs.code(err);
      tm.begin();
      hipLaunchKernelGGL(k_ob_pick, dim3(1), dim3(256), 0, stream, st, shift);
      tm.end(OB_K_PICK, 256.0 * 16.0);
      if (cs.failed(hipGetLastError(), "k_ob_pick")) return cs.code(err);
    }
    ObSel got{};
    if (cs.failed(hipMemcpyAsync(&got, st, sizeof(ObSel), hipMemcpyDeviceToHost, stream), "selection read") ||
        cs.failed(hipStreamSynchronize(stream), "selection"))
      return cs.code(err);
    n = got.below + got.equal;   // every row at or below the K-th image
    if (n < plan.hi || n > total || got.k >= got.equal) {
      if (err) *err = "order by: the selection counted " + std::to_string(n) + " candidates for K = " + std::to_string(plan.hi);
      return NBG_E_DEVICE;
    }
    if (cs.failed(sc.alloc((void**)&rows_a, n * 8), "candidates")) return cs.code(err);
    tm.begin();
    hipLaunchKernelGGL(k_ob_compact, dim3(ch.grid), dim3(BLOCK), 0, stream, ch.dev, ch.n, col0, flags_of(0), st, rows_a, n);
    tm.end(OB_K_COMPACT, (double)total * 8.0 + (double)n * 8.0);
    unsigned long long ncand = 0;
    if (cs.failed(hipGetLastError(), "k_ob_compact") ||
        cs.failed(hipMemcpyAsync(&ncand, &st->ncand, 8, hipMemcpyDeviceToHost, stream), "candidate count") ||
        cs.failed(hipStreamSynchronize(stream), "compaction"))
      return cs.code(err);
    if (ncand != n) {
      if (err) *err = "order by: " + std::to_string(ncand) + " candidates compacted, " + std::to_string(n) + " counted";
      return NBG_E_DEVICE;
    }
  } else {
    if (cs.failed(sc.alloc((void**)&rows_a, n * 8), "permutation")) return cs.code(err);
    tm.begin();
    hipLaunchKernelGGL(k_ob_iota, dim3(ch.grid), dim3(BLOCK), 0, stream, ch.dev, ch.n, rows_a);
    tm.end(OB_K_IOTA, (double)n * 8.0);
    if (cs.failed(hipGetLastError(), "k_ob_iota")) return cs.code(err);
  }

  // ---- stable LSD passes over the factors, last first
  uint64_t *rows_b = nullptr, *keys_a = nullptr, *keys_b = nullptr;
  void* tmp = nullptr;
  if (cs.failed(sc.alloc((void**)&rows_b, n * 8), "permutation buffer") ||
      cs.failed(sc.alloc((void**)&keys_a, n * 8), "sort keys") || cs.failed(sc.alloc((void**)&keys_b, n * 8), "sort keys"))
    return cs.code(err);
  rocprim::double_buffer<uint64_t> keys(keys_a, keys_b), perm(rows_a, rows_b);
  size_t tmp_bytes = 0;
  if (cs.failed(rocprim::radix_sort_pairs(nullptr, tmp_bytes, keys, perm, (size_t)n, 0u, 64u, stream), "sort sizing") ||
      cs.failed(sc.alloc(&tmp, tmp_bytes), "sort scratch"))
    return cs.code(err);
  for (int f = plan.nf - 1; f >= 0; --f) {
    tm.begin();
    hipLaunchKernelGGL(k_ob_image, dim3(ob_flat_grid(n)), dim3(BLOCK), 0, stream, perm.current(), n, hcols[plan.col[f]],
                       flags_of(f), keys.current());
    tm.end(OB_K_IMAGE, (double)n * 24.0);
    if (cs.failed(hipGetLastError(), "k_ob_image")) return cs.code(err);
    tm.begin();
    const hipError_t se = rocprim::radix_sort_pairs(tmp, tmp_bytes, keys, perm, (size_t)n, 0u, 64u, stream);
    tm.end(OB_K_SORT, (double)n * 32.0);
    if (cs.failed(se, "radix_sort_pairs")) return cs.code(err);
  }
  tm.begin();
  hipLaunchKernelGGL(k_ob_gather, dim3(ob_flat_grid(nout)), dim3(BLOCK), 0, stream, perm.current() + plan.lo, nout, cols,
                     plan.ncols, ocols);
  tm.end(OB_K_GATHER, (double)nout * (8.0 + plan.ncols * 16.0));
  if (cs.failed(hipGetLastError(), "k_ob_gather") || cs.failed(hipStreamSynchronize(stream), "ordering")) return cs.code(err);
  *outw = res.release();
  return NBG_OK;
}

}  // namespace nbg
