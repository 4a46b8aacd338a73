// nebula_amd — GO FROM $-.col / $var.col over a device-resident result (gfx950, wave64).
// GoExecutor::setupStarts (src/graph/GoExecutor.cpp:365-399) with InterimResult::getVIDs and
// buildIndex (src/graph/InterimResult.cpp:29-72, :158-250) over the row segments earlier stages leave
// in HBM: the start list and the $- / $var input index are built where the rows lie and handed to
// the hop kernels as they are (go.cpp drives this file between go_prepare and go_launch).
//   k_gp_resolve  per row: the FROM cell searched in Snapshot::d_vids (k_fv_resolve's search); a dense
//                 id per logical row (NO_ROW: no vertex), one count per chunk, and — when the
//                 statement is DISTINCT or reads $- / $var — atomicMax(last_row[dense], row + 1)
//                 into a zeroed table of nv 32-bit entries
//   k_gp_table    per block of GP_TBLOCK table entries: the non-zero ones counted; under DISTINCT
//                 their capped degrees summed per OVER type
//   k_yr_scan     (yieldrows.hip, as it is) chunk counts and table-block counts into bases and totals
//   k_gp_degrees  without DISTINCT: the found rows' capped degrees summed per OVER type
//   --- one read-back: found rows, unique vertices, the per-type sums (GpCounts) ---
//   k_gp_emit     the found rows' dense ids at chunk base + rank: the start list in fetch order
//   k_gp_compact  the table's non-zero entries at block base + rank: the DISTINCT start list
//                 (ascending dense id) and / or the input index — in_ids = the vid, in_cols[c] = the
//                 cell of the winning logical row, found through the chunk list
// The table gives "the last row of a vid wins" (the largest logical row + 1 survives) and, read in
// ascending dense id, keys that are already sorted by vid: d_vids is ascending.  No kernel waits on
// another workgroup: every dependency is a kernel boundary on one stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "stage.h"
#include "ws.h"

namespace nbg {

const char* const kGpKernelNames[GP_KINDS] = {"k_gp_resolve", "k_gp_table", "k_gp_degrees", "k_gp_emit", "k_gp_compact"};

namespace {

constexpr uint32_t GP_TBLOCK = (uint32_t)OB_CHUNK;   // table entries a workgroup walks per block
constexpr int GP_STEPS = (int)(OB_CHUNK / BLOCK);

struct GpTypes {
  int n;
  uint32_t cap;
  const uint32_t* row_ptr[MAX_TYPES_Q];
};
struct GpIndexOut {
  int64_t* ids;                      // null: no index
  uint32_t mask;                     // the columns gathered
  int64_t* col[MAX_INPUT_COLS];
};

// the block's sum of one 64-bit value per thread, in thread 0 (lds: WAVES cells, free again on return)
__device__ __forceinline__ unsigned long long gp_block_sum(unsigned long long v, unsigned long long* lds) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t lo = __shfl_down((uint32_t)v, o, 64), hi = __shfl_down((uint32_t)(v >> 32), o, 64);
    v += ((unsigned long long)hi << 32) | lo;
  }
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned long long t = 0;
  if (threadIdx.x == 0)
    for (int w = 0; w < WAVES; ++w) t += lds[w];
  __syncthreads();
  return t;
}

__global__ void __launch_bounds__(BLOCK) k_gp_resolve(const uint64_t* __restrict__ chunk, uint32_t nchunks,
                                                      const int64_t* const* __restrict__ cols, int vid_col,
                                                      const int64_t* __restrict__ vids, uint64_t nv,
                                                      uint32_t* __restrict__ dense, uint32_t* __restrict__ ccount,
                                                      uint32_t* __restrict__ last_row) {
  __shared__ uint32_t wcnt[WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t* __restrict__ vcol = cols[vid_col];
  for (uint32_t k = blockIdx.x; k < nchunks; k += gridDim.x) {
    const uint64_t b = chunk[3 * k], len = chunk[3 * k + 1], lo = chunk[3 * k + 2];
    uint32_t mine = 0;   // (wave-uniform)
    for (uint64_t c0 = 0; c0 < len; c0 += BLOCK) {
      const uint64_t i = c0 + threadIdx.x;
      bool found = false;
      if (i < len) {
        const int64_t vid = vcol[b + i];
        const uint64_t d = fv_lower_bound(vids, 0, nv, vid);
        found = d < nv && vids[d] == vid;
        dense[lo + i] = found ? (uint32_t)d : NO_ROW;
        if (found && last_row) atomicMax(&last_row[d], (uint32_t)(lo + i + 1));
      }
      mine += (uint32_t)__popcll(__ballot(found));
    }
    if (lane == 0) wcnt[wave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t t = 0;
      for (int w = 0; w < WAVES; ++w) t += wcnt[w];
      ccount[k] = t;
    }
    __syncthreads();   // (wcnt is rewritten for the next chunk)
  }
}

// the capped degree of vertex d over one CSR
__device__ __forceinline__ uint32_t gp_degree(const uint32_t* __restrict__ rp, uint32_t d, uint32_t cap) {
  const uint32_t deg = rp[d + 1] - rp[d];
  return deg < cap ? deg : cap;
}

__global__ void __launch_bounds__(BLOCK) k_gp_table(const uint32_t* __restrict__ last_row, uint64_t nv, uint32_t nblocks,
                                                    uint32_t* __restrict__ ucount, GpTypes ty,
                                                    unsigned long long* __restrict__ deg) {
  __shared__ unsigned long long lds[WAVES];
  for (uint32_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    const uint64_t d0 = (uint64_t)blk * GP_TBLOCK;
    unsigned long long mine = 0;
    for (int s = 0; s < GP_STEPS; ++s) {
      const uint64_t d = d0 + (uint64_t)s * BLOCK + threadIdx.x;
      mine += d < nv && last_row[d] != 0;
    }
    const unsigned long long cnt = gp_block_sum(mine, lds);
    if (threadIdx.x == 0) ucount[blk] = (uint32_t)cnt;
    for (int t = 0; t < ty.n; ++t) {   // (DISTINCT only: the unique list's edge space)
      unsigned long long sum = 0;
      for (int s = 0; s < GP_STEPS; ++s) {
        const uint64_t d = d0 + (uint64_t)s * BLOCK + threadIdx.x;
        if (d < nv && last_row[d] != 0) sum += gp_degree(ty.row_ptr[t], (uint32_t)d, ty.cap);
      }
      sum = gp_block_sum(sum, lds);
      if (threadIdx.x == 0 && sum) atomicAdd(&deg[t], sum);
    }
  }
}

__global__ void __launch_bounds__(BLOCK) k_gp_degrees(const uint32_t* __restrict__ dense, uint64_t n, GpTypes ty,
                                                      unsigned long long* __restrict__ deg) {
  __shared__ unsigned long long lds[WAVES];
  for (int t = 0; t < ty.n; ++t) {
    unsigned long long sum = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BLOCK) {
      const uint32_t d = dense[i];
      if (d != NO_ROW) sum += gp_degree(ty.row_ptr[t], d, ty.cap);
    }
    sum = gp_block_sum(sum, lds);
    if (threadIdx.x == 0 && sum) atomicAdd(&deg[t], sum);
  }
}

// Ranks of the block's takers over GP_STEPS strides of BLOCK entries: woff[s * WAVES + wave] becomes
// the number of takers before that wave's stride (two barriers; the caller adds lane_rank).
__device__ __forceinline__ void gp_rank_strides(uint32_t* woff, int steps) {
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t total = 0;
    for (int j = 0; j < steps * WAVES; ++j) {
      const uint32_t c = woff[j];
      woff[j] = total;
      total += c;
    }
  }
  __syncthreads();
}

__global__ void __launch_bounds__(BLOCK) k_gp_emit(const uint64_t* __restrict__ chunk, uint32_t nchunks,
                                                   const uint32_t* __restrict__ dense, const uint32_t* __restrict__ cbase,
                                                   uint32_t* __restrict__ dst, uint64_t cap) {
  __shared__ uint32_t woff[GP_STEPS * WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (uint32_t k = blockIdx.x; k < nchunks; k += gridDim.x) {
    const uint64_t len = chunk[3 * k + 1], lo = chunk[3 * k + 2];                       // len <= OB_CHUNK
    const int steps = (int)((len < OB_CHUNK ? len : OB_CHUNK) + BLOCK - 1) / BLOCK;     // <= GP_STEPS
    for (int s = 0; s < steps; ++s) {
      const uint64_t i = (uint64_t)s * BLOCK + threadIdx.x;
      const bool take = i < len && dense[lo + (i < len ? i : 0)] != NO_ROW;
      const unsigned long long bal = __ballot(take);
      if (lane == 0) woff[s * WAVES + wave] = (uint32_t)__popcll(bal);
    }
    gp_rank_strides(woff, steps);
    const uint64_t base = cbase[k];
    for (int s = 0; s < steps; ++s) {
      const uint64_t i = (uint64_t)s * BLOCK + threadIdx.x;
      const uint32_t d = i < len ? dense[lo + i] : NO_ROW;
      const unsigned long long bal = __ballot(d != NO_ROW);
      const uint64_t slot = base + woff[s * WAVES + wave] + lane_rank(bal);
      if (d != NO_ROW && slot < cap) dst[slot] = d;
    }
    __syncthreads();   // (woff is rewritten for the next chunk)
  }
}

__global__ void __launch_bounds__(BLOCK) k_gp_compact(const uint32_t* __restrict__ last_row, uint64_t nv, uint32_t nblocks,
                                                      const uint32_t* __restrict__ ubase, uint64_t cap,
                                                      uint32_t* __restrict__ list, GpIndexOut ix,
                                                      const int64_t* __restrict__ vids,
                                                      const int64_t* const* __restrict__ cols,
                                                      const uint64_t* __restrict__ chunk, uint32_t nchunks) {
  __shared__ uint32_t woff[GP_STEPS * WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (uint32_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    const uint64_t d0 = (uint64_t)blk * GP_TBLOCK;
    for (int s = 0; s < GP_STEPS; ++s) {
      const uint64_t d = d0 + (uint64_t)s * BLOCK + threadIdx.x;
      const unsigned long long bal = __ballot(d < nv && last_row[d < nv ? d : 0] != 0);
      if (lane == 0) woff[s * WAVES + wave] = (uint32_t)__popcll(bal);
    }
    gp_rank_strides(woff, GP_STEPS);
    const uint64_t base = ubase[blk];
    for (int s = 0; s < GP_STEPS; ++s) {
      const uint64_t d = d0 + (uint64_t)s * BLOCK + threadIdx.x;
      const uint32_t lr = d < nv ? last_row[d] : 0u;
      const unsigned long long bal = __ballot(lr != 0);
      const uint64_t slot = base + woff[s * WAVES + wave] + lane_rank(bal);
      if (!lr || slot >= cap) continue;
      if (list) list[slot] = (uint32_t)d;
      if (!ix.ids) continue;
      ix.ids[slot] = vids[d];
      // the winning logical row's chunk: the last one that starts at or before it
      const uint64_t r = lr - 1;
      uint32_t k0 = 0, k1 = nchunks;   // chunk[3 k0 + 2] <= r < chunk[3 k1 + 2]
      while (k1 - k0 > 1) {
        const uint32_t km = (k0 + k1) >> 1;
        if (chunk[3 * (uint64_t)km + 2] <= r) k0 = km;
        else k1 = km;
      }
      const uint64_t off = r - chunk[3 * (uint64_t)k0 + 2];
      if (off >= chunk[3 * (uint64_t)k0 + 1]) continue;   // (no such row: cannot happen for a row k_gp_resolve stored)
      const uint64_t phys = chunk[3 * (uint64_t)k0] + off;
      for (uint32_t m = ix.mask; m; m &= m - 1) {
        const int c = __builtin_ctz(m);
        ix.col[c][slot] = cols[c][phys];
      }
    }
    __syncthreads();   // (woff is rewritten for the next block)
  }
}

}  // namespace

struct GoPipe {
  StageStatus cs{"GO FROM $-"};
  StageScratch sc;   // (declared before the timer: the timer's events are resolved first)
  StageTimer<GP_KINDS> tm{nullptr, nullptr, {}, nullptr};
  StageChunks ch;
  GpPlan plan;
  Workspace* inw = nullptr;
  hipStream_t stream = nullptr;
  uint64_t n = 0;
  uint32_t nblocks = 0;   // table blocks
  uint32_t *dense = nullptr, *ccount = nullptr, *cbase = nullptr, *last_row = nullptr, *ucount = nullptr, *ubase = nullptr;
  GpCounts* state = nullptr;
  GpCounts counts{};
  GpTypes types() const {
    GpTypes ty{};
    ty.n = plan.ntypes;
    ty.cap = plan.cap;
    for (int t = 0; t < plan.ntypes; ++t) ty.row_ptr[t] = plan.row_ptr[t];
    return ty;
  }
  unsigned table_grid() const { return std::min<unsigned>(std::max<uint32_t>(nblocks, 1), STAGE_GRID); }
};

int32_t gopipe_open(Workspace* inw, hipStream_t stream, const std::vector<std::pair<uint64_t, uint64_t>>& segs,
                    const GpPlan& plan, StageProf<GP_KINDS>* prof, GoPipe** out, GpCounts* counts, std::string* err) {
  *out = nullptr;
  uint64_t n = 0;
  for (auto& sg : segs) n += sg.second;
  if (!inw || !n || n > 0xFFFFFFFFull || plan.vid_col < 0 || plan.vid_col >= MAX_YIELDS || !plan.vids ||
      plan.nv >= (uint64_t)NO_ROW || plan.ntypes < 0 || plan.ntypes > MAX_TYPES_Q) {
    if (err) *err = "GO FROM $-: empty input or plan";
    return NBG_E_INVALID_ARGUMENT;
  }
  std::unique_ptr<GoPipe, void (*)(GoPipe*)> p(new GoPipe(), gopipe_close);
  p->plan = plan;
  p->inw = inw;
  p->stream = stream;
  p->n = n;
  p->tm.prof = prof;
  p->tm.stream = stream;
  StageStatus& cs = p->cs;
  StageScratch& sc = p->sc;
  const bool table = plan.distinct || plan.index;
  p->nblocks = table ? (uint32_t)cdiv(plan.nv, GP_TBLOCK) : 0;
  if (p->ch.upload(cs, sc, stream, segs, 0, n)) return cs.code(err);
  // one block for the rest of the scratch (an allocation costs more than these kernels at small
  // inputs): the counters and the table first, cleared by one memset
  size_t total = 0;
  auto carve = [&](size_t bytes) {
    const size_t at = total;
    total += (bytes + 255) & ~(size_t)255;
    return at;
  };
  const size_t o_state = carve(sizeof(GpCounts)), o_table = carve(table ? plan.nv * 4 : 0), cleared = total;
  const size_t o_ucount = carve((size_t)p->nblocks * 4), o_ubase = carve((size_t)p->nblocks * 4);
  const size_t o_dense = carve(n * 4), o_ccount = carve((size_t)p->ch.n * 4), o_cbase = carve((size_t)p->ch.n * 4);
  char* block = nullptr;
  if (cs.failed(sc.alloc((void**)&block, total), "scratch") || cs.failed(hipMemsetAsync(block, 0, cleared, stream), "scratch clear"))
    return cs.code(err);
  p->state = (GpCounts*)(block + o_state);
  if (table) {
    p->last_row = (uint32_t*)(block + o_table);
    p->ucount = (uint32_t*)(block + o_ucount);
    p->ubase = (uint32_t*)(block + o_ubase);
  }
  p->dense = (uint32_t*)(block + o_dense);
  p->ccount = (uint32_t*)(block + o_ccount);
  p->cbase = (uint32_t*)(block + o_cbase);

  StageTimer<GP_KINDS>& tm = p->tm;
  const GpTypes none{};
  tm.begin();
  hipLaunchKernelGGL(k_gp_resolve, dim3(p->ch.grid), dim3(BLOCK), 0, stream, p->ch.dev, p->ch.n,
                     (const int64_t* const*)inw->d_row_cols, plan.vid_col, plan.vids, plan.nv, p->dense, p->ccount, p->last_row);
  tm.end(GP_K_RESOLVE, (double)n * (8.0 + 4.0 + (table ? 4.0 : 0.0)));
  if (cs.failed(hipGetLastError(), "k_gp_resolve")) return cs.code(err);
  if (table) {
    tm.begin();
    hipLaunchKernelGGL(k_gp_table, dim3(p->table_grid()), dim3(BLOCK), 0, stream, p->last_row, plan.nv, p->nblocks, p->ucount,
                       plan.distinct ? p->types() : none, p->state->deg);
    tm.end(GP_K_TABLE, (double)plan.nv * 4.0 * (1 + (plan.distinct ? plan.ntypes : 0)));
    if (cs.failed(hipGetLastError(), "k_gp_table") ||
        cs.failed(launch_yr_scan(p->ucount, p->nblocks, p->ubase, (YrState*)&p->state->unique, stream), "k_yr_scan"))
      return cs.code(err);
  }
  if (cs.failed(launch_yr_scan(p->ccount, p->ch.n, p->cbase, (YrState*)&p->state->found, stream), "k_yr_scan"))
    return cs.code(err);
  if (!plan.distinct && plan.ntypes) {
    tm.begin();
    hipLaunchKernelGGL(k_gp_degrees, dim3(std::min<unsigned>((unsigned)cdiv(n, BLOCK * 8), STAGE_GRID)), dim3(BLOCK), 0, stream,
                       p->dense, n, p->types(), p->state->deg);
    tm.end(GP_K_DEGREES, (double)n * 4.0 * plan.ntypes);
    if (cs.failed(hipGetLastError(), "k_gp_degrees")) return cs.code(err);
  }
  // ---- the one read-back
  if (cs.failed(hipMemcpyAsync(&p->counts, p->state, sizeof(GpCounts), hipMemcpyDeviceToHost, stream), "counts read") ||
      cs.failed(hipStreamSynchronize(stream), "join"))
    return cs.code(err);
  if (p->counts.found > n || p->counts.unique > p->counts.found) {
    if (err) *err = "GO FROM $-: " + std::to_string(p->counts.found) + " rows found of " + std::to_string(n);
    return NBG_E_DEVICE;
  }
  *counts = p->counts;
  *out = p.release();
  return NBG_OK;
}

hipError_t gopipe_list(GoPipe* p, Workspace* ws, uint32_t* host) {
  const uint64_t cap = p->plan.distinct ? p->counts.unique : p->counts.found;
  uint32_t* dst = nullptr;
  if (ws) {
    if (cap > ws->cap_frontier || ws->stream != p->stream) return hipErrorInvalidValue;
    dst = ws->frontier[0];
  } else {
    HIP_TRY(p->sc.alloc((void**)&dst, cap * 4));
  }
  if (cap) {
    p->tm.begin();
    if (p->plan.distinct) {
      hipLaunchKernelGGL(k_gp_compact, dim3(p->table_grid()), dim3(BLOCK), 0, p->stream, p->last_row, p->plan.nv, p->nblocks,
                         p->ubase, cap, dst, GpIndexOut{}, p->plan.vids, (const int64_t* const*)p->inw->d_row_cols, p->ch.dev,
                         p->ch.n);
      p->tm.end(GP_K_COMPACT, (double)p->plan.nv * 4.0 + (double)cap * 4.0);
    } else {
      hipLaunchKernelGGL(k_gp_emit, dim3(p->ch.grid), dim3(BLOCK), 0, p->stream, p->ch.dev, p->ch.n, p->dense, p->cbase, dst,
                         cap);
      p->tm.end(GP_K_EMIT, (double)p->n * 4.0 + (double)cap * 4.0);
    }
    HIP_TRY(hipGetLastError());
  }
  if (host && cap) {
    HIP_TRY(hipMemcpyAsync(host, dst, cap * 4, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
  }
  return hipSuccess;
}

hipError_t gopipe_index(GoPipe* p, uint32_t mask, int ncols, int64_t** in_ids, std::vector<int64_t*>* cols) {
  if (!p->last_row || ncols < 0 || ncols > MAX_INPUT_COLS || ncols > MAX_YIELDS) return hipErrorInvalidValue;
  const uint64_t cap = p->counts.unique;
  cols->assign(ncols, nullptr);
  GpIndexOut ix{};
  HIP_TRY(hipMalloc((void**)in_ids, std::max<uint64_t>(cap, 1) * 8));
  ix.ids = *in_ids;
  int nref = 0;
  for (int c = 0; c < ncols; ++c) {
    if (!((mask >> c) & 1u)) continue;
    HIP_TRY(hipMalloc((void**)&(*cols)[c], std::max<uint64_t>(cap, 1) * 8));
    ix.col[c] = (*cols)[c];
    ix.mask |= 1u << c;
    ++nref;
  }
  if (!cap) return hipSuccess;
  p->tm.begin();
  hipLaunchKernelGGL(k_gp_compact, dim3(p->table_grid()), dim3(BLOCK), 0, p->stream, p->last_row, p->plan.nv, p->nblocks,
                     p->ubase, cap, (uint32_t*)nullptr, ix, p->plan.vids, (const int64_t* const*)p->inw->d_row_cols, p->ch.dev,
                     p->ch.n);
  p->tm.end(GP_K_COMPACT, (double)p->plan.nv * 4.0 + (double)cap * (8.0 + 16.0 * nref));
  return hipGetLastError();
}

void gopipe_close(GoPipe* p) { delete p; }

}  // namespace nbg
