// nebula_amd — UNION / INTERSECT / MINUS over two device-resident results (gfx950, wave64).
// SetExecutor (src/graph/SetExecutor.cpp:98-383) over the row segments earlier stages leave in HBM.
// A cell is read through so_cell: a right-side cell goes through its column's cast to the left's
// type (InterimResult::castTo*) and, for hashing and comparing, -0.0 is 0.0 in a DOUBLE column.
//   k_so_insert   rows of one side into an open-addressing row table (k_gb_keys' CAS and
//                 re-compare over every column): UNION DISTINCT inserts the left, then the right,
//                 and a slot's CAS winner is that value's survivor; INTERSECT inserts the right and
//                 counts its multiplicity per slot (one atomic per distinct row of a wave); MINUS
//                 inserts the right
//   k_so_probe    left rows probe read-only: MINUS keeps the absent ones, INTERSECT those that
//                 take a unit of their slot's counter; one keep-flag byte per row
//   k_so_emit     kept rows compacted into the one-segment result, every column: ballot / mbcnt
//                 positions inside a wave, one reservation per chunk (k_ob_compact)
//   k_so_copy     UNION ALL: chunk slices at their logical offsets, the right through its casts
// Both inputs are walked through the chunk list of stage.h, one workgroup per chunk.  No kernel
// waits on another workgroup: every dependency is a kernel boundary on one stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "ordimg.h"
#include "stage.h"
#include "ws.h"

namespace nbg {

const char* const kSoKernelNames[SO_KINDS] = {"k_so_insert", "k_so_probe", "k_so_emit", "k_so_copy"};

namespace {

constexpr int SO_ROUNDS = 8;            // distinct rows a wave combines per 64 rows before its lanes go alone
constexpr uint32_t SO_F_COUNT = 1u;     // k_so_insert: count the inserted rows per slot
constexpr uint32_t SO_F_SKIP_NAN = 2u;  // ... leave out rows holding a NaN in a DOUBLE column
constexpr uint32_t SO_F_MARK = 4u;      // ... flag (and count) the rows that won their slot
constexpr uint64_t SO_SEED = 0x7365746F70ull;

struct SoSides {
  int64_t* const* cols[2];   // the column bases of the left (0) and the right (1) input
};
// the state of one call: rows kept so far, k_so_emit's slot counter
struct SoState {
  unsigned long long kept, emitted;
};

__device__ __forceinline__ uint64_t so_mix64(uint64_t x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}

__device__ __forceinline__ bool so_is_nan(uint64_t bits) { return (bits & ~SIGN64) > 0x7FF0000000000000ull; }

// a right cell as the left's type (InterimResult.cpp:292-538)
__device__ __forceinline__ int64_t so_cast(int64_t v, uint8_t op) {
  switch (op) {
    case SO_D2I: return (int64_t)__longlong_as_double((long long)v);   // NaN, |x| >= 2^63: unspecified
    case SO_B2I: case SO_I2B: return v != 0;
    case SO_I2D: return (int64_t)__double_as_longlong(__ll2double_rn((long long)v));
    case SO_B2D: return (int64_t)__double_as_longlong(v != 0 ? 1.0 : 0.0);
    case SO_D2B: return __longlong_as_double((long long)v) != 0.0;
    default: return v;
  }
}

// fold: the cell as it is hashed and compared (-0.0 is 0.0 in a DOUBLE column), else as it is stored
__device__ __forceinline__ uint64_t so_cell(const SoPlan* __restrict__ pl, const SoSides& sd, int side, int col,
                                            uint64_t row, bool fold) {
  int64_t v = sd.cols[side][col][row];
  if (side) v = so_cast(v, pl->cast[col]);
  if (fold && pl->dbl[col] && (uint64_t)v == SIGN64) v = 0;
  return (uint64_t)v;
}

// a row reference: the side in bit 63, physical row + 1 below (0: an empty slot)
__device__ __forceinline__ unsigned long long so_ref(int side, uint64_t row) {
  return ((unsigned long long)side << 63) | (unsigned long long)(row + 1);
}

__device__ __forceinline__ uint64_t so_row_hash(const SoPlan* __restrict__ pl, const SoSides& sd, int side,
                                                uint64_t row) {
  uint64_t h = SO_SEED;
  for (int c = 0; c < pl->ncols; ++c) h = so_mix64(h ^ so_cell(pl, sd, side, c, row, true) ^ (uint64_t)c);
  return h;
}

__device__ __forceinline__ bool so_row_eq(const SoPlan* __restrict__ pl, const SoSides& sd, unsigned long long ref,
                                          int side, uint64_t row) {
  const int rs = (int)(ref >> 63);
  const uint64_t rr = (uint64_t)(ref & ~SIGN64) - 1;
  bool eq = true;
  for (int c = 0; c < pl->ncols && eq; ++c) eq = so_cell(pl, sd, rs, c, rr, true) == so_cell(pl, sd, side, c, row, true);
  return eq;
}

__device__ __forceinline__ bool so_row_nan(const SoPlan* __restrict__ pl, const SoSides& sd, int side, uint64_t row) {
  bool nan = false;
  for (int c = 0; c < pl->ncols; ++c) nan = nan || (pl->dbl[c] && so_is_nan(so_cell(pl, sd, side, c, row, true)));
  return nan;
}

__device__ __forceinline__ void so_wave_total(unsigned long long mine, unsigned long long* total) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(total, mine);
}

// chunk[3k..3k+2] = (first physical row, rows (<= OB_CHUNK), logical index of the first row)
__global__ void __launch_bounds__(BLOCK) k_so_insert(const uint64_t* __restrict__ chunk, uint32_t nchunks, int side,
                                                     const SoPlan* __restrict__ pl, SoSides sd,
                                                     unsigned long long* __restrict__ tab, uint32_t* __restrict__ cnt,
                                                     uint64_t tmask, uint32_t flags, uint8_t* __restrict__ keep,
                                                     SoState* __restrict__ st) {
  const int lane = threadIdx.x & 63;
  unsigned long long mine = 0;
  for (uint32_t k = blockIdx.x; k < nchunks; k += gridDim.x) {
    const uint64_t b = chunk[3 * k], len = chunk[3 * k + 1], lo = chunk[3 * k + 2];
    for (uint64_t c0 = 0; c0 < len; c0 += BLOCK) {
      const uint64_t i = c0 + threadIdx.x;
      const bool valid = i < len;
      const uint64_t row = b + (valid ? i : 0);
      const bool ins = valid && !((flags & SO_F_SKIP_NAN) && so_row_nan(pl, sd, side, row));
      uint64_t slot = 0;
      if (ins) {
        const unsigned long long me = so_ref(side, row);
        for (uint64_t p = so_row_hash(pl, sd, side, row) & tmask;; p = (p + 1) & tmask) {
          unsigned long long cur = tab[p];
          if (cur == 0ull) {
            cur = atomicCAS(tab + p, 0ull, me);
            if (cur == 0ull) {   // this row is its value's survivor
              if (flags & SO_F_MARK) {
                keep[lo + i] = 1;
                ++mine;
              }
              slot = p;
              break;
            }
          }
          if (so_row_eq(pl, sd, cur, side, row)) {
            slot = p;
            break;
          }
        }
      }
      if (flags & SO_F_COUNT) {
        // one atomic per distinct row of the wave: the first pending lane's slot and the lanes on it
        unsigned long long rem = __ballot(ins);
        for (int round = 0; rem && round < SO_ROUNDS; ++round) {
          const int leader = __ffsll(rem) - 1;
          const uint64_t ls = (uint64_t)__shfl((unsigned long long)slot, leader);
          const unsigned long long m = __ballot(((rem >> lane) & 1ull) && slot == ls);
          if (lane == leader) atomicAdd(cnt + ls, (uint32_t)__popcll(m));
          rem &= ~m;
        }
        if ((rem >> lane) & 1ull) atomicAdd(cnt + slot, 1u);
      }
    }
  }
  if (flags & SO_F_MARK) so_wave_total(mine, &st->kept);
}

__global__ void __launch_bounds__(BLOCK) k_so_probe(const uint64_t* __restrict__ chunk, uint32_t nchunks,
                                                    const SoPlan* __restrict__ pl, SoSides sd,
                                                    const unsigned long long* __restrict__ tab,
                                                    uint32_t* __restrict__ cnt, uint64_t tmask,
                                                    uint8_t* __restrict__ keep, SoState* __restrict__ st) {
  const int lane = threadIdx.x & 63;
  const bool minus = pl->op == NBG_SET_MINUS;
  unsigned long long mine = 0;
  for (uint32_t k = blockIdx.x; k < nchunks; k += gridDim.x) {
    const uint64_t b = chunk[3 * k], len = chunk[3 * k + 1], lo = chunk[3 * k + 2];
    for (uint64_t c0 = 0; c0 < len; c0 += BLOCK) {
      const uint64_t i = c0 + threadIdx.x;
      const bool valid = i < len;
      const uint64_t row = b + (valid ? i : 0);
      bool found = false;
      uint64_t slot = 0;
      if (valid && !so_row_nan(pl, sd, 0, row)) {   // a NaN cell equals nothing
        for (uint64_t p = so_row_hash(pl, sd, 0, row) & tmask;; p = (p + 1) & tmask) {
          const unsigned long long cur = tab[p];
          if (cur == 0ull) break;
          if (so_row_eq(pl, sd, cur, 0, row)) {
            found = true;
            slot = p;
            break;
          }
        }
      }
      bool take = valid && !found;
      if (!minus) {
        // INTERSECT: the row takes one unit of its slot's counter.  The counter is tested before it
        // is decremented, so it goes below zero by at most the rows in flight and never wraps; the
        // lanes of a wave on one slot draw their units with one atomic.
        take = false;
        unsigned long long rem = __ballot(found);
        for (int round = 0; rem && round < SO_ROUNDS; ++round) {
          const int leader = __ffsll(rem) - 1;
          const uint64_t ls = (uint64_t)__shfl((unsigned long long)slot, leader);
          const bool match = ((rem >> lane) & 1ull) && slot == ls;
          const unsigned long long m = __ballot(match);
          int32_t before = 0;
          if (lane == leader && (int32_t)__hip_atomic_load(cnt + ls, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > 0)
            before = (int32_t)atomicSub(cnt + ls, (uint32_t)__popcll(m));
          before = __shfl(before, leader);
          if (match) take = (int32_t)lane_rank(m) < before;
          rem &= ~m;
        }
        if ((rem >> lane) & 1ull) {
          if ((int32_t)__hip_atomic_load(cnt + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > 0)
            take = (int32_t)atomicSub(cnt + slot, 1u) > 0;
        }
      }
      if (valid) {
        keep[lo + i] = take;
        mine += take;
      }
    }
  }
  so_wave_total(mine, &st->kept);
}

__global__ void __launch_bounds__(BLOCK) k_so_emit(const uint64_t* __restrict__ chunk, uint32_t nchunks, int side,
                                                   const uint8_t* __restrict__ keep, const SoPlan* __restrict__ pl,
                                                   SoSides sd, int64_t* const* __restrict__ ocols,
                                                   SoState* __restrict__ st, uint64_t cap) {
  // two walks over a chunk's flags, as k_ob_compact: the waves' counts per step, one reservation
  // for the whole chunk, then each wave's rows at its offset in row order
  constexpr int STEPS = (int)(OB_CHUNK / BLOCK);
  __shared__ uint32_t woff[STEPS * WAVES];
  __shared__ unsigned long long sbase;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ncols = pl->ncols;
  for (uint32_t k = blockIdx.x; k < nchunks; k += gridDim.x) {
    const uint64_t b = chunk[3 * k], len = chunk[3 * k + 1], lo = chunk[3 * k + 2];   // len <= OB_CHUNK
    const int steps = (int)((len < OB_CHUNK ? len : OB_CHUNK) + BLOCK - 1) / BLOCK;   // <= STEPS
    for (int s = 0; s < steps; ++s) {
      const uint64_t i = (uint64_t)s * BLOCK + threadIdx.x;
      const bool take = i < len && keep[lo + (i < len ? i : 0)];
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
      sbase = total ? atomicAdd(&st->emitted, (unsigned long long)total) : 0ull;
    }
    __syncthreads();
    const uint64_t base = sbase;
    for (int s = 0; s < steps; ++s) {
      const uint64_t i = (uint64_t)s * BLOCK + threadIdx.x;
      const bool take = i < len && keep[lo + (i < len ? i : 0)];
      const unsigned long long bal = __ballot(take);
      const uint64_t slot = base + woff[s * WAVES + wave] + lane_rank(bal);
      if (take && slot < cap)
        for (int c = 0; c < ncols; ++c) ocols[c][slot] = (int64_t)so_cell(pl, sd, side, c, b + i, false);
    }
    __syncthreads();   // (woff and sbase are rewritten for the next chunk)
  }
}

__global__ void __launch_bounds__(BLOCK) k_so_copy(const uint64_t* __restrict__ chunk, uint32_t nchunks, int side,
                                                   const SoPlan* __restrict__ pl, SoSides sd,
                                                   int64_t* const* __restrict__ ocols, uint64_t obase) {
  for (uint32_t k = blockIdx.x; k < nchunks; k += gridDim.x) {
    const uint64_t b = chunk[3 * k], len = chunk[3 * k + 1], lo = chunk[3 * k + 2];
    for (int c = 0; c < pl->ncols; ++c) {
      int64_t* __restrict__ dst = ocols[c] + obase + lo;
      for (uint64_t i = threadIdx.x; i < len; i += BLOCK) dst[i] = (int64_t)so_cell(pl, sd, side, c, b + i, false);
    }
  }
}

}  // namespace

int32_t ws_set_op(Workspace* lw, Workspace* rw, hipStream_t stream,
                  const std::vector<std::pair<uint64_t, uint64_t>>& lsegs,
                  const std::vector<std::pair<uint64_t, uint64_t>>& rsegs, const SoPlan& plan, Workspace** outw,
                  uint64_t* rows, StageProf<SO_KINDS>* prof, std::string* err) {
  *outw = nullptr;
  *rows = 0;
  StageStatus cs("set operation");
  uint64_t n[2] = {0, 0};
  for (auto& sg : lsegs) n[0] += sg.second;
  for (auto& sg : rsegs) n[1] += sg.second;
  const bool all = plan.op == NBG_SET_UNION && !plan.distinct;
  if (plan.op < NBG_SET_UNION || plan.op > NBG_SET_MINUS || plan.ncols < 1 || plan.ncols > MAX_YIELDS || !n[0] || !n[1]) {
    if (err) *err = "set operation: empty input or plan";
    return NBG_E_INVALID_ARGUMENT;
  }
  auto too_large = [&]() {
    if (err) *err = "set operation: a result of 2^32 rows or more";
    return NBG_E_UNSUPPORTED;
  };
  if (all && n[0] + n[1] > 0xFFFFFFFFull) return too_large();
  if (plan.op == NBG_SET_INTERSECT && n[1] > 0x7FFFFFFFull) {   // (a slot's counter is a signed 32-bit count)
    if (err) *err = "set operation: INTERSECT with a right input of 2^31 rows or more";
    return NBG_E_UNSUPPORTED;
  }

  RowsWs res;
  StageScratch sc;   // (declared before the timer: the timer's events are resolved first)
  StageTimer<SO_KINDS> tm{prof, stream, {}, nullptr};
  const SoSides sd{{lw->d_row_cols, rw->d_row_cols}};
  StageChunks ch[2];
  // (the wait after each upload is not for the chunk lists' sake: without it MINUS over few distinct
  // rows measured 2.9 or 4.2 ms per call instead of a steady 3.4)
  for (int s = 0; s < 2; ++s)
    if (ch[s].upload(cs, sc, stream, s ? rsegs : lsegs, 0, n[s]) || cs.failed(hipStreamSynchronize(stream), "chunk upload"))
      return cs.code(err);
  SoPlan* d_plan = nullptr;
  if (cs.failed(sc.alloc((void**)&d_plan, sizeof(SoPlan)), "plan") ||
      cs.failed(hipMemcpyAsync(d_plan, &plan, sizeof(SoPlan), hipMemcpyHostToDevice, stream), "plan upload"))
    return cs.code(err);
  const double row_bytes = plan.ncols * 8.0;

  if (all) {   // the left's rows, then the right's
    if (cs.failed(res.reserve(stream, n[0] + n[1], plan.ncols), "result rows")) return cs.code(err);
    int64_t* const* ocols = (int64_t* const*)res.w->d_row_cols;
    for (int s = 0; s < 2; ++s) {
      tm.begin();
      hipLaunchKernelGGL(k_so_copy, dim3(ch[s].grid), dim3(BLOCK), 0, stream, ch[s].dev, ch[s].n, s, d_plan, sd, ocols,
                         s ? n[0] : 0ull);
      tm.end(SO_K_COPY, (double)n[s] * row_bytes * 2.0);
      if (cs.failed(hipGetLastError(), "k_so_copy")) return cs.code(err);
    }
    if (cs.failed(hipStreamSynchronize(stream), "copy")) return cs.code(err);
    *outw = res.w;
    res.w = nullptr;
    *rows = n[0] + n[1];
    return NBG_OK;
  }

  // ---- the row table and the keep flags
  const bool uni = plan.op == NBG_SET_UNION;
  const uint64_t inserted = uni ? n[0] + n[1] : n[1];
  uint64_t T = SO_MIN_SLOTS;
  while (T < 2 * inserted) T <<= 1;
  unsigned long long* tab = nullptr;
  uint32_t* cnt = nullptr;
  SoState* st = nullptr;
  uint8_t* keep[2] = {nullptr, nullptr};
  if (cs.failed(sc.alloc((void**)&tab, T * 8), "row table") || cs.failed(sc.alloc((void**)&cnt, T * 4), "row table counters") ||
      cs.failed(sc.alloc((void**)&st, sizeof(SoState)), "state") || cs.failed(sc.alloc((void**)&keep[0], n[0]), "keep flags") ||
      (uni && cs.failed(sc.alloc((void**)&keep[1], n[1]), "keep flags")) ||
      cs.failed(hipMemsetAsync(tab, 0, T * 8, stream), "row table clear") ||
      cs.failed(hipMemsetAsync(cnt, 0, T * 4, stream), "row table clear") ||
      cs.failed(hipMemsetAsync(st, 0, sizeof(SoState), stream), "state clear") ||
      (uni && (cs.failed(hipMemsetAsync(keep[0], 0, n[0], stream), "keep flags clear") ||
               cs.failed(hipMemsetAsync(keep[1], 0, n[1], stream), "keep flags clear"))))
    return cs.code(err);
  auto insert = [&](int s, uint32_t flags) {
    tm.begin();
    hipLaunchKernelGGL(k_so_insert, dim3(ch[s].grid), dim3(BLOCK), 0, stream, ch[s].dev, ch[s].n, s, d_plan, sd, tab, cnt,
                       T - 1, flags, keep[s], st);
    tm.end(SO_K_INSERT, (double)n[s] * (row_bytes + 12.0));
    return cs.failed(hipGetLastError(), "k_so_insert");
  };
  if (uni) {
    if (insert(0, SO_F_MARK) || insert(1, SO_F_MARK)) return cs.code(err);
  } else {
    if (insert(1, SO_F_SKIP_NAN | (plan.op == NBG_SET_INTERSECT ? SO_F_COUNT : 0u))) return cs.code(err);
    tm.begin();
    hipLaunchKernelGGL(k_so_probe, dim3(ch[0].grid), dim3(BLOCK), 0, stream, ch[0].dev, ch[0].n, d_plan, sd, tab, cnt, T - 1,
                       keep[0], st);
    tm.end(SO_K_PROBE, (double)n[0] * (row_bytes + 13.0));
    if (cs.failed(hipGetLastError(), "k_so_probe")) return cs.code(err);
  }
  SoState got{};
  if (cs.failed(hipMemcpyAsync(&got, st, sizeof(SoState), hipMemcpyDeviceToHost, stream), "kept rows read") ||
      cs.failed(hipStreamSynchronize(stream), "row table passes"))
    return cs.code(err);
  const uint64_t nout = got.kept;
  if (nout > n[0] + (uni ? n[1] : 0)) {
    if (err) *err = "set operation: " + std::to_string(nout) + " rows kept of " + std::to_string(n[0] + n[1]);
    return NBG_E_DEVICE;
  }
  if (nout > 0xFFFFFFFFull) return too_large();
  if (!nout) return NBG_OK;

  // ---- the kept rows, compacted
  if (cs.failed(res.reserve(stream, nout, plan.ncols), "result rows")) return cs.code(err);
  int64_t* const* ocols = (int64_t* const*)res.w->d_row_cols;
  for (int s = 0; s < (uni ? 2 : 1); ++s) {
    tm.begin();
    hipLaunchKernelGGL(k_so_emit, dim3(ch[s].grid), dim3(BLOCK), 0, stream, ch[s].dev, ch[s].n, s, keep[s], d_plan, sd, ocols,
                       st, nout);
    tm.end(SO_K_EMIT, (double)n[s] + (double)nout * row_bytes * (uni ? 1.0 : 2.0));
    if (cs.failed(hipGetLastError(), "k_so_emit")) return cs.code(err);
  }
  if (cs.failed(hipMemcpyAsync(&got, st, sizeof(SoState), hipMemcpyDeviceToHost, stream), "emitted rows read") ||
      cs.failed(hipStreamSynchronize(stream), "emission"))
    return cs.code(err);
  if (got.emitted != nout) {
    if (err) *err = "set operation: " + std::to_string(got.emitted) + " rows emitted, " + std::to_string(nout) + " kept";
    return NBG_E_DEVICE;
  }
  *outw = res.release();
  *rows = nout;
  return NBG_OK;
}

}  // namespace nbg
