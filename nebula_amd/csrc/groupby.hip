// nebula_amd — GROUP BY with aggregates over a device-resident GO result (gfx950).
// GroupByExecutor::groupingData (src/graph/GroupByExecutor.cpp:226-322) and the functions of
// src/graph/AggregateFunction.h, over the row segments a GO leaves in HBM (rows.hip):
//   k_gb_keys      every row's key into an open-addressing table (k_distinct_mark's hash and
//                  compare over the key columns); a slot's winner draws a dense group id
//   k_gb_accum     every row finds its group (read-only probe) and applies the aggregates,
//                  combined inside the wave first; accumulators in LDS (few groups) or HBM
//   k_gb_accum     again for STD: the squared distances from the now known averages
//   k_gb_distinct  COUNT_DISTINCT: a second table keyed by (group, payload)
//   k_gb_emit      one result row per group
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

#include "ordimg.h"
#include "stage.h"
#include "ws.h"

namespace nbg {

namespace {

constexpr int GB_ROUNDS = 8;   // groups a wave combines per 64 rows before its lanes go alone

__device__ __forceinline__ uint64_t gb_mix64(uint64_t x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}

// a key cell: -0.0 is 0.0 in a DOUBLE column (ColumnValue::operator==, std::hash<double>)
__device__ __forceinline__ uint64_t gb_cell(int64_t v, uint8_t dbl) {
  return (dbl && (uint64_t)v == SIGN64) ? 0ull : (uint64_t)v;
}

__device__ __forceinline__ uint64_t gb_key_hash(int64_t* const* __restrict__ cols, const GbPlan* __restrict__ pl,
                                                uint64_t row) {
  uint64_t h = 0x6E6562756C61ull;
  for (int c = 0; c < pl->nkeys; ++c) h = gb_mix64(h ^ gb_cell(cols[pl->key_col[c]][row], pl->key_dbl[c]) ^ (uint64_t)c);
  return h;
}

__device__ __forceinline__ bool gb_key_eq(int64_t* const* __restrict__ cols, const GbPlan* __restrict__ pl, uint64_t a,
                                          uint64_t b) {
  bool eq = true;
  for (int c = 0; c < pl->nkeys && eq; ++c) {
    const int64_t* col = cols[pl->key_col[c]];
    eq = gb_cell(col[a], pl->key_dbl[c]) == gb_cell(col[b], pl->key_dbl[c]);
  }
  return eq;
}

// the group of a row whose key k_gb_keys inserted (read-only probe)
__device__ __forceinline__ uint32_t gb_find(int64_t* const* __restrict__ cols, const GbPlan* __restrict__ pl,
                                            const unsigned long long* __restrict__ tab,
                                            const uint32_t* __restrict__ gidtab, uint64_t tmask, uint64_t row) {
  for (uint64_t p = gb_key_hash(cols, pl, row) & tmask;; p = (p + 1) & tmask) {
    const unsigned long long cur = tab[p];
    if (cur == 0ull) return 0;   // (not reached: every row of the segments was inserted)
    if (cur - 1 == row || gb_key_eq(cols, pl, cur - 1, row)) return gidtab[p];
  }
}

__device__ __forceinline__ uint64_t gb_identity(uint8_t op) {
  switch (op) {
    case GB_MIN: case GB_AND: return ~0ull;
    case GB_SUM_D: case GB_SQ: return SIGN64;   // -0.0: x + -0.0 == x for every x
    default: return 0ull;
  }
}

__device__ __forceinline__ uint64_t gb_combine(uint8_t op, uint64_t a, uint64_t b) {
  switch (op) {
    case GB_SUM_D: case GB_SQ: return (uint64_t)__double_as_longlong(__dadd_rn(__longlong_as_double((long long)a),
                                                                             __longlong_as_double((long long)b)));
    case GB_MAX: return a > b ? a : b;
    case GB_MIN: return a < b ? a : b;
    case GB_AND: return a & b;
    case GB_OR: return a | b;
    case GB_XOR: return a ^ b;
    default: return a + b;
  }
}

__device__ __forceinline__ uint64_t gb_wave_reduce(uint8_t op, uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = gb_combine(op, v, (uint64_t)__shfl_xor((unsigned long long)v, o));
  return v;
}

__device__ __forceinline__ void gb_apply(unsigned long long* p, uint8_t op, uint64_t v) {
  switch (op) {
    case GB_SUM_D: case GB_SQ: atomicAdd(reinterpret_cast<double*>(p), __longlong_as_double((long long)v)); break;
    case GB_MAX: atomicMax(p, (unsigned long long)v); break;
    case GB_MIN: atomicMin(p, (unsigned long long)v); break;
    case GB_AND: atomicAnd(p, (unsigned long long)v); break;
    case GB_OR: atomicOr(p, (unsigned long long)v); break;
    case GB_XOR: atomicXor(p, (unsigned long long)v); break;
    default: atomicAdd(p, (unsigned long long)v); break;
  }
}

__device__ __forceinline__ double gb_avg(uint64_t sum, bool dbl, uint64_t count) {
  const double s = dbl ? __longlong_as_double((long long)sum) : (double)(int64_t)sum;
  return __ddiv_rn(s, (double)count);
}

// what row `row` of group `gid` contributes to accumulator `ac`
__device__ __forceinline__ uint64_t gb_value(const GbAcc& ac, int64_t* const* __restrict__ cols, uint64_t row,
                                             const unsigned long long* __restrict__ gacc, uint64_t G, uint32_t gid) {
  const uint64_t v = (uint64_t)(ac.col >= 0 ? cols[ac.col][row] : ac.bits);
  switch (ac.op) {
    case GB_COUNT: return 1;
    case GB_MAX: case GB_MIN: return ord_image(v, ac.dbl);
    case GB_SQ: {
      const double x = ac.dbl ? __longlong_as_double((long long)v) : (double)(int64_t)v;
      const double d = __dsub_rn(x, gb_avg(gacc[(uint64_t)ac.ref * G + gid], ac.dbl, gacc[gid]));
      return (uint64_t)__double_as_longlong(__dmul_rn(d, d));
    }
    default: return v;
  }
}

__device__ __forceinline__ bool gb_in_pass(uint8_t op, int pass) {
  return pass == 2 ? op == GB_SQ : (op != GB_SQ && op != GB_DISTINCT);
}

// ----------------------------------------------------------------------------- key pass
// seg[3k..3k+2] = (first row, rows, unused), as the digest walks them
__global__ void __launch_bounds__(BLOCK) k_gb_keys(const uint64_t* __restrict__ seg, int nseg,
                                                   int64_t* const* __restrict__ cols, const GbPlan* __restrict__ pl,
                                                   unsigned long long* __restrict__ tab, uint32_t* __restrict__ gidtab,
                                                   uint64_t tmask, unsigned long long* __restrict__ counter) {
  for (int k = blockIdx.x; k < nseg; k += gridDim.x) {
    const uint64_t b = seg[3 * k], len = seg[3 * k + 1];
    for (uint64_t i = threadIdx.x; i < len; i += BLOCK) {
      const uint64_t row = b + i;
      for (uint64_t p = gb_key_hash(cols, pl, row) & tmask;; p = (p + 1) & tmask) {
        unsigned long long cur = tab[p];
        if (cur == 0ull) {
          cur = atomicCAS(tab + p, 0ull, (unsigned long long)(row + 1));
          if (cur == 0ull) {   // this row represents a new group
            gidtab[p] = (uint32_t)atomicAdd(counter, 1ull);
            break;
          }
        }
        if (gb_key_eq(cols, pl, cur - 1, row)) break;
      }
    }
  }
}

__global__ void __launch_bounds__(BLOCK) k_gb_init(const GbPlan* __restrict__ pl, unsigned long long* __restrict__ acc,
                                                   uint64_t G) {
  const uint64_t n = (uint64_t)pl->nacc * G;
  for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BLOCK)
    acc[i] = gb_identity(pl->acc[i / G].op);
}

// ----------------------------------------------------------------------------- accumulate pass
// acc[slot * G + group].  LDS: the workgroup accumulates into its own copy and flushes it once.
template <bool LDS>
__global__ void __launch_bounds__(BLOCK) k_gb_accum(const uint64_t* __restrict__ seg, int nseg,
                                                    int64_t* const* __restrict__ cols, const GbPlan* __restrict__ pl,
                                                    const unsigned long long* __restrict__ tab,
                                                    const uint32_t* __restrict__ gidtab, uint64_t tmask,
                                                    unsigned long long* __restrict__ acc, uint64_t G, int pass) {
  extern __shared__ unsigned long long lacc[];
  const int lane = threadIdx.x & 63;
  const int nacc = pl->nacc;
  const uint64_t cells = (uint64_t)nacc * G;
  if (LDS) {
    for (uint64_t i = threadIdx.x; i < cells; i += BLOCK) lacc[i] = gb_identity(pl->acc[i / G].op);
    __syncthreads();
  }
  unsigned long long* tgt = LDS ? lacc : acc;
  for (int k = blockIdx.x; k < nseg; k += gridDim.x) {
    const uint64_t b = seg[3 * k], len = seg[3 * k + 1];
    for (uint64_t c0 = 0; c0 < len; c0 += BLOCK) {
      const uint64_t i = c0 + threadIdx.x;
      const bool valid = i < len;
      const uint64_t row = b + (valid ? i : 0);
      uint32_t gid = 0;
      if (valid && pl->nkeys) gid = gb_find(cols, pl, tab, gidtab, tmask, row);
      // one atomic per (group, aggregate) per wave: the first pending lane's group, the lanes that
      // share it, their values reduced across the wave
      unsigned long long rem = __ballot(valid);
      for (int round = 0; rem && round < GB_ROUNDS; ++round) {
        const int leader = __ffsll(rem) - 1;
        const uint32_t lg = (uint32_t)__shfl((int)gid, leader);
        const bool match = ((rem >> lane) & 1ull) && gid == lg;
        const unsigned long long m = __ballot(match);
        const uint64_t n = (uint64_t)__popcll(m);
        for (int a = 0; a < nacc; ++a) {
          const GbAcc ac = pl->acc[a];
          if (!gb_in_pass(ac.op, pass)) continue;
          uint64_t v;
          if (ac.op == GB_COUNT) {
            v = n;
          } else {
            v = match ? gb_value(ac, cols, row, acc, G, gid) : gb_identity(ac.op);
            if (n > 1) v = gb_wave_reduce(ac.op, v);
          }
          if (lane == leader) gb_apply(tgt + (uint64_t)a * G + lg, ac.op, v);
        }
        rem &= ~m;
      }
      if ((rem >> lane) & 1ull) {   // more than GB_ROUNDS groups among these 64 rows: each lane alone
        for (int a = 0; a < nacc; ++a) {
          const GbAcc ac = pl->acc[a];
          if (!gb_in_pass(ac.op, pass)) continue;
          gb_apply(tgt + (uint64_t)a * G + gid, ac.op, gb_value(ac, cols, row, acc, G, gid));
        }
      }
    }
  }
  if (LDS) {
    __syncthreads();
    for (uint64_t i = threadIdx.x; i < cells; i += BLOCK) {
      const uint8_t op = pl->acc[i / G].op;
      const uint64_t v = lacc[i];
      if (gb_in_pass(op, pass) && v != gb_identity(op)) gb_apply(acc + i, op, v);
    }
  }
}

// ----------------------------------------------------------------------------- COUNT_DISTINCT
// accumulator `a`: distinct (group, payload) pairs; a pair's first row adds 1 to its group's cell
__global__ void __launch_bounds__(BLOCK) k_gb_distinct(const uint64_t* __restrict__ seg, int nseg,
                                                       int64_t* const* __restrict__ cols,
                                                       const GbPlan* __restrict__ pl,
                                                       const unsigned long long* __restrict__ tab,
                                                       const uint32_t* __restrict__ gidtab, uint64_t tmask, int a,
                                                       unsigned long long* __restrict__ dtab, uint64_t dmask,
                                                       unsigned long long* __restrict__ acc, uint64_t G) {
  const GbAcc ac = pl->acc[a];
  const int64_t* __restrict__ col = cols[ac.col];
  for (int k = blockIdx.x; k < nseg; k += gridDim.x) {
    const uint64_t b = seg[3 * k], len = seg[3 * k + 1];
    for (uint64_t i = threadIdx.x; i < len; i += BLOCK) {
      const uint64_t row = b + i;
      const uint32_t gid = pl->nkeys ? gb_find(cols, pl, tab, gidtab, tmask, row) : 0u;
      const uint64_t v = gb_cell(col[row], ac.dbl);
      for (uint64_t p = gb_mix64(gb_mix64(0x6E6562756C61ull ^ gid) ^ v) & dmask;; p = (p + 1) & dmask) {
        unsigned long long cur = dtab[p];
        if (cur == 0ull) {
          cur = atomicCAS(dtab + p, 0ull, (unsigned long long)(row + 1));
          if (cur == 0ull) {
            atomicAdd(acc + (uint64_t)a * G + gid, 1ull);
            break;
          }
        }
        const uint64_t orow = cur - 1;
        if (gb_cell(col[orow], ac.dbl) == v &&
            (pl->nkeys ? gb_find(cols, pl, tab, gidtab, tmask, orow) : 0u) == gid)
          break;
      }
    }
  }
}

// ----------------------------------------------------------------------------- emit pass
// one row per group at its id: the table's occupied slots (tslots of them), or the one group
__global__ void __launch_bounds__(BLOCK) k_gb_emit(const GbPlan* __restrict__ pl,
                                                   const unsigned long long* __restrict__ tab,
                                                   const uint32_t* __restrict__ gidtab, uint64_t tslots,
                                                   int64_t* const* __restrict__ cols,
                                                   const unsigned long long* __restrict__ acc, uint64_t G,
                                                   int64_t* const* __restrict__ ocols) {
  for (uint64_t p = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; p < tslots; p += (uint64_t)gridDim.x * BLOCK) {
    uint64_t gid = 0, row = 0;
    if (pl->nkeys) {
      const unsigned long long cur = tab[p];
      if (cur == 0ull) continue;
      gid = gidtab[p];
      row = cur - 1;
    }
    if (gid >= G) continue;
    const uint64_t count = acc[gid];
    for (int o = 0; o < pl->nout; ++o) {
      const GbOut ou = pl->out[o];
      const uint64_t s = acc[(uint64_t)ou.slot * G + gid];
      int64_t v;
      switch (ou.emit) {
        case GE_KEY: v = cols[ou.col][row]; break;
        case GE_CONST: v = ou.bits; break;
        case GE_ORD_I: v = (int64_t)ord_unimage(s, 0); break;
        case GE_ORD_D: v = (int64_t)ord_unimage(s, 1); break;
        case GE_AVG_I: v = __double_as_longlong(gb_avg(s, false, count)); break;
        case GE_AVG_D: v = __double_as_longlong(gb_avg(s, true, count)); break;
        case GE_STD:
          v = __double_as_longlong(__dsqrt_rn(__ddiv_rn(__longlong_as_double((long long)s), (double)count)));
          break;
        default: v = (int64_t)s; break;
      }
      ocols[o][gid] = v;
    }
  }
}

}  // namespace

int32_t ws_group_by(Workspace* inw, hipStream_t stream, const std::vector<std::pair<uint64_t, uint64_t>>& segs,
                    const GbPlan& plan, Workspace** outw, uint64_t* groups, std::string* err) {
  *outw = nullptr;
  *groups = 0;
  StageStatus cs("group by");
  std::vector<uint64_t> meta;
  uint64_t total = 0;
  for (auto& sg : segs) {
    if (!sg.second) continue;
    meta.insert(meta.end(), {sg.first, sg.second, 0});
    total += sg.second;
  }
  if (!total || plan.nacc < 1 || plan.nacc > GB_MAX_ACC || plan.nout < 1 || plan.nout > MAX_YIELDS) {
    if (err) *err = "group by: empty input or plan";
    return NBG_E_INVALID_ARGUMENT;
  }
  const int nseg = (int)(meta.size() / 3);
  const unsigned grid = (unsigned)(nseg < 8192 ? nseg : 8192);
  uint64_t tcap = 1024;   // sized as YIELD DISTINCT sizes its table (ws_distinct)
  while (tcap < 2 * total) tcap <<= 1;
  bool any_sq = false, any_distinct = false;
  for (int a = 0; a < plan.nacc; ++a) {
    any_sq = any_sq || plan.acc[a].op == GB_SQ;
    any_distinct = any_distinct || plan.acc[a].op == GB_DISTINCT;
  }

  StageScratch sc;
  uint64_t* d_meta = nullptr;
  GbPlan* d_plan = nullptr;
  unsigned long long *tab = nullptr, *counter = nullptr, *acc = nullptr, *dtab = nullptr;
  uint32_t* gidtab = nullptr;
  if (cs.failed(sc.alloc((void**)&d_meta, meta.size() * 8), "segment list") ||
      cs.failed(sc.alloc((void**)&d_plan, sizeof(GbPlan)), "plan") ||
      cs.failed(sc.alloc((void**)&counter, 8), "group counter"))
    return cs.code(err);
  if (cs.failed(hipMemcpyAsync(d_meta, meta.data(), meta.size() * 8, hipMemcpyHostToDevice, stream), "segment upload") ||
      cs.failed(hipMemcpyAsync(d_plan, &plan, sizeof(GbPlan), hipMemcpyHostToDevice, stream), "plan upload") ||
      cs.failed(hipMemsetAsync(counter, 0, 8, stream), "counter reset"))
    return cs.code(err);
  int64_t* const* cols = inw->d_row_cols;

  uint64_t G = 1;
  if (plan.nkeys) {
    if (cs.failed(sc.alloc((void**)&tab, tcap * 8), "group table") ||
        cs.failed(sc.alloc((void**)&gidtab, tcap * 4), "group ids"))
      return cs.code(err);
    if (cs.failed(hipMemsetAsync(tab, 0, tcap * 8, stream), "table reset")) return cs.code(err);
    hipLaunchKernelGGL(k_gb_keys, dim3(grid), dim3(BLOCK), 0, stream, d_meta, nseg, cols, d_plan, tab, gidtab, tcap - 1,
                       counter);
    if (cs.failed(hipGetLastError(), "k_gb_keys")) return cs.code(err);
    unsigned long long hg = 0;
    if (cs.failed(hipMemcpyAsync(&hg, counter, 8, hipMemcpyDeviceToHost, stream), "group count") ||
        cs.failed(hipStreamSynchronize(stream), "key pass"))
      return cs.code(err);
    G = hg;
    if (G == 0 || G > total) {
      if (err) *err = "group by: the key pass counted " + std::to_string(G) + " groups of " + std::to_string(total) + " rows";
      return NBG_E_DEVICE;
    }
    if (G > 0xFFFFFFFFull) {
      if (err) *err = "group by: 2^32 groups or more";
      return NBG_E_UNSUPPORTED;
    }
  } else if (cs.failed(hipStreamSynchronize(stream), "uploads")) {   // (the host buffers above are locals)
    return cs.code(err);
  }

  const uint64_t cells = (uint64_t)plan.nacc * G;
  if (cs.failed(sc.alloc((void**)&acc, cells * 8), "accumulators")) return cs.code(err);
  hipLaunchKernelGGL(k_gb_init, dim3((unsigned)std::min<uint64_t>(cdiv(cells, BLOCK), 4096)), dim3(BLOCK), 0, stream,
                     d_plan, acc, G);
  if (cs.failed(hipGetLastError(), "k_gb_init")) return cs.code(err);
  const bool lds = cells * 8 <= GB_LDS_BYTES;
  for (int pass = 1; pass <= (any_sq ? 2 : 1); ++pass) {
    if (lds)
      hipLaunchKernelGGL(k_gb_accum<true>, dim3(grid), dim3(BLOCK), (size_t)(cells * 8), stream, d_meta, nseg, cols,
                         d_plan, tab, gidtab, tcap - 1, acc, G, pass);
    else
      hipLaunchKernelGGL(k_gb_accum<false>, dim3(grid), dim3(BLOCK), 0, stream, d_meta, nseg, cols, d_plan, tab, gidtab,
                         tcap - 1, acc, G, pass);
    if (cs.failed(hipGetLastError(), "k_gb_accum")) return cs.code(err);
  }
  if (any_distinct) {
    if (cs.failed(sc.alloc((void**)&dtab, tcap * 8), "COUNT_DISTINCT table")) return cs.code(err);
    for (int a = 0; a < plan.nacc; ++a) {
      if (plan.acc[a].op != GB_DISTINCT) continue;
      if (cs.failed(hipMemsetAsync(dtab, 0, tcap * 8, stream), "COUNT_DISTINCT table reset")) return cs.code(err);
      hipLaunchKernelGGL(k_gb_distinct, dim3(grid), dim3(BLOCK), 0, stream, d_meta, nseg, cols, d_plan, tab, gidtab,
                         tcap - 1, a, dtab, tcap - 1, acc, G);
      if (cs.failed(hipGetLastError(), "k_gb_distinct")) return cs.code(err);
    }
  }

  RowsWs res;
  if (cs.failed(res.reserve(stream, G, plan.nout), "result rows")) return cs.code(err);
  const uint64_t tslots = plan.nkeys ? tcap : 1;
  hipLaunchKernelGGL(k_gb_emit, dim3((unsigned)std::min<uint64_t>(cdiv(tslots, BLOCK), 8192)), dim3(BLOCK), 0, stream,
                     d_plan, tab, gidtab, tslots, cols, acc, G, (int64_t* const*)res.w->d_row_cols);
  if (cs.failed(hipGetLastError(), "k_gb_emit") || cs.failed(hipStreamSynchronize(stream), "aggregation")) return cs.code(err);
  *outw = res.release();
  *groups = G;
  return NBG_OK;
}

}  // namespace nbg
