// The final GO step over a statement index (stmtidx.hip) whose only YIELD is _dst: a segmented
// copy.  The list is the whole final frontier with its edge space over the filtered rows dst':
// every edge passes, so output row e of [0, total) is known before the kernel runs — it is
// dst'[seg_rs[k] + e - (seg_end[k] - deg_k)] for the entry k whose edge offsets hold e — and the
// result is one dense run out[region_base + e], rows in list order.  k_final_dst (final.hip)
// serves this shape too (NBG_FINAL_COPY=0) and every other one; it places rows with ballots and
// an LDS cursor because it cannot know which edges pass.  Here:
//   * the unit of work is a chunk of CH output rows, one wave per chunk and iteration, adjacent
//     chunks on the waves of one workgroup; every chunk but the list's last is full, and all 64
//     lanes store 16 B each, four times, at addresses that depend on the chunk index alone;
//   * the entry that owns a chunk's first row is found by a wave-wide search of seg_end, 64 probes
//     a round (the first round's probes stay in a register: two gathers for a list of up to
//     64^4 entries), down to a bracket of 64 entries, which is the window the chunk stages anyway.
//     The list producers are not touched: recording a chunk split beside tsplit made
//     k_expand<MARK>, which sits at its 64-VGPR budget, spill to scratch;
//   * a chunk inside one entry (most bytes, the degrees being skewed) is a straight copy;
//     otherwise the entries of the window set head bits and deltas in LDS as final.hip's tiles
//     do, over edge offsets only, and a row's source is two popcounts away;
//   * the search, the window, the rows' loads and their stores of successive chunks overlap: a
//     wave waits for memory once per chunk.
// A window that does not cover its chunk (a list whose offsets do not ascend) fails the query
// (SPLIT_BAD): the chunk's loads then read element 0 of dst' and its stores stay inside the
// chunk's own rows.
#include <hip/hip_runtime.h>

#include "nbg_internal.h"

namespace nbg {
namespace {

constexpr int CB = 256;            // threads per workgroup
constexpr int CW = CB / 64;        // waves per workgroup
constexpr int CH = 512;            // rows per chunk: one wave's unit of work (4 KB of rows)
constexpr int CM = CH / 64;        // head mask words
constexpr int CI = CH / 128;       // 16-byte stores per lane and chunk
static_assert(CH % 128 == 0, "a chunk is whole 16-byte stores of 64 lanes");

// two rows; 8-byte aligned only (a run of dst' starts at any row)
typedef long long row2 __attribute__((ext_vector_type(2), aligned(8)));

__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// a load issued where it is written (see final.hip)
template <typename T>
__device__ __forceinline__ T ld(const T* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

__device__ __forceinline__ uint32_t lanes_below(unsigned long long b) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
}

}  // namespace

// (Outside the anonymous namespace: profilers name it nbg::k_final_copy.)
__global__ void __launch_bounds__(CB) __attribute__((amdgpu_waves_per_eu(8)))
k_final_copy(FinalCopyArgs a) {
  __shared__ unsigned long long sMaskAll[CW][CM];   // chunk positions where an entry's rows start
  __shared__ uint32_t sDeltaAll[CW][CH + 1];        // head rank (1-based) -> row start - edge offset
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  unsigned long long* const sMask = sMaskAll[w];
  uint32_t* const sDelta = sDeltaAll[w];
  const uint32_t g = gridDim.x * CW;
  const uint32_t t_first = blockIdx.x * CW + w;   // adjacent chunks in one workgroup
  const unsigned long long packed = *a.acc;       // (list entries << 32 | edges)
  const uint64_t n = packed >> 32;
  const uint32_t n32 = (uint32_t)n, total = (uint32_t)packed;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (a.stat_e && !a.full_rp) *a.stat_e += total;
    if (a.stat_n) *a.stat_n = n;
  }
  const uint32_t nfull = total / CH;   // full chunks; the list's last rows are chunk nfull
  const uint32_t nlast = n32 ? n32 - 1 : 0u;
  int64_t* const out = a.out + a.region_base;
  // ---- the owner of row r (r < total): the first entry whose inclusive offset exceeds r.  64
  //      probes a round narrow [lo, hi) to a 64th; the first round's probes are the same for
  //      every chunk (lane j: the last entry of the j-th 64th of the list), loaded once
  const uint32_t step1 = (n32 + 63) / 64;
  const uint32_t probe1 = ld(a.seg_end + ((uint32_t)(lane + 1) * step1 - 1 < nlast ? (uint32_t)(lane + 1) * step1 - 1 : nlast));
  auto probe = [&](uint32_t lo, uint32_t hi, uint32_t step) -> uint32_t {
    const uint32_t at = lo + (uint32_t)(lane + 1) * step - 1;
    return ld(a.seg_end + (at < hi - 1 ? at : hi - 1));
  };
  auto narrow = [&](uint32_t* lo, uint32_t* hi, uint32_t step, uint32_t v, uint32_t r) {
    *lo += (uint32_t)__popcll(__ballot(v <= r)) * step;   // (< 64 probes pass: the last one is at hi - 1)
    if (*lo >= *hi) *lo = *hi - 1;                        // (offsets that do not ascend: stay inside the list)
    *hi = *hi - *lo < step ? *hi : *lo + step;
  };
  // the register round, then rounds waited for on the spot while more than two are left (a list
  // of more than 64^4 entries)
  auto begin = [&](uint32_t r, uint32_t* lo, uint32_t* hi) {
    *lo = 0;
    *hi = n32;
    if (n32 > 64) narrow(lo, hi, step1, probe1, r);
    while (*hi - *lo > 64u * 64u * 64u) {   // (wave-uniform)
      const uint32_t step = (*hi - *lo + 63) / 64;
      narrow(lo, hi, step, probe(*lo, *hi, step), r);
    }
  };
  // (returns lo with the owner in [lo, lo + 64))
  auto bracket = [&](uint32_t r) -> uint32_t {
    uint32_t lo, hi;
    begin(r, &lo, &hi);
    while (hi - lo > 64) {   // (wave-uniform)
      const uint32_t step = (hi - lo + 63) / 64;
      narrow(&lo, &hi, step, probe(lo, hi, step), r);
    }
    return lo;
  };
  // lane k's entry s0 + k: the raw edge offsets where it starts and ends and its row start, loaded
  // at clamped indices with no branch; `window` applies the bounds when the values are used
  auto stage = [&](uint32_t s0, uint32_t* x0, uint32_t* x1, uint32_t* rr) {
    const uint32_t q = s0 + (uint32_t)lane;
    const uint32_t c0 = q == 0 ? 0u : (q - 1 < n32 ? q - 1 : nlast);
    const uint32_t c1 = q < n32 ? q : nlast;
    *x0 = ld(a.seg_end + c0);
    *x1 = ld(a.seg_end + c1);
    *rr = ld(a.seg_rs + c1);
  };
  auto window = [&](uint32_t s0, uint32_t x0, uint32_t x1, uint32_t rr, uint32_t* st, uint32_t* en, uint32_t* r) {
    const uint32_t q = s0 + (uint32_t)lane;
    *st = q == 0 ? 0u : (q - 1 < n32 ? x0 : 0xFFFFFFFFu);
    *en = q < n32 ? x1 : 0xFFFFFFFFu;
    *r = q < n32 ? rr : 0u;
  };
  // The source rows of a chunk that spans entries: lane's rows are chunk positions
  // i * 128 + 2 * lane + {0, 1}.  The entries from kb on hold the chunk's rows [r0, r0 + nb);
  // (st, en, rs) is the window at kb.  A position past nb reads the chunk's first row.  False
  // (and element 0 everywhere) when the entries do not cover the chunk.
  auto resolve = [&](uint32_t kb, uint32_t r0, uint32_t nb, uint32_t st, uint32_t en, uint32_t rs,
                     uint32_t (&idx)[2 * CI]) -> bool {
    const uint32_t r1 = r0 + nb;
    if (lane < CM) sMask[lane] = 0;
    uint32_t heads = 0;
    bool first_ok = false, reached = false;
    for (uint32_t s0 = kb;; s0 += 64) {   // (wave-uniform) 64 entries a round
      if (s0 != kb) {
        uint32_t x0, x1, rr;
        stage(s0, &x0, &x1, &rr);
        window(s0, x0, x1, rr, &st, &en, &rs);
      }
      const bool in = s0 + (uint32_t)lane < n32;
      const uint32_t lo = st > r0 ? st : r0, hi = en < r1 ? en : r1;
      const bool head = in && lo < hi;
      const unsigned long long hb = __ballot(head);
      const uint32_t rank = heads + 1 + lanes_below(hb);
      if (head && rank <= (uint32_t)CH) {
        const uint32_t p = lo - r0;   // < nb <= CH
        sDelta[rank] = rs - st;
        atomicOr(&sMask[p >> 6], 1ull << (p & 63));
      }
      if (heads == 0 && hb) first_ok = __ballot(head && lo == r0) != 0;   // the first head owns the first row
      heads += (uint32_t)__popcll(hb);
      reached = __ballot(in && en >= r1) != 0;   // the offsets ascend: no later entry has rows here
      if (reached || nlast - s0 < 64) break;
    }
    wave_lds_sync();
    const bool ok = first_ok && reached && heads <= (uint32_t)CH;
    uint32_t before = 0;
    const int hw = lane >> 5;                     // which word of a pair holds the lane's two bits
    const int b0 = (2 * lane) & 63;
    const unsigned long long le0 = ~0ull >> (63 - b0), le1 = ~0ull >> (62 - b0);
#pragma unroll
    for (int i = 0; i < CI; ++i) {
      const unsigned long long m0 = sMask[2 * i], m1 = sMask[2 * i + 1];
      const uint32_t c0 = (uint32_t)__popcll(m0);
      const unsigned long long m = hw ? m1 : m0;
      const uint32_t base = before + (hw ? c0 : 0u);
      const uint32_t p = (uint32_t)(i * 128 + 2 * lane);
      idx[2 * i] = r0 + p + sDelta[base + (uint32_t)__popcll(m & le0)];
      idx[2 * i + 1] = r0 + p + 1 + sDelta[base + (uint32_t)__popcll(m & le1)];
      before += c0 + (uint32_t)__popcll(m1);
    }
    wave_lds_sync();   // (the next chunk rewrites the window)
    const uint32_t jsafe = ok ? (uint32_t)__builtin_amdgcn_readfirstlane((int)idx[0]) : 0u;
#pragma unroll
    for (int i = 0; i < CI; ++i) {
      const uint32_t p = (uint32_t)(i * 128 + 2 * lane);
      if (!ok || p >= nb) idx[2 * i] = jsafe;
      if (!ok || p + 1 >= nb) idx[2 * i + 1] = jsafe;
    }
    return ok;
  };
  // non-temporal: the rows are not read again by this query (solo launch 113.7 us against
  // 118.7 us with ordinary stores)
  auto store2 = [&](int64_t* p, row2 v) { __builtin_nontemporal_store(v, reinterpret_cast<row2*>(p)); };
  // a full chunk's rows: every lane, 16 B, no condition
  auto store_chunk = [&](const row2 (&v)[CI], uint32_t tt) {
    int64_t* const o = out + (uint64_t)tt * CH + 2 * lane;
#pragma unroll
    for (int i = 0; i < CI; ++i) store2(o + i * 128, v[i]);
  };
  // the rows of full chunk tt from its staged window at kb, every load issued before the first is
  // waited for
  auto fetch = [&](uint32_t tt, uint32_t kb, uint32_t x0, uint32_t x1, uint32_t rr, row2 (&v)[CI]) {
    const uint32_t r0 = tt * CH;
    uint32_t st, en, rs;
    window(kb, x0, x1, rr, &st, &en, &rs);
    // the entry that owns the chunk's first row, and whether it owns the whole chunk
    const unsigned long long own = __ballot(kb + (uint32_t)lane < n32 && st <= r0 && r0 < en);
    const int l0 = own ? __ffsll((long long)own) - 1 : 0;
    const uint32_t st0 = (uint32_t)__builtin_amdgcn_readlane((int)st, l0);
    const uint32_t en0 = (uint32_t)__builtin_amdgcn_readlane((int)en, l0);
    const uint32_t rs0 = (uint32_t)__builtin_amdgcn_readlane((int)rs, l0);
    if (own && en0 - r0 >= (uint32_t)CH) {   // (wave-uniform) inside one entry: a straight copy
      const int64_t* const src = a.dst_vid + (uint64_t)(rs0 + (r0 - st0)) + 2 * lane;
#pragma unroll
      for (int i = 0; i < CI; ++i) v[i] = *reinterpret_cast<const row2*>(src + i * 128);
    } else {
      uint32_t idx[2 * CI];
      const bool ok = resolve(kb, r0, CH, st, en, rs, idx);
      if (!ok && lane == 0) atomicOr(a.err_flag, SPLIT_BAD);
#pragma unroll
      for (int i = 0; i < CI; ++i) {
        v[i].x = ld(a.dst_vid + idx[2 * i]);
        v[i].y = ld(a.dst_vid + idx[2 * i + 1]);
      }
    }
  };
  // ---- the full chunks t_first, t_first + g, ...: a pipeline of one memory round trip per
  //      iteration.  In iteration `it` the wave's chunk `it` starts its search (the register round,
  //      then the first gather), chunk it - 1 takes its second gather, chunk it - 2 stages its
  //      window, chunk it - 3 loads its rows and chunk it - 4 stores them; every value an iteration
  //      uses was requested by the one before it.  (Searching, staging and loading one chunk after
  //      the other, four dependent round trips each, ran as long as k_final_dst.)
  const uint32_t mine = t_first < nfull ? (nfull - 1 - t_first) / g + 1 : 0u;   // the wave's full chunks
  uint32_t a_lo = 0, a_hi = 0, a_step = 0, a_val = 0, b_lo = 0, b_hi = 0, b_step = 0, b_val = 0;
  bool a_pend = false, b_pend = false;
  uint32_t s_kb = 0, s_x0 = 0, s_x1 = 0, s_rr = 0;
  row2 cur[CI];
#pragma unroll
  for (int i = 0; i < CI; ++i) cur[i] = row2{0, 0};
  for (uint32_t it = 0; mine && it < mine + 4; ++it) {   // (wave-uniform conditions throughout)
    if (it >= 4) store_chunk(cur, t_first + (it - 4) * g);
    if (it >= 3 && it < mine + 3) fetch(t_first + (it - 3) * g, s_kb, s_x0, s_x1, s_rr, cur);
    if (it >= 2 && it < mine + 2) {
      if (b_pend) narrow(&b_lo, &b_hi, b_step, b_val, (t_first + (it - 2) * g) * CH);
      s_kb = b_lo;
      stage(s_kb, &s_x0, &s_x1, &s_rr);
    }
    if (it >= 1 && it < mine + 1) {
      b_lo = a_lo;
      b_hi = a_hi;
      if (a_pend) narrow(&b_lo, &b_hi, a_step, a_val, (t_first + (it - 1) * g) * CH);
      b_pend = b_hi - b_lo > 64;
      if (b_pend) {
        b_step = (b_hi - b_lo + 63) / 64;
        b_val = probe(b_lo, b_hi, b_step);
      }
    }
    if (it < mine) {
      begin((t_first + it * g) * CH, &a_lo, &a_hi);
      a_pend = a_hi - a_lo > 64;
      if (a_pend) {
        a_step = (a_hi - a_lo + 63) / 64;
        a_val = probe(a_lo, a_hi, a_step);
      }
    }
  }
  // ---- the list's last rows: the only chunk with predicated stores
  const uint32_t rem = total - nfull * CH;
  if (rem && t_first == nfull % g) {   // (wave-uniform)
    const uint32_t r0 = nfull * CH;
    const uint32_t kb = bracket(r0);
    uint32_t x0, x1, rr, st, en, rs, idx[2 * CI];
    stage(kb, &x0, &x1, &rr);
    window(kb, x0, x1, rr, &st, &en, &rs);
    const bool ok = resolve(kb, r0, rem, st, en, rs, idx);
    if (!ok && lane == 0) atomicOr(a.err_flag, SPLIT_BAD);
    int64_t v[2 * CI];
#pragma unroll
    for (int i = 0; i < 2 * CI; ++i) v[i] = ld(a.dst_vid + idx[i]);
#pragma unroll
    for (int i = 0; i < CI; ++i) {
      const uint32_t p = (uint32_t)(i * 128 + 2 * lane);
      if (ok && p < rem) out[(uint64_t)r0 + p] = v[2 * i];
      if (ok && p + 1 < rem) out[(uint64_t)r0 + p + 1] = v[2 * i + 1];
    }
  }
  if (a.full_rp) {   // (uniform) E_N over the unfiltered rows: 64 frontier entries per wave and round
    // (folded into the chunk pipeline, a round's ids, offsets and sum one iteration apart, the solo
    // launch measured 118.7-121.4 us against 113.7 us with this loop)
    unsigned long long sum = 0;
    for (uint64_t i = (uint64_t)t_first * 64 + lane; i < n; i += (uint64_t)g * 64) {
      const uint32_t v = a.ids[i];
      if (v != NO_ROW && (!a.visible || a.visible[v])) sum += a.full_rp[v + 1] - a.full_rp[v];
    }
    for (int o = 32; o; o >>= 1) sum += __shfl_down(sum, o, 64);
    if (lane == 0 && sum) atomicAdd(a.stat_e, sum);
  }
  // one segment: the host reads workgroup 0's count as the run's length
  if (threadIdx.x == 0) a.blk_rows[blockIdx.x] = blockIdx.x == 0 ? total : 0u;
}

hipError_t launch_final_copy(const FinalCopyArgs& a, unsigned grid, hipStream_t s) {
  hipLaunchKernelGGL(k_final_copy, dim3(grid), dim3(CB), 0, s, a);
  return hipGetLastError();
}

}  // namespace nbg
