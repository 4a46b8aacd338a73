// nebula_amd — RowSetWriter bytes of a device-resident result (gfx950, wave64).
// What graphd's InterimResult holds beside its schema (GoExecutor.cpp:707-779,
// InterimResult.cpp:602-640): for every row, in fetch order, varint(len(row)) + row, with
//   row = [offsetBytes - 1] [cord size after column 16, after column 32: offsetBytes each, LE] cord
// (RowWriter.cpp:26-95 with schema version 0, RowSetWriter.cpp:21-33) and the cord the cells as
// RowWriter::operator<< writes them for the column's type (RowWriter.inl:9-45): INT / TIMESTAMP a
// varint of the payload as uint64, VID and DOUBLE the 8 payload bytes, BOOL one byte, STRING
// varint(length) + bytes.
//   k_re_size   one lane per row: the row's encoded length, and each chunk's byte sum
//   k_re_scan   exclusive scan of the chunk sums into chunk bases and the total (one workgroup)
//   k_re_emit   one workgroup per chunk: tiles of RE_TILE rows are encoded into an LDS staging
//               buffer and streamed to the output 16 bytes per lane; a tile that does not fit it
//               is cut into its waves' 64 rows, each staged the same way when it fits (wide
//               numeric rows) and else stored directly, a wave per row (long strings)
// The input is walked through the chunk list of stage.h, one workgroup per chunk.  No kernel waits
// on another workgroup: every dependency is a kernel boundary on one stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "stage.h"
#include "ws.h"

namespace nbg {

const char* const kReKernelNames[RE_KINDS] = {"k_re_size", "k_re_scan", "k_re_emit"};

namespace {

constexpr int RE_TILE = BLOCK;   // rows of one tile: one per lane

struct ReArgs {
  const uint64_t* chunk;            // stage_chunks' list: (first physical row, rows, first logical row)
  const uint8_t* chunk_type;        // the OVER position of each chunk
  uint32_t nchunks;
  const int64_t* const* cols;       // the input's column bases (device array)
  int ncols;
  uint64_t types[2];                // NBG_T_* of column c: 4 bits at 4 * (c & 15) of types[c >> 4]
  const uint32_t* soff;             // the dictionary: string i is sbytes[soff[i], soff[i + 1])
  const char* sbytes;
  uint64_t sn;
  const uint32_t* koff;             // the constants outside it: entry OVER position * ncols + column
  const char* kbytes;
  uint32_t* rlen;                   // [rows] a row's bytes in the output, its length prefix included
  uint64_t* csum;                   // [nchunks] the chunk's bytes
  const uint64_t* cbase;            // [nchunks] the chunk's first output byte
  uint8_t* out;
};

struct ReStr {
  const char* p;
  uint32_t n;
};
// A string cell: an even, non-negative code inside the dictionary is the dictionary's string;
// every other code spells the constant of the cell's (OVER position, column) — as nbg_rows_fetch
// reads it (engine.cpp materialize_rows).
__device__ __forceinline__ ReStr re_string(const ReArgs& a, int64_t code, uint32_t kentry) {
  if (code >= 0 && !(code & 1) && (uint64_t)(code >> 1) < a.sn) {
    const uint32_t o = a.soff[code >> 1];
    return ReStr{a.sbytes + o, a.soff[(code >> 1) + 1] - o};
  }
  const uint32_t o = a.koff[kentry];
  return ReStr{a.kbytes + o, a.koff[kentry + 1] - o};
}

// folly::encodeVarint's length: 7 payload bits per byte, from the leading-zero count
__device__ __forceinline__ uint32_t varint_len(uint64_t v) { return (uint32_t)(70 - __builtin_clzll(v | 1)) / 7u; }
// calcOccupiedBytes (RowWriter.cpp:77-85): the bytes that hold v, at least one
__device__ __forceinline__ uint32_t occupied_bytes(uint64_t v) { return (uint32_t)(71 - __builtin_clzll(v | 1)) / 8u; }

__device__ __forceinline__ uint32_t re_type(const ReArgs& a, int c) {
  return (uint32_t)((c < 16 ? a.types[0] : a.types[1]) >> (4 * (c & 15))) & 15u;
}

// A cell that is no string, as the n bytes it is written in: byte k is ((v >> shift * k) & mask),
// with `more` set in every byte but the last.  A varint has 7 payload bits per byte and the
// continuation bit; VID and DOUBLE are the 8 payload bytes; BOOL is one byte, 0 or 1.
struct ReCell {
  uint64_t v;
  uint32_t n, shift, mask, more;
};
__device__ __forceinline__ ReCell re_cell(uint32_t t, int64_t v) {
  const bool fixed = t == NBG_T_VID || t == NBG_T_DOUBLE, flag = t == NBG_T_BOOL;
  ReCell x;
  x.v = flag ? (uint64_t)(v != 0) : (uint64_t)v;
  x.n = fixed ? 8u : flag ? 1u : varint_len(x.v);
  x.shift = fixed || flag ? 8u : 7u;
  x.mask = fixed || flag ? 0xFFu : 0x7Fu;
  x.more = fixed || flag ? 0u : 0x80u;
  return x;
}

struct ReDims {
  uint64_t cord;         // the cells' bytes
  uint64_t off0, off1;   // the cord's size after column 16 and after column 32
  uint32_t noff, ob;     // block offsets and their width (offsetBytes)
  uint64_t len;          // header + offsets + cord: what the prefix encodes
  __device__ uint64_t total() const { return varint_len(len) + len; }
};
__device__ __forceinline__ ReDims re_measure(const ReArgs& a, uint64_t row, uint32_t kbase) {
  ReDims d{};
  for (int c = 0; c < a.ncols; ++c) {
    const int64_t v = a.cols[c][row];
    const uint32_t t = re_type(a, c);
    if (t == NBG_T_STRING) {
      const uint32_t n = re_string(a, v, kbase + c).n;
      d.cord += varint_len(n) + n;
    } else {
      d.cord += re_cell(t, v).n;
    }
    if (c == 15) d.off0 = d.cord;
    if (c == 31) d.off1 = d.cord;
  }
  d.noff = (uint32_t)a.ncols >> 4;   // (ncols <= 32: at most two)
  d.ob = occupied_bytes(d.cord);
  d.len = 1 + (uint64_t)d.noff * d.ob + d.cord;
  return d;
}

// The bytes of one row into `put`: put.byte(b) appends one byte, put.bytes(p, n) a string's.  Both
// paths of k_re_emit go through this one walk, so they cannot write different bytes.
template <class Put>
__device__ __forceinline__ void put_cell(Put& put, const ReCell& x) {
  for (uint32_t k = 0; k < x.n; ++k)
    put.byte((uint8_t)(((x.v >> (x.shift * k)) & x.mask) | (k + 1 < x.n ? x.more : 0u)));
}
template <class Put>
__device__ __forceinline__ void put_varint(Put& put, uint64_t v) { put_cell(put, re_cell(NBG_T_INT, (int64_t)v)); }
template <class Put>
__device__ __forceinline__ void re_write(const ReArgs& a, uint64_t row, uint32_t kbase, const ReDims& d, Put& put) {
  put_varint(put, d.len);
  put.byte((uint8_t)(d.ob - 1));
  if (d.noff > 0) put_cell(put, ReCell{d.off0, d.ob, 8u, 0xFFu, 0u});
  if (d.noff > 1) put_cell(put, ReCell{d.off1, d.ob, 8u, 0xFFu, 0u});
  for (int c = 0; c < a.ncols; ++c) {
    const int64_t v = a.cols[c][row];
    const uint32_t t = re_type(a, c);
    if (t == NBG_T_STRING) {
      const ReStr s = re_string(a, v, kbase + c);
      put_varint(put, s.n);
      put.bytes(s.p, s.n);
    } else {
      put_cell(put, re_cell(t, v));
    }
  }
}

struct PutLds {            // one lane writes its row into the staging buffer
  uint8_t* at;
  __device__ __forceinline__ void byte(uint8_t b) { *at++ = b; }
  __device__ __forceinline__ void bytes(const char* p, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) at[i] = (uint8_t)p[i];
    at += n;
  }
};
struct PutWave {           // a wave writes one row to the output: lane 0 the cells' own bytes, the
  uint8_t* at;             // 64 lanes a string's, each a byte of every 64-byte run
  int lane;
  __device__ __forceinline__ void byte(uint8_t b) {
    if (lane == 0) *at = b;
    ++at;
  }
  __device__ __forceinline__ void bytes(const char* p, uint32_t n) {
    for (uint32_t i = (uint32_t)lane; i < n; i += 64) at[i] = (uint8_t)p[i];
    at += n;
  }
};

__device__ __forceinline__ uint64_t wave_incl_scan64(uint64_t v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t t = (uint64_t)__shfl_up((unsigned long long)v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}
// block_excl_scan (ws.h) over 64-bit values
__device__ __forceinline__ uint64_t block_excl_scan64(uint64_t v, uint64_t* total, uint64_t* lds) {
  const uint64_t inc = wave_incl_scan64(v);
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 63) lds[w] = inc;
  __syncthreads();
  uint64_t pre = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < WAVES; ++i) {
    const uint64_t s = lds[i];
    pre += (i < w) ? s : 0ull;
    tot += s;
  }
  __syncthreads();
  *total = tot;
  return pre + inc - v;
}

__global__ void __launch_bounds__(BLOCK) k_re_size(const ReArgs a) {
  __shared__ uint64_t lds[WAVES];
  for (uint32_t k = blockIdx.x; k < a.nchunks; k += gridDim.x) {
    const uint64_t first = a.chunk[3 * k], rows = a.chunk[3 * k + 1], logical = a.chunk[3 * k + 2];
    const uint32_t kbase = (uint32_t)a.chunk_type[k] * (uint32_t)a.ncols;
    uint64_t sum = 0;
    for (uint64_t i = threadIdx.x; i < rows; i += BLOCK) {
      const uint64_t t = re_measure(a, first + i, kbase).total();
      a.rlen[logical + i] = (uint32_t)t;
      sum += t;
    }
    uint64_t total = 0;
    (void)block_excl_scan64(sum, &total, lds);
    if (threadIdx.x == 0) a.csum[k] = total;
  }
}

// base[k] = sum of sum[0..k), *total = the sum of all; each thread scans a contiguous slice
// (k_yr_scan's shape over 64-bit sums)
__global__ void __launch_bounds__(BLOCK) k_re_scan(const uint64_t* __restrict__ sum, uint32_t n, uint64_t* __restrict__ base,
                                                   uint64_t* __restrict__ total) {
  __shared__ uint64_t lds[WAVES];
  const uint32_t per = (n + BLOCK - 1) / BLOCK;
  const uint64_t first = (uint64_t)threadIdx.x * per;
  const uint32_t lo = first < n ? (uint32_t)first : n;
  const uint32_t hi = first + per < n ? (uint32_t)(first + per) : n;
  uint64_t s = 0;
  for (uint32_t i = lo; i < hi; ++i) s += sum[i];
  uint64_t tot = 0;
  uint64_t run = block_excl_scan64(s, &tot, lds);
  for (uint32_t i = lo; i < hi; ++i) {
    base[i] = run;
    run += sum[i];
  }
  if (threadIdx.x == 0) *total = tot;
}

__global__ void __launch_bounds__(BLOCK) k_re_emit(const ReArgs a) {
  // the staging buffer: byte p of it is output byte (tile base - pad) + p, pad the tile base's
  // offset in its 16-byte line, so a 16-byte slot of LDS is a 16-byte line of the output
  __shared__ __attribute__((aligned(16))) uint8_t stage[RE_STAGE_BYTES];
  __shared__ uint64_t lds[WAVES];
  __shared__ uint64_t wstart[WAVES + 1];   // a cut tile: the first byte of each wave's rows, then the tile's size
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (uint32_t k = blockIdx.x; k < a.nchunks; k += gridDim.x) {
    const uint64_t first = a.chunk[3 * k], rows = a.chunk[3 * k + 1], logical = a.chunk[3 * k + 2];
    const uint32_t kbase = (uint32_t)a.chunk_type[k] * (uint32_t)a.ncols;
    uint64_t tbase = a.cbase[k];   // the tile's first output byte
    for (uint64_t t0 = 0; t0 < rows; t0 += RE_TILE) {
      const uint64_t i = t0 + threadIdx.x;
      const bool live = i < rows;
      const uint64_t mine = live ? a.rlen[logical + i] : 0;
      uint64_t tile = 0;
      const uint64_t at = block_excl_scan64(mine, &tile, lds);   // (its barriers also fence the last tile's reads of `stage`)
      // A tile that fits the buffer is one staged part; a larger one is cut into its waves' 64 rows,
      // each staged when it fits (wide numeric rows) and stored directly when not (long strings).
      const bool whole = (tbase & 15) + tile <= RE_STAGE_BYTES;   // (workgroup-uniform, as all below)
      if (!whole) {
        if (lane == 0) wstart[wave] = at;
        if (threadIdx.x == 0) wstart[WAVES] = tile;
        __syncthreads();
      }
      for (int s = 0; s < (whole ? 1 : WAVES); ++s) {
        const uint64_t p0 = whole ? 0 : wstart[s];             // the part's first byte in the tile
        const uint64_t pbytes = (whole ? tile : wstart[s + 1]) - p0;
        const uint64_t pbase = tbase + p0;
        const uint32_t pad = (uint32_t)(pbase & 15);
        const bool mine_here = whole || wave == s;
        if (pad + pbytes <= RE_STAGE_BYTES) {
          if (live && mine_here) {
            PutLds put{stage + pad + (uint32_t)(at - p0)};
            re_write(a, first + i, kbase, re_measure(a, first + i, kbase), put);
          }
          __syncthreads();
          const uint32_t end = pad + (uint32_t)pbytes;
          uint8_t* const line0 = a.out + (pbase - pad);
          for (uint32_t p = threadIdx.x * 16; p < end; p += BLOCK * 16) {
            if (p >= pad && p + 16 <= end) {
              *reinterpret_cast<uint4*>(line0 + p) = *reinterpret_cast<const uint4*>(stage + p);
            } else {   // the part's unaligned head and tail: the neighbours' bytes of the line are not ours
              const uint32_t q1 = p + 16 < end ? p + 16 : end;
              for (uint32_t q = p < pad ? pad : p; q < q1; ++q) line0[q] = stage[q];
            }
          }
          __syncthreads();   // (the next part overwrites `stage`)
        } else if (mine_here) {   // (never a whole tile: it would have been cut) the wave's rows, one after the other
          for (int j = 0; j < 64; ++j) {
            const uint64_t rat = (uint64_t)__shfl((unsigned long long)at, j, 64);
            const uint64_t r = t0 + (uint64_t)wave * 64 + j;   // (wave-uniform)
            if (r >= rows) break;
            PutWave put{a.out + tbase + rat, lane};
            re_write(a, first + r, kbase, re_measure(a, first + r, kbase), put);
          }
        }
      }
      tbase += tile;
    }
  }
}

}  // namespace

int32_t ws_rows_encode(Workspace* inw, hipStream_t stream, const std::vector<std::pair<uint64_t, uint64_t>>& segs,
                       const RePlan& plan, void* (*grow)(void* ctx, uint64_t bytes), void* ctx, uint64_t* len,
                       StageProf<RE_KINDS>* prof, std::string* err) {
  *len = 0;
  StageStatus cs("rows encode");
  uint64_t n = 0;
  for (auto& sg : segs) n += sg.second;
  if (plan.ncols < 1 || plan.ncols > MAX_YIELDS || !n || n > 0xFFFFFFFFull) {
    if (err) *err = "rows encode: empty input or plan";
    return NBG_E_INVALID_ARGUMENT;
  }

  StageScratch sc;   // (declared before the timer: the timer's events are resolved first)
  StageTimer<RE_KINDS> tm{prof, stream, {}, nullptr};
  StageChunks ch;
  if (ch.upload(cs, sc, stream, segs, 0, n)) return cs.code(err);
  if (plan.chunk_type.size() != ch.n || plan.koff.empty()) {
    if (err) *err = "rows encode: the chunk list and its OVER positions disagree";
    return NBG_E_DEVICE;
  }
  ReArgs a{};
  uint8_t* ctype = nullptr;
  uint32_t* koff = nullptr;
  char* kbytes = nullptr;
  uint64_t* csum = nullptr;
  uint64_t* cbase = nullptr;
  uint64_t* total = nullptr;
  if (cs.failed(sc.alloc((void**)&ctype, ch.n), "chunk types") ||
      cs.failed(sc.alloc((void**)&koff, plan.koff.size() * 4), "constant offsets") ||
      cs.failed(sc.alloc((void**)&kbytes, plan.kbytes.size()), "constant bytes") ||
      cs.failed(sc.alloc((void**)&a.rlen, n * 4), "row lengths") || cs.failed(sc.alloc((void**)&csum, (size_t)ch.n * 8), "chunk sums") ||
      cs.failed(sc.alloc((void**)&cbase, (size_t)ch.n * 8), "chunk bases") || cs.failed(sc.alloc((void**)&total, 8), "total") ||
      cs.failed(hipMemcpyAsync(ctype, plan.chunk_type.data(), ch.n, hipMemcpyHostToDevice, stream), "chunk type upload") ||
      cs.failed(hipMemcpyAsync(koff, plan.koff.data(), plan.koff.size() * 4, hipMemcpyHostToDevice, stream), "constant upload") ||
      (!plan.kbytes.empty() &&
       cs.failed(hipMemcpyAsync(kbytes, plan.kbytes.data(), plan.kbytes.size(), hipMemcpyHostToDevice, stream), "constant upload")))
    return cs.code(err);
  a.chunk = ch.dev;
  a.chunk_type = ctype;
  a.nchunks = ch.n;
  a.cols = (const int64_t* const*)inw->d_row_cols;
  a.ncols = plan.ncols;
  for (int c = 0; c < plan.ncols; ++c) a.types[c >> 4] |= (uint64_t)(plan.type[c] & 15) << (4 * (c & 15));
  a.soff = plan.str.off;
  a.sbytes = plan.str.bytes;
  a.sn = plan.str.off && plan.str.bytes ? plan.str.n : 0;
  a.koff = koff;
  a.kbytes = kbytes;
  a.csum = csum;
  a.cbase = cbase;

  tm.begin();
  hipLaunchKernelGGL(k_re_size, dim3(ch.grid), dim3(BLOCK), 0, stream, a);
  tm.end(RE_K_SIZE, (double)n * (8.0 * plan.ncols + 4.0));
  if (cs.failed(hipGetLastError(), "k_re_size")) return cs.code(err);
  tm.begin();
  hipLaunchKernelGGL(k_re_scan, dim3(1), dim3(BLOCK), 0, stream, csum, ch.n, cbase, total);
  tm.end(RE_K_SCAN, (double)ch.n * 16.0);
  uint64_t bytes = 0;
  if (cs.failed(hipGetLastError(), "k_re_scan") ||
      cs.failed(hipMemcpyAsync(&bytes, total, 8, hipMemcpyDeviceToHost, stream), "total read") ||
      cs.failed(hipStreamSynchronize(stream), "sizing"))
    return cs.code(err);
  // every row is at least its prefix, its header byte and a byte per cell; at most rlen's 32 bits
  if (bytes < n * (2 + (uint64_t)plan.ncols) || bytes / n > 0xFFFFFFFFull) {
    if (err) *err = "rows encode: " + std::to_string(bytes) + " bytes for " + std::to_string(n) + " rows";
    return NBG_E_DEVICE;
  }

  if (cs.failed(sc.alloc((void**)&a.out, bytes), "encoded rows")) return cs.code(err);
  void* host = grow(ctx, bytes);
  if (!host) {
    if (err) *err = "rows encode: pinned host memory for " + std::to_string(bytes) + " bytes";
    return NBG_E_OUT_OF_MEMORY;
  }
  tm.begin();
  hipLaunchKernelGGL(k_re_emit, dim3(ch.grid), dim3(BLOCK), 0, stream, a);
  tm.end(RE_K_EMIT, (double)n * (8.0 * plan.ncols + 4.0) + (double)bytes);
  if (cs.failed(hipGetLastError(), "k_re_emit") ||
      cs.failed(hipMemcpyAsync(host, a.out, bytes, hipMemcpyDeviceToHost, stream), "encoded rows copy") ||
      cs.failed(hipStreamSynchronize(stream), "emission"))
    return cs.code(err);
  *len = bytes;
  return NBG_OK;
}

}  // namespace nbg
