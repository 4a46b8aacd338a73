// nebula_amd — device-resident rows from RowSetWriter bytes (gfx950, wave64): the inverse of
// rowenc.hip.  What InterimResult::getRows / buildIndex do with a RowReader per row
// (InterimResult.cpp:74-140, 158-250; RowReader.cpp:213-258; RowSetReader.cpp): every row is
//   varint(len(row)) [header byte] [version bytes] [ncols >> 4 block offsets] cord
// and the cord the cells by the column's type: INT / TIMESTAMP a varint, VID and DOUBLE 8 bytes,
// BOOL one byte, STRING varint(length) + bytes.
// The length-prefix chain is sequential, so the host walks it (rowdec.h rd_walk) and uploads, with
// the bytes, one 8-byte start per chunk of OB_CHUNK rows and each row's 32-bit offset from it.
//   k_rd_cells   one workgroup per chunk, tiles of BLOCK rows, one lane per row: the lane walks its
//                row's header and cells with rd_cell (rowdec.h, the function the host program
//                proves) and stores each column's 8-byte payload at its row index; a STRING cell is
//                a binary search of the dictionary and becomes its code
// The row bytes are read straight from global memory: a wave's rows are adjacent.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>
#include <string>

#include "stage.h"
#include "ws.h"
#include "rowdec.h"

namespace nbg {

const char* const kRdKernelNames[RD_KINDS] = {"rd_host_walk", "rd_host_upload", "k_rd_cells"};

static_assert(RD_CHUNK == OB_CHUNK, "rowdec.h restates OB_CHUNK");
static_assert(RD_T_BOOL == NBG_T_BOOL && RD_T_INT == NBG_T_INT && RD_T_VID == NBG_T_VID && RD_T_FLOAT == NBG_T_FLOAT &&
                  RD_T_DOUBLE == NBG_T_DOUBLE && RD_T_STRING == NBG_T_STRING && RD_T_TIMESTAMP == NBG_T_TIMESTAMP,
              "rowdec.h restates NBG_T_*");

namespace {

struct RdArgs {
  const uint8_t* data;              // the RowSetWriter bytes
  uint64_t len;
  const uint64_t* cstart;           // [nchunks] the first byte of the chunk's first row
  const uint32_t* roff;             // [rows] the row's first byte from its chunk's start
  uint64_t rows;
  uint32_t nchunks;
  int ncols;
  uint64_t types[2];                // NBG_T_* of column c: 4 bits at 4 * (c & 15) of types[c >> 4]
  const uint32_t* soff;             // the dictionary: string i is sbytes[soff[i], soff[i + 1])
  const char* sbytes;
  uint64_t sn;
  int64_t* out[MAX_YIELDS];
  RdRecord* rec;
};

__device__ __forceinline__ uint32_t rd_type(const RdArgs& a, int c) {
  return (uint32_t)((c < 16 ? a.types[0] : a.types[1]) >> (4 * (c & 15))) & 15u;
}

// The code of the string s[0, n) as every stage reads it (string_code, exprc.cpp): 2 x its index
// in the sorted dictionary; the empty string the dictionary lacks is -1, i.e. 2 x 0 - 1.  The order
// is std::string's: by unsigned bytes, then by length.  *found is false for every other miss.
__device__ __forceinline__ int64_t rd_string_code(const RdArgs& a, const uint8_t* s, uint64_t n, bool* found) {
  uint64_t lo = 0, hi = a.sn;
  while (lo < hi) {   // the first entry not below s
    const uint64_t mid = (lo + hi) >> 1;
    const uint32_t o = a.soff[mid], m = a.soff[mid + 1] - o;
    const uint8_t* d = reinterpret_cast<const uint8_t*>(a.sbytes) + o;
    const uint64_t common = m < n ? m : n;
    int cmp = 0;
    for (uint64_t i = 0; i < common && !cmp; ++i) cmp = (int)d[i] - (int)s[i];
    if (cmp < 0 || (!cmp && m < n)) lo = mid + 1;
    else hi = mid;
  }
  *found = true;
  if (lo < a.sn) {
    const uint32_t o = a.soff[lo], m = a.soff[lo + 1] - o;
    if (m == n) {
      const uint8_t* d = reinterpret_cast<const uint8_t*>(a.sbytes) + o;
      bool same = true;
      for (uint64_t i = 0; i < n && same; ++i) same = d[i] == s[i];
      if (same) return 2 * (int64_t)lo;
    }
  }
  if (!n) return -1;
  *found = false;
  return 0;
}

__global__ void __launch_bounds__(BLOCK) k_rd_cells(const RdArgs a) {
  for (uint32_t k = blockIdx.x; k < a.nchunks; k += gridDim.x) {
    const uint64_t base = a.cstart[k], r0 = (uint64_t)k * OB_CHUNK;
    const uint64_t nr = a.rows - r0 < OB_CHUNK ? a.rows - r0 : OB_CHUNK;
    for (uint64_t i = threadIdx.x; i < nr; i += BLOCK) {   // a tile of BLOCK rows, one lane per row
      const uint64_t row = r0 + i;
      uint64_t pos = base + a.roff[row], n = 0;
      // the host walk vouches for the prefix, the row's end and its header; they are read again
      // through the same bounded functions, so a row that did not hold reads nothing outside `len`
      int bad = -1;
      uint64_t end = pos;
      if (!rd_varint(a.data, a.len, &pos, &n) || n > a.len - pos) bad = 0;
      else {
        end = pos + n;
        if (!rd_header(a.data, end, a.ncols, &pos)) bad = 0;
      }
      uint32_t missing = 0;
      for (int c = 0; c < a.ncols; ++c) {
        RdCell cell;
        const uint32_t t = rd_type(a, c);
        if (bad < 0 && !rd_cell(a.data, end, t, &pos, &cell)) bad = c;
        int64_t v = 0;
        if (bad < 0) {
          v = (int64_t)cell.bits;
          if (t == NBG_T_STRING) {
            bool found;
            v = rd_string_code(a, a.data + cell.str_at, cell.str_len, &found);
            missing += !found;
          }
        }
        a.out[c][row] = v;   // (a wave's stores to a column: 512 contiguous bytes)
      }
      if (bad >= 0) {
        atomicAdd(&a.rec->malformed, 1ull);
        atomicMin(&a.rec->first, (unsigned long long)(row * 64 + (uint64_t)bad));
      }
      if (missing) atomicAdd(&a.rec->missing, (unsigned long long)missing);
    }
  }
}

constexpr uint64_t rd_align8(uint64_t x) { return (x + 7) & ~7ull; }

}  // namespace

// the pinned block and its device copy: [bytes, padded to 8][chunk starts][row offsets]
uint64_t rd_block_bytes(uint64_t len, uint64_t nchunks, uint64_t rows) { return rd_align8(len) + nchunks * 8 + rows * 4; }

int32_t ws_rows_decode(hipStream_t stream, const uint8_t* data, uint64_t len, const uint64_t* chunk_start, uint64_t nchunks,
                       const uint32_t* row_off, uint64_t rows, void* block, const RdPlan& plan, Workspace** outw,
                       RdRecord* rec, StageProf<RD_KINDS>* prof, std::string* err) {
  *outw = nullptr;
  StageStatus cs("rows decode");
  if (plan.ncols < 1 || plan.ncols > MAX_YIELDS || !rows || rows > 0xFFFFFFFFull || !len || !block ||
      nchunks != (rows + OB_CHUNK - 1) / OB_CHUNK) {
    if (err) *err = "rows decode: empty input or plan";
    return NBG_E_INVALID_ARGUMENT;
  }

  RowsWs res;
  if (cs.failed(res.reserve(stream, rows, plan.ncols), "result rows")) return cs.code(err);

  StageScratch sc;   // (declared before the timer: the timer's events are resolved first)
  StageTimer<RD_KINDS> tm{prof, stream, {}, nullptr};
  const uint64_t total = rd_block_bytes(len, nchunks, rows), at_chunks = rd_align8(len), at_rows = at_chunks + nchunks * 8;
  uint8_t* dev = nullptr;
  RdRecord* d_rec = nullptr;
  const RdRecord clear;
  if (cs.failed(sc.alloc((void**)&dev, total), "row bytes") || cs.failed(sc.alloc((void**)&d_rec, sizeof(RdRecord)), "record"))
    return cs.code(err);
  // ---- the pinned copy and one DMA
  const auto t0 = std::chrono::steady_clock::now();
  uint8_t* host = static_cast<uint8_t*>(block);
  std::memcpy(host, data, len);
  std::memset(host + len, 0, at_chunks - len);
  std::memcpy(host + at_chunks, chunk_start, nchunks * 8);
  std::memcpy(host + at_rows, row_off, rows * 4);
  if (cs.failed(hipMemcpyAsync(dev, host, total, hipMemcpyHostToDevice, stream), "row bytes upload") ||
      cs.failed(hipMemcpyAsync(d_rec, &clear, sizeof(RdRecord), hipMemcpyHostToDevice, stream), "record clear"))
    return cs.code(err);
  if (tm.on()) {   // (only the profile waits here: the kernel is ordered behind the DMA by the stream)
    if (cs.failed(hipStreamSynchronize(stream), "upload")) return cs.code(err);
    prof->launches[RD_K_UPLOAD]++;
    prof->ms[RD_K_UPLOAD] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    prof->bytes[RD_K_UPLOAD] += (double)total;
  }

  RdArgs a{};
  a.data = dev;
  a.len = len;
  a.cstart = reinterpret_cast<const uint64_t*>(dev + at_chunks);
  a.roff = reinterpret_cast<const uint32_t*>(dev + at_rows);
  a.rows = rows;
  a.nchunks = (uint32_t)nchunks;
  a.ncols = plan.ncols;
  uint64_t cells = 0;
  for (int c = 0; c < plan.ncols; ++c) {
    a.types[c >> 4] |= (uint64_t)(plan.type[c] & 15) << (4 * (c & 15));
    a.out[c] = ws_row_col(res.w, c);
    cells += rows;
  }
  a.soff = plan.str.off;
  a.sbytes = plan.str.bytes;
  a.sn = plan.str.off && plan.str.bytes ? plan.str.n : 0;
  a.rec = d_rec;

  const unsigned grid = (unsigned)std::min<uint64_t>(nchunks, STAGE_GRID);
  tm.begin();
  hipLaunchKernelGGL(k_rd_cells, dim3(grid), dim3(BLOCK), 0, stream, a);
  tm.end(RD_K_CELLS, (double)total + 8.0 * (double)cells);
  if (cs.failed(hipGetLastError(), "k_rd_cells") ||
      cs.failed(hipMemcpyAsync(rec, d_rec, sizeof(RdRecord), hipMemcpyDeviceToHost, stream), "record read") ||
      cs.failed(hipStreamSynchronize(stream), "cells"))
    return cs.code(err);
  *outw = res.release();
  return NBG_OK;
}

}  // namespace nbg
