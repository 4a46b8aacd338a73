// nebula_amd — the read side of RowSetWriter bytes (nbg_rows_decode: rowdec.hip, stages.cpp): the
// host walk that finds and validates every row's start, and the cell reader the host and the
// kernel share.  What RowSetReader and RowReader do per row (RowSetReader.cpp, RowReader.cpp:
// 213-258).  Nothing here calls HIP, so a stand-alone program can run all of it under a host
// sanitizer (tests/host/rowdec_host.cpp).
// Every read is bounded by the row's end, and a row's end by the length of the buffer.
#pragma once
#include <cstdint>
#include <vector>

#ifndef NBG_HD
#if defined(__HIPCC__)
#define NBG_HD __host__ __device__
#else
#define NBG_HD
#endif
#endif

namespace nbg {

constexpr uint64_t RD_CHUNK = 2048;   // rows per chunk (OB_CHUNK, nbg_internal.h): one 8-byte start each
// NBG_T_* (include/nbg.h), restated so that this header stands alone
constexpr uint32_t RD_T_BOOL = 1, RD_T_INT = 2, RD_T_VID = 3, RD_T_FLOAT = 4, RD_T_DOUBLE = 5, RD_T_STRING = 6,
                   RD_T_TIMESTAMP = 7;

// folly::decodeVarint bounded by `end`: at most 10 bytes, read as uint64_t (the 10th byte's bits
// above bit 63 fall off).  False: the bytes end inside it, or an 11th byte would follow.
NBG_HD inline bool rd_varint(const uint8_t* bytes, uint64_t end, uint64_t* pos, uint64_t* v) {
  uint64_t p = *pos, x = 0;
  for (uint32_t k = 0; k < 10; ++k) {
    if (p >= end) return false;
    const uint8_t b = bytes[p++];
    x |= (uint64_t)(b & 0x7Fu) << (7 * k);
    if (!(b & 0x80u)) {
      *pos = p;
      *v = x;
      return true;
    }
  }
  return false;
}

// The row header at *pos (RowReader.cpp:213-241): the header byte — offsetBytes - 1 in its low 3
// bits, the count of schema-version bytes in its top 3 — the version bytes and ncols >> 4 block
// offsets of offsetBytes each.  Leaves *pos at the cord's first byte.  False: the row is empty or
// shorter than its header.
NBG_HD inline bool rd_header(const uint8_t* bytes, uint64_t row_end, int ncols, uint64_t* pos) {
  if (*pos >= row_end) return false;
  const uint8_t h = bytes[*pos];
  const uint64_t hdr = 1 + (uint64_t)(h >> 5) + (uint64_t)((uint32_t)ncols >> 4) * ((h & 7u) + 1u);
  if (hdr > row_end - *pos) return false;
  *pos += hdr;
  return true;
}

// One cell: its 8-byte payload, or the span of a string's bytes.
struct RdCell {
  uint64_t bits = 0;     // INT / TIMESTAMP / VID the value, DOUBLE its bits, BOOL 0 / 1
  uint64_t str_at = 0;   // STRING: the bytes are bytes[str_at, str_at + str_len)
  uint64_t str_len = 0;
};
// Reads the cell of NBG_T_* `type` at *pos and moves *pos past it (RowReader.cpp:243-258 skipToNext
// and the getters).  False: the cell would read past row_end, a varint has more than 10 bytes, or
// the type has no reader here (FLOAT); *pos is then unchanged.
NBG_HD inline bool rd_cell(const uint8_t* bytes, uint64_t row_end, uint32_t type, uint64_t* pos, RdCell* out) {
  uint64_t p = *pos;
  switch (type) {
    case RD_T_INT:
    case RD_T_TIMESTAMP:
      if (!rd_varint(bytes, row_end, &p, &out->bits)) return false;
      break;
    case RD_T_VID:
    case RD_T_DOUBLE: {
      if (p > row_end || row_end - p < 8) return false;
      uint64_t x = 0;
      for (uint32_t k = 0; k < 8; ++k) x |= (uint64_t)bytes[p + k] << (8 * k);
      out->bits = x;
      p += 8;
      break;
    }
    case RD_T_BOOL:
      if (p >= row_end) return false;
      out->bits = bytes[p++] != 0;
      break;
    case RD_T_STRING: {
      uint64_t n = 0;
      if (!rd_varint(bytes, row_end, &p, &n) || n > row_end - p) return false;
      out->str_at = p;
      out->str_len = n;
      p += n;
      break;
    }
    default:
      return false;
  }
  *pos = p;
  return true;
}

// What the walk found.  The scope limits come before the malformations, whichever the walk met
// first (nbg.h, nbg_rows_decode's statuses 4 and 5).
enum RdWalkStatus : int32_t {
  RD_WALK_OK = 0,
  RD_WALK_ROWS,        // 2^32 rows or more
  RD_WALK_CHUNK,       // a chunk of RD_CHUNK rows whose bytes reach 4 GiB
  RD_WALK_PREFIX,      // a length prefix over 10 bytes or running past len
  RD_WALK_PAST_END,    // a row running past len
  RD_WALK_EMPTY_ROW,   // a row of length 0: it has no header byte
  RD_WALK_HEADER,      // a row shorter than its own header
};
struct RdIndex {
  uint64_t rows = 0;
  std::vector<uint64_t> chunk_start;   // [ceil(rows / RD_CHUNK)] the first byte of the chunk's first row (its prefix)
  std::vector<uint32_t> row_off;       // [rows] the row's first byte (its prefix), from its chunk's start
  RdWalkStatus status = RD_WALK_OK;
  uint64_t bad_row = 0, bad_at = 0;    // a malformation: the row and the byte it was found at
};
inline bool rd_walk_malformed(RdWalkStatus s) { return s >= RD_WALK_PREFIX; }

// The length-prefix chain of (data, len) under a schema of ncols fields: RowSetReader's iteration,
// with RowReader's header check per row.
inline RdIndex rd_walk(const uint8_t* data, uint64_t len, int ncols) {
  RdIndex ix;
  bool too_many = false, chunk_big = false;
  RdWalkStatus bad = RD_WALK_OK;
  uint64_t pos = 0, cstart = 0;
  // (room for rows of 8 bytes and more without a reallocation; untouched pages cost nothing)
  if (len) ix.row_off.reserve((size_t)(len / 8 < 1024 ? 1024 : len / 8));
  while (pos < len) {
    const uint64_t at = pos;
    uint64_t n = 0;
    if (!rd_varint(data, len, &pos, &n)) bad = RD_WALK_PREFIX;
    else if (n > len - pos) bad = RD_WALK_PAST_END;
    else if (!n) bad = RD_WALK_EMPTY_ROW;
    else {
      uint64_t h = pos;
      if (!rd_header(data, pos + n, ncols, &h)) bad = RD_WALK_HEADER;
    }
    if (bad) {
      ix.bad_row = ix.rows;
      ix.bad_at = at;
      break;
    }
    if (ix.rows >= 0xFFFFFFFFull) too_many = true;
    if (!too_many && !chunk_big) {
      if (ix.rows % RD_CHUNK == 0) {
        cstart = at;
        ix.chunk_start.push_back(at);
      }
      if (pos + n - cstart > 0xFFFFFFFFull) chunk_big = true;   // (so every offset fits 32 bits)
      else ix.row_off.push_back((uint32_t)(at - cstart));
    }
    ++ix.rows;
    pos += n;
  }
  ix.status = too_many ? RD_WALK_ROWS : chunk_big ? RD_WALK_CHUNK : bad;
  return ix;
}

}  // namespace nbg
