// Stand-alone check of nbg_rows_decode's host side (nebula_amd/csrc/rowdec.h), built with
// -fsanitize=address,undefined by tests/test_rowdec_host.py: the walk of the length prefixes and
// the cell reader the kernel shares, over well-formed rowsets and over every malformed case.  Each
// input lives in a heap block of exactly its length, so a read past it is an ASan report.  No HIP,
// no GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "rowdec.h"

#define CHECK(x)                                                 \
  do {                                                           \
    if (!(x)) {                                                  \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      return 1;                                                  \
    }                                                            \
  } while (0)

using namespace nbg;
using Bytes = std::vector<uint8_t>;

namespace {

// a writer of this test's own (RowWriter.cpp:26-95, RowSetWriter.cpp:21-33)
void put_varint(Bytes& b, uint64_t v) {
  while (v >= 0x80) {
    b.push_back((uint8_t)(v | 0x80));
    v >>= 7;
  }
  b.push_back((uint8_t)v);
}
void put_le(Bytes& b, uint64_t v, int n) {
  for (int k = 0; k < n; ++k) b.push_back((uint8_t)(v >> (8 * k)));
}
void put_str(Bytes& b, const std::string& s) {
  put_varint(b, s.size());
  b.insert(b.end(), s.begin(), s.end());
}
// header byte (offsetBytes ob, nver version bytes), the version bytes, noff offsets, the cord
Bytes row_of(const Bytes& cord, int ob, int nver, int noff) {
  Bytes r;
  r.push_back((uint8_t)((ob - 1) | (nver << 5)));
  for (int k = 0; k < nver; ++k) r.push_back(0xEE);
  for (int k = 0; k < noff; ++k) put_le(r, 0xABCDEF, ob);
  r.insert(r.end(), cord.begin(), cord.end());
  return r;
}
void add_row(Bytes& set, const Bytes& row) {
  put_varint(set, row.size());
  set.insert(set.end(), row.begin(), row.end());
}

// the input in a heap block of exactly its size
struct Exact {
  std::unique_ptr<uint8_t[]> p;
  uint64_t n;
  explicit Exact(const Bytes& b) : p(new uint8_t[b.size() ? b.size() : 1]), n(b.size()) {
    if (n) std::memcpy(p.get(), b.data(), n);
  }
};

RdIndex walk(const Bytes& b, int ncols) {
  Exact e(b);
  return rd_walk(e.p.get(), e.n, ncols);
}

// Decodes row `r` of the walked set as the kernel does: prefix, header, the cells by type.
// Returns the column that failed (-1: none; -2: the row itself), the values in *out.
struct Val {
  uint64_t bits;
  std::string str;
};
int decode_row(const uint8_t* data, uint64_t len, const RdIndex& ix, uint64_t r, const std::vector<uint32_t>& types,
               std::vector<Val>* out) {
  uint64_t pos = ix.chunk_start[r / RD_CHUNK] + ix.row_off[r], n = 0;
  if (!rd_varint(data, len, &pos, &n) || n > len - pos) return -2;
  const uint64_t end = pos + n;
  if (!rd_header(data, end, (int)types.size(), &pos)) return -2;
  for (size_t c = 0; c < types.size(); ++c) {
    RdCell cell;
    const uint64_t before = pos;
    if (!rd_cell(data, end, types[c], &pos, &cell)) {
      if (pos != before) return -3;   // (a failed read leaves *pos alone)
      return (int)c;
    }
    if (pos > end) return -3;
    Val v{cell.bits, std::string()};
    if (types[c] == RD_T_STRING) {
      if (cell.str_at + cell.str_len > end) return -3;
      v.str.assign(reinterpret_cast<const char*>(data) + cell.str_at, cell.str_len);
    }
    out->push_back(v);
  }
  return -1;
}

}  // namespace

int main() {
  // ---- varints of every length, and the bounds of rd_varint itself
  {
    const uint64_t vals[] = {0, 127, 128, (1ull << 14) - 1, 1ull << 14, (1ull << 21) - 1, 1ull << 21, (1ull << 28) - 1,
                             1ull << 28, (1ull << 35) - 1, 1ull << 35, (1ull << 42) - 1, 1ull << 42, (1ull << 49) - 1,
                             1ull << 49, (1ull << 56) - 1, 1ull << 56, (1ull << 63) - 1, 1ull << 63, ~0ull};
    for (uint64_t v : vals) {
      Bytes b;
      put_varint(b, v);
      Exact e(b);
      uint64_t pos = 0, got = 1;
      CHECK(rd_varint(e.p.get(), e.n, &pos, &got) && got == v && pos == e.n);
      for (uint64_t cut = 0; cut < e.n; ++cut) {   // every truncation fails and moves nothing
        pos = 0;
        CHECK(!rd_varint(e.p.get(), cut, &pos, &got) && pos == 0);
      }
    }
    Bytes eleven(10, 0x80);   // ten continuation bytes: an 11th would follow
    eleven.push_back(0x01);
    Exact e(eleven);
    uint64_t pos = 0, got = 0;
    CHECK(!rd_varint(e.p.get(), e.n, &pos, &got) && pos == 0);
  }

  // ---- a well-formed set: (VID, INT, DOUBLE, BOOL, STRING, TIMESTAMP), three header forms
  {
    const std::vector<uint32_t> types = {RD_T_VID, RD_T_INT, RD_T_DOUBLE, RD_T_BOOL, RD_T_STRING, RD_T_TIMESTAMP};
    struct Row {
      int64_t vid, i;
      uint64_t dbits;
      bool b;
      std::string s;
      int64_t ts;
    };
    const std::vector<Row> rows = {
        {-5, 0, 0x8000000000000000ull, false, "", 1},
        {INT64_MIN, -1, 0x7FF8000000000123ull, true, "a", INT64_MAX},
        {INT64_MAX, INT64_MIN, 0x7FF0000000000000ull, true, std::string(300, 'x'), 128},
        {7, 16383, 0xFFF0000000000000ull, false, std::string("a\0b", 3), 0},
    };
    Bytes set;
    for (size_t r = 0; r < rows.size(); ++r) {
      Bytes cord;
      put_le(cord, (uint64_t)rows[r].vid, 8);
      put_varint(cord, (uint64_t)rows[r].i);
      put_le(cord, rows[r].dbits, 8);
      cord.push_back(rows[r].b ? 1 : 0);
      put_str(cord, rows[r].s);
      put_varint(cord, (uint64_t)rows[r].ts);
      if (r == 3) cord.insert(cord.end(), {9, 9, 9});   // left-over cord bytes are ignored
      add_row(set, row_of(cord, 1 + (int)(r % 3), (int)(r % 3) * 2, 0));   // (no offsets: 6 columns)
    }
    Exact e(set);
    const RdIndex ix = rd_walk(e.p.get(), e.n, (int)types.size());
    CHECK(ix.status == RD_WALK_OK && ix.rows == rows.size());
    CHECK(ix.chunk_start.size() == 1 && ix.chunk_start[0] == 0 && ix.row_off.size() == rows.size() && ix.row_off[0] == 0);
    for (size_t r = 0; r < rows.size(); ++r) {
      std::vector<Val> got;
      CHECK(decode_row(e.p.get(), e.n, ix, r, types, &got) == -1);
      CHECK(got.size() == 6);
      CHECK((int64_t)got[0].bits == rows[r].vid && (int64_t)got[1].bits == rows[r].i && got[2].bits == rows[r].dbits);
      CHECK(got[3].bits == (rows[r].b ? 1u : 0u) && got[4].str == rows[r].s && (int64_t)got[5].bits == rows[r].ts);
    }
  }

  // ---- block offsets: 16, 17, 32 columns skip 1, 1, 2 offsets of the header's width
  for (int nc : {1, 15, 16, 17, 31, 32})
    for (int ob : {1, 2, 3}) {
      Bytes cord;
      for (int c = 0; c < nc; ++c) put_varint(cord, 1000u + (unsigned)c);
      Bytes set;
      add_row(set, row_of(cord, ob, 0, nc >> 4));
      add_row(set, row_of(cord, ob, 1, nc >> 4));
      Exact e(set);
      const RdIndex ix = rd_walk(e.p.get(), e.n, nc);
      CHECK(ix.status == RD_WALK_OK && ix.rows == 2);
      const std::vector<uint32_t> types((size_t)nc, RD_T_INT);
      for (uint64_t r = 0; r < 2; ++r) {
        std::vector<Val> got;
        CHECK(decode_row(e.p.get(), e.n, ix, r, types, &got) == -1);
        for (int c = 0; c < nc; ++c) CHECK(got[c].bits == 1000u + (unsigned)c);
      }
    }

  // ---- chunks: a start every RD_CHUNK rows, offsets from it
  {
    Bytes set;
    const uint64_t n = 2 * RD_CHUNK + 1;
    for (uint64_t r = 0; r < n; ++r) {
      Bytes cord;
      put_varint(cord, r);
      add_row(set, row_of(cord, 1, 0, 0));
    }
    Exact e(set);
    const RdIndex ix = rd_walk(e.p.get(), e.n, 1);
    CHECK(ix.status == RD_WALK_OK && ix.rows == n && ix.chunk_start.size() == 3 && ix.row_off.size() == n);
    CHECK(ix.row_off[RD_CHUNK] == 0 && ix.row_off[2 * RD_CHUNK] == 0 && ix.row_off[1] == 3);
    for (uint64_t r : {(uint64_t)0, RD_CHUNK - 1, RD_CHUNK, 2 * RD_CHUNK}) {
      std::vector<Val> got;
      CHECK(decode_row(e.p.get(), e.n, ix, r, {RD_T_INT}, &got) == -1 && got[0].bits == r);
    }
    CHECK(walk({}, 1).rows == 0 && walk({}, 1).status == RD_WALK_OK);
  }

  // ---- status 5: what the walk refuses.  A good row stands in front, so the bad one is row 1.
  {
    Bytes good;
    Bytes cord;
    put_varint(cord, 5);
    add_row(good, row_of(cord, 1, 0, 0));
    auto with = [&](const Bytes& tail) {
      Bytes b = good;
      b.insert(b.end(), tail.begin(), tail.end());
      return b;
    };
    RdIndex ix = walk(with({0x80}), 1);   // a truncated prefix
    CHECK(ix.status == RD_WALK_PREFIX && ix.bad_row == 1 && ix.bad_at == good.size());
    ix = walk(with({0x80, 0x80, 0x80}), 1);
    CHECK(ix.status == RD_WALK_PREFIX);
    Bytes eleven(10, 0x80);   // an 11-byte prefix
    eleven.push_back(0x01);
    eleven.insert(eleven.end(), 64, 0);
    ix = walk(with(eleven), 1);
    CHECK(ix.status == RD_WALK_PREFIX && ix.bad_row == 1);
    ix = walk(with({3, 0, 1}), 1);   // a row past len: 3 announced, 2 there
    CHECK(ix.status == RD_WALK_PAST_END && ix.bad_row == 1);
    Bytes huge;   // a length near 2^64: no wrap-around
    put_varint(huge, ~0ull - 2);
    huge.push_back(0);
    ix = walk(with(huge), 1);
    CHECK(ix.status == RD_WALK_PAST_END);
    ix = walk(with({0, 2, 0, 1}), 1);   // a zero-length row
    CHECK(ix.status == RD_WALK_EMPTY_ROW && ix.bad_row == 1);
    ix = walk(with({2, 0x40, 0xEE}), 1);   // a header longer than its row: two version bytes, one there
    CHECK(ix.status == RD_WALK_HEADER && ix.bad_row == 1);
    ix = walk(with({2, 0x01, 0x00}), 16);   // ... one block offset of 2 bytes, one byte there
    CHECK(ix.status == RD_WALK_HEADER);
    ix = walk(with({1, 0x00}), 1);   // (a header alone is a row: its cells are the device's to miss)
    CHECK(ix.status == RD_WALK_OK && ix.rows == 2);
    CHECK(!rd_walk_malformed(RD_WALK_OK) && !rd_walk_malformed(RD_WALK_ROWS) && !rd_walk_malformed(RD_WALK_CHUNK) &&
          rd_walk_malformed(RD_WALK_PREFIX) && rd_walk_malformed(RD_WALK_HEADER));
  }

  // ---- status 6: cells that would read past their row's end; another row follows, so the bytes
  // behind the row's end are there to be read by a reader that forgot the bound
  {
    auto first_bad = [&](const Bytes& cord, const std::vector<uint32_t>& types, int* col) {
      Bytes set, next;
      add_row(set, row_of(cord, 1, 0, 0));
      put_le(next, 0x1122334455667788ull, 8);
      put_le(next, 0x1122334455667788ull, 8);
      add_row(set, row_of(next, 1, 0, 0));
      Exact e(set);
      const RdIndex ix = rd_walk(e.p.get(), e.n, (int)types.size());
      if (ix.status != RD_WALK_OK || ix.rows != 2) return false;
      std::vector<Val> got;
      *col = decode_row(e.p.get(), e.n, ix, 0, types, &got);
      return true;
    };
    int col = -9;
    Bytes cord(10, 0x80);   // a varint cell of 11 bytes
    cord.push_back(0x01);
    CHECK(first_bad(cord, {RD_T_INT}, &col) && col == 0);
    CHECK(first_bad(cord, {RD_T_TIMESTAMP}, &col) && col == 0);
    cord.assign({0x05});   // a varint cell cut by the row's end
    cord.push_back(0x80);
    CHECK(first_bad(cord, {RD_T_INT, RD_T_INT}, &col) && col == 1);
    cord.assign(7, 0x11);   // a VID cell with 7 bytes left
    CHECK(first_bad(cord, {RD_T_VID}, &col) && col == 0);
    CHECK(first_bad(cord, {RD_T_DOUBLE}, &col) && col == 0);
    cord.assign(8, 0x11);   // ... the well-formed rowset under a schema with one VID column too many
    CHECK(first_bad(cord, {RD_T_VID, RD_T_VID}, &col) && col == 1);
    CHECK(first_bad(cord, {RD_T_VID}, &col) && col == -1);
    cord.assign({5, 'a', 'b'});   // a string length past the row's end
    CHECK(first_bad(cord, {RD_T_STRING}, &col) && col == 0);
    cord.clear();
    put_varint(cord, ~0ull);   // ... near 2^64: no wrap-around
    CHECK(first_bad(cord, {RD_T_STRING}, &col) && col == 0);
    cord.assign({0x01});   // a BOOL with nothing left
    CHECK(first_bad(cord, {RD_T_BOOL, RD_T_BOOL}, &col) && col == 1);
    cord.assign(8, 0);   // FLOAT has no reader
    CHECK(first_bad(cord, {RD_T_FLOAT}, &col) && col == 0);
  }
  std::puts("rowdec host walk and cells OK");
  return 0;
}
