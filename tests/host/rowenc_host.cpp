// Stand-alone check of nbg_rows_encode's host-side tables (nebula_amd/csrc/rowenc.h), built with
// -fsanitize=address,undefined by tests/test_rowenc_host.py: the per-chunk OVER positions and the
// table of string constants outside the dictionary.  No HIP, no GPU.
#include <cstdio>
#include <cstdlib>

#include "rowenc.h"

#define CHECK(x)                                                 \
  do {                                                           \
    if (!(x)) {                                                  \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      return 1;                                                  \
    }                                                            \
  } while (0)

int main() {
  using namespace nbg;
  const uint64_t CHUNK = 2048;
  {   // one chunk per started 2,048 rows of a segment, in segment order; an empty segment has none
    const std::vector<std::pair<uint64_t, uint64_t>> segs = {{0, 1}, {100, 2048}, {9000, 2049}, {20000, 0}, {30000, 5000}};
    const std::vector<int> types = {0, 1, 2, 3, 31};
    const std::vector<uint8_t> got = re_chunk_types(segs, types, CHUNK);
    const std::vector<uint8_t> want = {0, 1, 2, 2, 31, 31, 31};
    CHECK(got == want);
    CHECK(re_chunk_types({}, {}, CHUNK).empty());
    CHECK(re_chunk_types({{5, 7}}, {}, CHUNK) == std::vector<uint8_t>{0});   // (a missing type reads as position 0)
  }
  {   // a big segment: as many entries as chunks
    const std::vector<uint8_t> got = re_chunk_types({{0, (1ull << 22) + 1}}, {7}, CHUNK);
    CHECK(got.size() == 2049 && got.front() == 7 && got.back() == 7);
  }
  {   // the constants: entry t * ncols + c; only string columns; a short row has empty entries
    const std::vector<std::vector<std::string>> cs = {{"", "one", "skipped"}, {"x", "zwei"}, {}};
    const std::vector<uint8_t> is_string = {1, 1, 0};
    const ReConsts k = re_const_table(cs, is_string, 3);
    CHECK(k.fits);
    CHECK(k.off.size() == 3 * 3 + 1);
    const std::vector<uint32_t> want = {0, 0, 3, 3, 4, 8, 8, 8, 8, 8};
    CHECK(k.off == want);
    CHECK(std::string(k.bytes.begin(), k.bytes.end()) == "onexzwei");
    for (size_t e = 0; e + 1 < k.off.size(); ++e) CHECK(k.off[e] <= k.off[e + 1] && k.off[e + 1] <= k.bytes.size());
  }
  {   // no types at all, no columns: one offset, no bytes
    const ReConsts k = re_const_table({}, {}, 0);
    CHECK(k.off.size() == 1 && k.off[0] == 0 && k.bytes.empty());
    const ReConsts k2 = re_const_table({{"a"}}, {}, 1);   // (no column marked: nothing copied)
    CHECK(k2.off.size() == 2 && k2.bytes.empty());
  }
  std::puts("rowenc host tables OK");
  return 0;
}
