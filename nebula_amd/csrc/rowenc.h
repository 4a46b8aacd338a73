// nebula_amd — the host-side tables of nbg_rows_encode (rowenc.hip, stages.cpp).  Nothing here
// calls HIP, so a stand-alone program can run these under a host sanitizer
// (tests/host/rowenc_host.cpp).
#pragma once
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

namespace nbg {

// The OVER position of every chunk that stage_chunks (stage.h) cuts `segs` = (first row, rows)
// into over all rows: a segment of n rows is ceil(n / chunk) chunks, an empty one none.  types[i]
// is segment i's OVER position (< 256: NBG_MAX_OVER is 32).
inline std::vector<uint8_t> re_chunk_types(const std::vector<std::pair<uint64_t, uint64_t>>& segs,
                                           const std::vector<int>& types, uint64_t chunk) {
  std::vector<uint8_t> out;
  for (size_t i = 0; i < segs.size(); ++i) {
    const uint64_t n = (segs[i].second + chunk - 1) / chunk;
    out.insert(out.end(), (size_t)n, (uint8_t)(i < types.size() ? types[i] : 0));
  }
  return out;
}

// The string constants outside the dictionary, as the kernels read them: entry t * ncols + c is
// what OVER position t spells in column c, bytes[off[e], off[e + 1]).  A column that is no
// string column, or a position that names fewer columns, has an empty entry.
struct ReConsts {
  std::vector<uint32_t> off;   // [types * ncols + 1]
  std::vector<char> bytes;
  bool fits = true;            // the bytes fit 32-bit offsets
};
inline ReConsts re_const_table(const std::vector<std::vector<std::string>>& const_str, const std::vector<uint8_t>& is_string,
                               int ncols) {
  ReConsts k;
  k.off.reserve(const_str.size() * (size_t)ncols + 1);
  k.off.push_back(0);
  for (const std::vector<std::string>& per_type : const_str)
    for (int c = 0; c < ncols; ++c) {
      if (c < (int)per_type.size() && c < (int)is_string.size() && is_string[c])
        k.bytes.insert(k.bytes.end(), per_type[c].begin(), per_type[c].end());
      if (k.bytes.size() > 0xFFFFFFFFull) k.fits = false;
      k.off.push_back((uint32_t)k.bytes.size());
    }
  return k;
}

}  // namespace nbg
