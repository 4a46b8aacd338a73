// Order-preserving 64-bit images of column payloads, shared by GROUP BY's MAX / MIN (groupby.hip)
// and ORDER BY's sort keys (orderby.hip): signed int64 and IEEE doubles onto unsigned order.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace nbg {

constexpr uint64_t SIGN64 = 1ull << 63;

// ints: flip the sign bit.  doubles: negatives complemented (so larger magnitude sorts lower),
// non-negatives above them; NaNs land at the ends by their bits (IEEE total order).
__host__ __device__ __forceinline__ uint64_t ord_image(uint64_t v, uint8_t dbl) {
  if (!dbl) return v ^ SIGN64;
  return (v & SIGN64) ? ~v : (v | SIGN64);
}
__host__ __device__ __forceinline__ uint64_t ord_unimage(uint64_t v, uint8_t dbl) {
  if (!dbl) return v ^ SIGN64;
  return (v & SIGN64) ? (v & ~SIGN64) : ~v;
}

}  // namespace nbg
