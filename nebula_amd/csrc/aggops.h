// The fold of the aggregate YIELD's accumulators (YaOp, nbg_internal.h), shared by k_ya_reduce
// (kernels.hip) and k_ya_finish (yieldagg.hip): every accumulator is 8 bytes, MAX / MIN hold
// ordimg.h's order-preserving image.
#pragma once
#include <hip/hip_runtime.h>

#include "ordimg.h"
#include "ws.h"

namespace nbg {

__device__ __forceinline__ uint64_t ya_identity(uint8_t op) {
  switch (op) {
    case YA_MIN: case YA_AND: return ~0ull;
    case YA_SUM_D: case YA_SQ: return SIGN64;   // -0.0: x + -0.0 == x for every x
    default: return 0ull;
  }
}

__device__ __forceinline__ uint64_t ya_combine(uint8_t op, uint64_t a, uint64_t b) {
  switch (op) {
    case YA_SUM_D: case YA_SQ: return (uint64_t)__double_as_longlong(__dadd_rn(__longlong_as_double((long long)a),
                                                                             __longlong_as_double((long long)b)));
    case YA_MAX: return a > b ? a : b;
    case YA_MIN: return a < b ? a : b;
    case YA_AND: return a & b;
    case YA_OR: return a | b;
    case YA_XOR: return a ^ b;
    default: return a + b;
  }
}

// every lane gets the fold of the wave's 64 values (a butterfly: the same pairing on every run)
__device__ __forceinline__ uint64_t ya_wave_reduce(uint8_t op, uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = ya_combine(op, v, (uint64_t)__shfl_xor((unsigned long long)v, o));
  return v;
}

// the fold of a workgroup's values in thread 0: the waves' folds combined in wave order.  `wp`
// holds WAVES cells; two barriers, so the cells are free again on return.
__device__ __forceinline__ uint64_t ya_block_reduce(uint8_t op, uint64_t v, uint64_t* wp) {
  v = ya_wave_reduce(op, v);
  if ((threadIdx.x & 63) == 0) wp[threadIdx.x >> 6] = v;
  __syncthreads();
  uint64_t t = wp[0];
  for (int w = 1; w < WAVES; ++w) t = ya_combine(op, t, wp[w]);
  __syncthreads();
  return t;
}

__device__ __forceinline__ bool ya_in_pass(uint8_t op, int pass) { return (op == YA_SQ) == (pass == 1); }

// the mean a STD measures from: the AVG of the same argument
__device__ __forceinline__ double ya_avg(uint64_t sum, bool dbl, uint64_t n) {
  const double s = dbl ? __longlong_as_double((long long)sum) : (double)(int64_t)sum;
  return __ddiv_rn(s, (double)n);
}

}  // namespace nbg
