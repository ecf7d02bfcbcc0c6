// block_sum.hpp -- the fixed-order workgroup sum of the fp64 reductions (reg.hip, track.hip): no floating-point atomics, the same
// input gives the same bits.
#pragma once
#include <hip/hip_runtime.h>

// Sum of N doubles per lane over the workgroup in a fixed order: shuffles within each wave (lane l += lane l + off, off = 32 .. 1),
// then thread 0 adds the wave sums in wave order.  Valid in thread 0 only.  Every thread of the workgroup must call it.
template <int N, int WAVES>
__device__ __forceinline__ void block_sum(double (&v)[N], double (*red)[WAVES]) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += __shfl_down(v[i], off);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int i = 0; i < N; ++i) red[i][wave] = v[i];
  __syncthreads();
  if (threadIdx.x == 0)
#pragma unroll
    for (int i = 0; i < N; ++i) {
      v[i] = red[i][0];
#pragma unroll
      for (int w = 1; w < WAVES; ++w) v[i] += red[i][w];
    }
}
