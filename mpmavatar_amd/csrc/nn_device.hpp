// nn_device.hpp -- the brute-force nearest-target search of the geometry metrics (geo.hip, mpmhip_nn_dist2) as device code and its
// launch, for the two translation units that run it: geo.hip (Chamfer, F-score) and track.hip (collision_penalty's nearest body
// vertex).  The kernel and the slicing rule are geo.hip's, moved here unchanged; each translation unit gets its own copy (static).
// Measured numbers: DESIGN.md section 8, profiles/geo_metrics_bench.*.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "entry.hpp"
#include "geo_math.hpp"

namespace nn {

using geo::P3;

constexpr int TPB = 256;
#ifndef GEO_NN_Q
#define GEO_NN_Q 4  // queries per lane (chosen by measurement)
#endif
constexpr int NN_Q = GEO_NN_Q;
constexpr int NN_TILE = 1024;  // targets staged in LDS at a time (12 KB)
constexpr int NN_CHUNK = 32;   // targets between two looks at "did this lane's minimum move"
static_assert(NN_TILE % NN_CHUNK == 0 && NN_CHUNK % 2 == 0, "tiles are whole chunks, chunks whole pairs");

typedef float f2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ P3 ld3(const float *p, size_t i) { return P3{p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }

// geo::pair_d2 for two targets at once, operation for operation (so that the index search below finds the very bits
// the minimum was taken over): v_pk_add_f32 x3, v_pk_mul_f32, v_pk_fma_f32 x2.
__device__ __forceinline__ f2 pair_d2x2(P3 q, f2 tx, f2 ty, f2 tz) {
  f2 dx = q.x - tx, dy = q.y - ty, dz = q.z - tz;
  return __builtin_elementwise_fma(dz, dz, __builtin_elementwise_fma(dy, dy, dx * dx));
}

// Nearest target of every query, brute force.  Grid: x = query tile (TPB * NN_Q queries, NN_Q per lane in registers),
// y = target slice [y * slice_len, min(n_dst, (y + 1) * slice_len)).  The workgroup walks its slice in LDS tiles; target
// coordinates are wave-uniform, so the reads are broadcast reads of one address.  The inner loop keeps the running
// minimum only (three-way min over two targets and the best so far); WHICH target it was is settled per chunk of
// NN_CHUNK targets -- "the minimum moved in this chunk" costs a compare per chunk instead of a compare and a select per
// target -- and the first index of the last chunk that moved it is found afterwards by recomputing that one chunk.
// Targets past the last whole chunk of the slice (fewer than NN_CHUNK) take a plain loop bounded by the slice's end:
// nothing outside [0, n_dst) is ever read or can win.  Each lane then folds (d2 bits << 32 | index) into best[q] with one
// 64-bit atomicMin: non-negative floats order like their bit patterns, so the fold does not depend on the order of the
// slices (bitwise reproducible) and ties go to the lowest index.
static __global__ __launch_bounds__(TPB) void k_nn_d2(const float *__restrict__ src, int n_src, const float *__restrict__ dst,
                                                      int n_dst, int slice_len, unsigned long long *best) {
  __shared__ __attribute__((aligned(16))) float xs[NN_TILE], ys[NN_TILE], zs[NN_TILE];  // read as pairs
  const int tid = threadIdx.x;
  const int64_t q0 = (int64_t)blockIdx.x * (TPB * NN_Q) + tid;
  const int j0 = (int)min((int64_t)blockIdx.y * slice_len, (int64_t)n_dst);
  const int j1 = (int)min((int64_t)j0 + slice_len, (int64_t)n_dst);
  const int jm = j0 + (j1 - j0) / NN_CHUNK * NN_CHUNK;  // end of the whole chunks

  P3 q[NN_Q];
  float bst[NN_Q], seen[NN_Q];
  int chunk[NN_Q];
#pragma unroll
  for (int k = 0; k < NN_Q; ++k) {
    int64_t i = q0 + (int64_t)k * TPB;
    q[k] = ld3(src, (size_t)(i < n_src ? i : n_src - 1));  // lanes past the end repeat the last query and skip the fold
    bst[k] = seen[k] = __builtin_inff();
    chunk[k] = -1;
  }

  for (int base = j0; base < jm; base += NN_TILE) {
    const int nt = min(NN_TILE, jm - base);
    __syncthreads();
    for (int i = tid; i < nt; i += TPB) {
      P3 t = ld3(dst, (size_t)(base + i));
      xs[i] = t.x; ys[i] = t.y; zs[i] = t.z;
    }
    __syncthreads();
    for (int c = 0; c < nt; c += NN_CHUNK) {
#pragma unroll
      for (int p = 0; p < NN_CHUNK; p += 2) {
        f2 tx = *(const f2 *)&xs[c + p], ty = *(const f2 *)&ys[c + p], tz = *(const f2 *)&zs[c + p];
#pragma unroll
        for (int k = 0; k < NN_Q; ++k) {
          f2 d = pair_d2x2(q[k], tx, ty, tz);
          bst[k] = __builtin_fminf(__builtin_fminf(bst[k], d.x), d.y);
        }
      }
#pragma unroll
      for (int k = 0; k < NN_Q; ++k)
        if (bst[k] < seen[k]) { seen[k] = bst[k]; chunk[k] = base + c; }
    }
  }

#pragma unroll
  for (int k = 0; k < NN_Q; ++k) {
    int idx = j0;  // stays in range whatever the coordinates hold (non-finite input: unspecified values, valid index)
    if (chunk[k] >= 0)
      for (int j = chunk[k] + NN_CHUNK - 1; j >= chunk[k]; --j)  // descending: the lowest matching index is kept
        if (geo::pair_d2(q[k], ld3(dst, (size_t)j)) == bst[k]) idx = j;
    for (int j = jm; j < j1; ++j) {
      float d = geo::pair_d2(q[k], ld3(dst, (size_t)j));
      if (d < bst[k]) { bst[k] = d; idx = j; }
    }
    int64_t i = q0 + (int64_t)k * TPB;
    if (i < n_src && j1 > j0)
      atomicMin(&best[i], ((unsigned long long)__float_as_uint(bst[k]) << 32) | (unsigned)idx);
  }
}

// best [n_src] = (d2 bits << 32 | lowest index of the exact minimum), on stream s.  n_src, n_dst > 0; slices = 0: chosen here.
static inline int launch_nearest(hipStream_t s, const float *src, int32_t n_src, const float *dst, int32_t n_dst, int32_t slices,
                                 uint64_t *best) {
  const int64_t tiles = ((int64_t)n_src + TPB * NN_Q - 1) / (TPB * NN_Q);
  if (slices == 0) {
    // auto: 100,000 queries are ~100 query tiles, far fewer than the 256 CUs x 8 workgroups that fill an MI355X with two
    // waves per SIMD, so the targets are cut until tiles x slices gets there -- but not below 8 chunks a slice, where the
    // per-slice tail and the atomic fold would start to show
    const int64_t want = (256 * 8 + tiles - 1) / tiles, most = (n_dst + 8 * NN_CHUNK - 1) / (8 * NN_CHUNK);
    slices = (int32_t)(want < most ? want : most);
  }
  if (slices > n_dst) slices = n_dst;
  if (slices > 65535) slices = 65535;  // grid y limit
  const int slice_len = (int)(((int64_t)n_dst + slices - 1) / slices);
  slices = (n_dst + slice_len - 1) / slice_len;  // no empty slice at the end
  ENTRY_CHECK(hipMemsetAsync(best, 0xff, (size_t)n_src * sizeof(uint64_t), s));
  hipLaunchKernelGGL(k_nn_d2, dim3((unsigned)tiles, (unsigned)slices), TPB, 0, s, src, n_src, dst, n_dst, slice_len,
                     (unsigned long long *)best);
  return entry::check(hipGetLastError());
}

}  // namespace nn
