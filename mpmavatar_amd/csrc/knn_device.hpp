// knn_device.hpp -- the exact k nearest targets of every query, brute force, for K <= 16 and points of 3 or 6 floats: the search
// behind find_k_closest_verts (utils/smplx_deformer.py:164-185, pytorch3d's knn_points), o3d_knn (preprocess/helpers.py:84-94) and
// the K = 1 search of lbs_weights_inpainting_*.py.  Next to k_nn_d2 (nn_device.hpp), which keeps the minimum only.
//   k_knn_slices  grid x = query tile (one query per lane, in registers), y = target slice.  The workgroup walks its slice in LDS
//                 tiles of KNN_TILE targets, one plane per coordinate (6 x 1024 floats = 24 KB); target coordinates are wave-uniform,
//                 so four targets' worth of one coordinate is one broadcast 16-byte read.  Each lane keeps knn::Nearest<KP> -- KP = K
//                 rounded up to 4, 8 or 16, a template argument, so the list lives in registers (0 bytes of scratch) -- and a float
//                 compare against its current KP-th distance guards the unrolled insertion.  A tile's tail is padded with +inf,
//                 which no compare lets in.  Each (slice, query) then writes its K keys (d2 bits << 32 | index) to `keys`.
//   k_knn_merge   one lane per query folds slices x K keys into the final K by the same insertion on the 64-bit keys.
// The key order is total, so the result does not depend on how the targets were sliced; no atomics.  An unfilled list entry is
// (+inf, first index of the slice): it loses to every finite distance and keeps indices in range whatever the input holds.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "entry.hpp"
#include "repose_math.hpp"

namespace knn {

constexpr int TPB = QUERY_TILE;
constexpr int KNN_TILE = 1024;  // targets staged in LDS at a time
static_assert(KNN_TILE % 4 == 0, "targets are read four at a time");

typedef float f4 __attribute__((ext_vector_type(4)));

template <int D, int KP>
static __global__ __launch_bounds__(TPB) void k_knn_slices(const float *__restrict__ src, int n_src, const float *__restrict__ dst, int n_dst,
                                                           int slice_len, int k_out, unsigned long long *__restrict__ keys) {
  __shared__ __attribute__((aligned(16))) float ts[D][KNN_TILE];
  const int tid = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * TPB + tid;
  const int j0 = (int)min((int64_t)blockIdx.y * slice_len, (int64_t)n_dst);
  const int j1 = (int)min((int64_t)j0 + slice_len, (int64_t)n_dst);

  float q[D];
  {
    const int64_t ic = i < n_src ? i : n_src - 1;  // lanes past the end repeat the last query and write nothing
#pragma unroll
    for (int d = 0; d < D; ++d) q[d] = src[(size_t)ic * D + d];
  }
  Nearest<KP> best;
  best.fill(__builtin_inff(), j0 < n_dst ? j0 : 0);

  for (int base = j0; base < j1; base += KNN_TILE) {
    const int nt = min(KNN_TILE, j1 - base), nt4 = (nt + 3) & ~3;
    __syncthreads();
    for (int t = tid; t < nt4; t += TPB) {
#pragma unroll
      for (int d = 0; d < D; ++d) ts[d][t] = t < nt ? dst[(size_t)(base + t) * D + d] : __builtin_inff();
    }
    __syncthreads();
    for (int c = 0; c < nt4; c += 4) {
      f4 t4[D];
#pragma unroll
      for (int d = 0; d < D; ++d) t4[d] = *(const f4 *)&ts[d][c];
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        float t[D];
#pragma unroll
        for (int d = 0; d < D; ++d) t[d] = t4[d][p];
        const float d2 = dist2<D>(q, t);
        if (d2 < best.worst()) best.insert(d2, base + c + p);
      }
    }
  }

  if (i < n_src) {
    unsigned long long *o = keys + ((size_t)blockIdx.y * n_src + (size_t)i) * k_out;
#pragma unroll
    for (int k = 0; k < KP; ++k)
      if (k < k_out) o[k] = key(best.d[k], best.j[k]);
  }
}

template <int KP>
static __global__ __launch_bounds__(TPB) void k_knn_merge(int n_src, int n_dst, int slices, int k_out, const unsigned long long *__restrict__ keys,
                                                          float *__restrict__ dists, int32_t *__restrict__ idx) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n_src) return;
  List<unsigned long long, KP> best;
  best.fill(~0ull);
  for (int s = 0; s < slices; ++s) {
    const unsigned long long *in = keys + ((size_t)s * n_src + (size_t)i) * k_out;
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      if (k < k_out) {
        const unsigned long long x = in[k];
        if (x < best.worst()) best.insert(x);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < KP; ++k) {
    if (k < k_out) {
      int32_t j = key_index(best.v[k]);
      if (j < 0 || j >= n_dst) j = 0;  // cannot happen for k_out <= n_dst; keeps the promise of in-range indices regardless
      dists[(size_t)i * k_out + k] = key_dist(best.v[k]);
      idx[(size_t)i * k_out + k] = j;
    }
  }
}

template <int D, int KP>
static inline int launch_knn_dk(hipStream_t s, const float *src, int32_t n, const float *dst, int32_t m, int32_t k, const Plan &p, uint64_t *keys,
                                float *dists, int32_t *idx) {
  hipLaunchKernelGGL((k_knn_slices<D, KP>), dim3((unsigned)p.tiles, (unsigned)p.slices), TPB, 0, s, src, n, dst, m, p.slice_len,
                     k, (unsigned long long *)keys);
  ENTRY_CHECK(hipGetLastError());
  hipLaunchKernelGGL((k_knn_merge<KP>), dim3((unsigned)p.tiles), TPB, 0, s, n, m, p.slices, k, (const unsigned long long *)keys, dists, idx);
  return entry::check(hipGetLastError());
}

// keys: p.slices * n * k values.  n, m > 0, 1 <= k <= min(m, 16), dim 3 or 6.
static inline int launch_knn(hipStream_t s, const float *src, int32_t n, const float *dst, int32_t m, int32_t dim, int32_t k, const Plan &p,
                             uint64_t *keys, float *dists, int32_t *idx) {
  const int kp = padded_k(k);
  if (dim == 3) {
    if (kp == 4) return launch_knn_dk<3, 4>(s, src, n, dst, m, k, p, keys, dists, idx);
    if (kp == 8) return launch_knn_dk<3, 8>(s, src, n, dst, m, k, p, keys, dists, idx);
    return launch_knn_dk<3, 16>(s, src, n, dst, m, k, p, keys, dists, idx);
  }
  if (kp == 4) return launch_knn_dk<6, 4>(s, src, n, dst, m, k, p, keys, dists, idx);
  if (kp == 8) return launch_knn_dk<6, 8>(s, src, n, dst, m, k, p, keys, dists, idx);
  return launch_knn_dk<6, 16>(s, src, n, dst, m, k, p, keys, dists, idx);
}

}  // namespace knn
