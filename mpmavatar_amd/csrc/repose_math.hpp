// repose_math.hpp -- re-posing through the body's skinning transforms (utils/smplx_deformer.py:164-337) and the k-nearest search
// under it, as per-item functions that compile for the device (repose.hip, knn_device.hpp) and for the host
// (tests/hostrepose/hostrepose.cpp):
//   knn::dist2<D>      the direct-form squared distance sum_d (q_d - t_d)^2, accumulated in ascending d with explicit fma
//   knn::key / List<K> the ordering key (bits of d2) << 32 | index as one unsigned 64-bit value, and a K-long ascending list held in
//                      registers: every loop over it has a compile-time trip count, so no element is indexed dynamically
//   rp::blend          T = sum_j w_j A_j, all 16 entries, ascending j, explicit fma
//   rp::inverse4       the general 4 x 4 inverse by cofactors (the last row of T is (0, 0, 0, sum w), and sum w != 1 in general)
//   knn::plan          how the targets are cut into slices (host code, shared with the host restatement)
//   rp::to_pose / to_tpose, rp::shepard_weights / shepard_entry
// fp32 throughout; no sums whose order depends on a launch.  A singular T gives non-finite output.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

namespace knn {

constexpr int MAX_K = 16;

template <int D>
__host__ __device__ __forceinline__ float dist2(const float *q, const float *t) {
  float d0 = q[0] - t[0];
  float s = d0 * d0;
#pragma unroll
  for (int d = 1; d < D; ++d) {
    const float e = q[d] - t[d];
    s = fmaf(e, e, s);
  }
  return s;
}

__host__ __device__ __forceinline__ uint32_t float_bits(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  return u;
}
__host__ __device__ __forceinline__ float bits_float(uint32_t u) {
  float x;
  memcpy(&x, &u, 4);
  return x;
}

constexpr int QUERY_TILE = 256;  // queries per workgroup of the search, one per lane

// the list length a K is searched with: K rounded up to 4, 8 or 16
constexpr int padded_k(int k) { return k <= 4 ? 4 : k <= 8 ? 8 : 16; }

struct Plan {
  int32_t slices, slice_len;
  int64_t tiles;
};

// slices = 0: cut the targets until tiles x slices fills the device (256 CUs x 8 workgroups), but not below 256 targets a slice
inline Plan plan(int32_t n, int32_t m, int32_t slices) {
  Plan p;
  p.tiles = ((int64_t)n + QUERY_TILE - 1) / QUERY_TILE;
  if (p.tiles < 1) p.tiles = 1;
  if (slices <= 0) {
    const int64_t want = (256 * 8 + p.tiles - 1) / p.tiles, most = ((int64_t)m + 255) / 256;
    slices = (int32_t)(want < most ? want : most);
  }
  if (slices > m) slices = m;
  if (slices > 65535) slices = 65535;  // grid y limit
  if (slices < 1) slices = 1;
  p.slice_len = (int32_t)(((int64_t)m + slices - 1) / slices);
  if (p.slice_len < 1) p.slice_len = 1;
  p.slices = (int32_t)(((int64_t)m + p.slice_len - 1) / p.slice_len);  // no empty slice at the end
  if (p.slices < 1) p.slices = 1;
  return p;
}

// non-negative floats order like their bit patterns, so the keys order by (d2, index)
__host__ __device__ __forceinline__ uint64_t key(float d2, int32_t index) { return ((uint64_t)float_bits(d2) << 32) | (uint32_t)index; }
__host__ __device__ __forceinline__ float key_dist(uint64_t k) { return bits_float((uint32_t)(k >> 32)); }
__host__ __device__ __forceinline__ int32_t key_index(uint64_t k) { return (int32_t)(uint32_t)(k & 0xffffffffull); }

// K values in ascending order.  insert(v) assumes v < worst(): the caller's guard; an equal value goes behind its equals.
template <typename T, int K>
struct List {
  T v[K];
  __host__ __device__ __forceinline__ void fill(T x) {
#pragma unroll
    for (int i = 0; i < K; ++i) v[i] = x;
  }
  __host__ __device__ __forceinline__ T worst() const { return v[K - 1]; }
  __host__ __device__ __forceinline__ void insert(T x) {
#pragma unroll
    for (int i = K - 1; i >= 0; --i) {
      const bool below = i > 0 && x < v[i > 0 ? i - 1 : 0];
      if (below) v[i] = v[i > 0 ? i - 1 : 0];
      else if (x < v[i]) v[i] = x;
    }
  }
};

// the same list as two arrays, for the search's inner loop: distances decide, the index rides along (targets arrive in ascending
// index order, so "behind its equals" is "the lower index first")
template <int K>
struct Nearest {
  float d[K];
  int32_t j[K];
  __host__ __device__ __forceinline__ void fill(float dist, int32_t index) {
#pragma unroll
    for (int i = 0; i < K; ++i) { d[i] = dist; j[i] = index; }
  }
  __host__ __device__ __forceinline__ float worst() const { return d[K - 1]; }
  __host__ __device__ __forceinline__ void insert(float dist, int32_t index) {
#pragma unroll
    for (int i = K - 1; i >= 0; --i) {
      const int p = i > 0 ? i - 1 : 0;
      const bool below = i > 0 && dist < d[p];
      if (below) { d[i] = d[p]; j[i] = j[p]; }
      else if (dist < d[i]) { d[i] = dist; j[i] = index; }
    }
  }
};

}  // namespace knn

namespace rp {

// T [16] row-major = sum_j w[j] A[16 j ..], ascending j
__host__ __device__ __forceinline__ void blend(const float *w, int n_joints, const float *A, float *T) {
#pragma unroll
  for (int e = 0; e < 16; ++e) T[e] = 0.f;
  for (int j = 0; j < n_joints; ++j) {
    const float wj = w[j];
    const float *a = A + 16 * (size_t)j;
#pragma unroll
    for (int e = 0; e < 16; ++e) T[e] = fmaf(wj, a[e], T[e]);
  }
}

// rows 0..2 of M (v, 1), summed in ascending column order as a matrix product does
__host__ __device__ __forceinline__ void apply3(const float *M, const float *v, float *out) {
#pragma unroll
  for (int r = 0; r < 3; ++r) out[r] = fmaf(M[4 * r + 2], v[2], fmaf(M[4 * r + 1], v[1], M[4 * r] * v[0])) + M[4 * r + 3];
}

// the inverse of a general 4 x 4 matrix by cofactors (2 x 2 minors of the upper and lower row pairs).  det == 0: non-finite.
__host__ __device__ __forceinline__ void inverse4(const float *m, float *inv) {
  const float s0 = m[0] * m[5] - m[4] * m[1], s1 = m[0] * m[6] - m[4] * m[2], s2 = m[0] * m[7] - m[4] * m[3];
  const float s3 = m[1] * m[6] - m[5] * m[2], s4 = m[1] * m[7] - m[5] * m[3], s5 = m[2] * m[7] - m[6] * m[3];
  const float c5 = m[10] * m[15] - m[14] * m[11], c4 = m[9] * m[15] - m[13] * m[11], c3 = m[9] * m[14] - m[13] * m[10];
  const float c2 = m[8] * m[15] - m[12] * m[11], c1 = m[8] * m[14] - m[12] * m[10], c0 = m[8] * m[13] - m[12] * m[9];
  const float det = s0 * c5 - s1 * c4 + s2 * c3 + s3 * c2 - s4 * c1 + s5 * c0;
  const float r = 1.0f / det;
  inv[0] = (m[5] * c5 - m[6] * c4 + m[7] * c3) * r;
  inv[1] = (-m[1] * c5 + m[2] * c4 - m[3] * c3) * r;
  inv[2] = (m[13] * s5 - m[14] * s4 + m[15] * s3) * r;
  inv[3] = (-m[9] * s5 + m[10] * s4 - m[11] * s3) * r;
  inv[4] = (-m[4] * c5 + m[6] * c2 - m[7] * c1) * r;
  inv[5] = (m[0] * c5 - m[2] * c2 + m[3] * c1) * r;
  inv[6] = (-m[12] * s5 + m[14] * s2 - m[15] * s1) * r;
  inv[7] = (m[8] * s5 - m[10] * s2 + m[11] * s1) * r;
  inv[8] = (m[4] * c4 - m[5] * c2 + m[7] * c0) * r;
  inv[9] = (-m[0] * c4 + m[1] * c2 - m[3] * c0) * r;
  inv[10] = (m[12] * s4 - m[13] * s2 + m[15] * s0) * r;
  inv[11] = (-m[8] * s4 + m[9] * s2 - m[11] * s0) * r;
  inv[12] = (-m[4] * c3 + m[5] * c1 - m[6] * c0) * r;
  inv[13] = (m[0] * c3 - m[1] * c1 + m[2] * c0) * r;
  inv[14] = (-m[12] * s3 + m[13] * s1 - m[14] * s0) * r;
  inv[15] = (m[8] * s3 - m[9] * s1 + m[10] * s0) * r;
}

// transform_to_pose :310-337: (T (v, 1))[:3], then + transl, then * scale; transl [3] and scale [1] may be NULL
__host__ __device__ __forceinline__ void to_pose(const float *T, const float *v, const float *transl, const float *scale, float *out) {
  apply3(T, v, out);
  if (transl) { out[0] += transl[0]; out[1] += transl[1]; out[2] += transl[2]; }
  if (scale) { out[0] *= scale[0]; out[1] *= scale[0]; out[2] *= scale[0]; }
}

// transform_to_t_pose :262-286: v' = v / scale - transl, then (T^-1 (v', 1))[:3].  Tinv [16] is written (the T the reference returns).
__host__ __device__ __forceinline__ void to_tpose(const float *T, const float *v, const float *transl, const float *scale, float *Tinv,
                                                  float *out) {
  float u[3] = {v[0], v[1], v[2]};
  if (scale) { u[0] /= scale[0]; u[1] /= scale[0]; u[2] /= scale[0]; }
  if (transl) { u[0] -= transl[0]; u[1] -= transl[1]; u[2] -= transl[2]; }
  inverse4(T, Tinv);
  apply3(Tinv, u, out);
}

// weights_from_k_closest_verts :201-204 with an integer power: w_k = clamp(d2_k, 1e-8)^-power / sum, the sum in ascending k.
// K <= knn::MAX_K; w [MAX_K] is written up to k.
__host__ __device__ __forceinline__ void shepard_weights(const float *d2, int k, int power, float *w) {
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < knn::MAX_K; ++i) {
    if (i < k) {
      const float c = fmaxf(d2[i], 1e-8f);
      float pw = 1.f;
      for (int e = 0; e < power; ++e) pw *= c;
      w[i] = 1.0f / pw;
      sum += w[i];
    }
  }
#pragma unroll
  for (int i = 0; i < knn::MAX_K; ++i)
    if (i < k) w[i] = w[i] / sum;
}

// the gather of :235-241 for one (point, joint): sum_k w_k lbs[idx_k, joint], ascending k; an index outside [0, n_verts) is clamped
__host__ __device__ __forceinline__ float shepard_entry(const float *w, const int32_t *idx, int k, const float *lbs, int n_verts, int n_joints,
                                                        int joint) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < knn::MAX_K; ++i) {
    if (i < k) {
      int32_t v = idx[i];
      v = v < 0 ? 0 : v >= n_verts ? n_verts - 1 : v;
      s = fmaf(w[i], lbs[(size_t)v * n_joints + joint], s);
    }
  }
  return s;
}

}  // namespace rp
