// geo.hip -- the geometry evaluation every run of the reference ends with (/root/reference/eval.py:30-56 ->
// metric.all_mesh_metrics, metric.py:56-63): area-weighted surface samples on both meshes, nearest neighbours in both
// directions, Chamfer distance and F-score.  Stand-alone maps on [dev] arrays like frames.hip: no solver context, no
// allocation and no synchronisation on the per-frame path; every buffer, scratch included, is the caller's.
//
// The hot path is k_nn_d2: brute force, exact, no worst case.  2 * n_src * n_dst point pairs per frame (2e10 at the
// reference's 100,000 samples), VALU-bound: per pair of targets and per query 3 packed subtracts, 1 packed multiply,
// 2 packed FMAs and one three-way minimum.  Measured numbers: DESIGN.md section 8, profiles/geo_metrics_bench.*.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "entry.hpp"
#include "geo_math.hpp"

namespace {

using namespace entry;
using geo::P3;

constexpr int TPB = 256;
#ifndef GEO_NN_Q
#define GEO_NN_Q 4  // queries per lane (chosen by measurement)
#endif
constexpr int NN_Q = GEO_NN_Q;
constexpr int NN_TILE = 1024;  // targets staged in LDS at a time (12 KB)
constexpr int NN_CHUNK = 32;   // targets between two looks at "did this lane's minimum move"
static_assert(NN_TILE % NN_CHUNK == 0 && NN_CHUNK % 2 == 0, "tiles are whole chunks, chunks whole pairs");
constexpr int RED_BLOCKS = MPMHIP_GEO_REDUCE_SCRATCH / 4;  // workgroups per distance array in k_geo_partial

typedef float f2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ P3 ld3(const float *p, size_t i) { return P3{p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }

__global__ void k_face_areas(const float *verts, const int32_t *faces, int n_f, float *area) {
  int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_f) return;
  const int32_t *t = faces + 3 * (size_t)f;
  area[f] = geo::face_area(ld3(verts, t[0]), ld3(verts, t[1]), ld3(verts, t[2]));
}

// trimesh.sample.sample_surface: face = searchsorted(cumsum(area), u0 * total) (side = "left": the FIRST face whose
// cumulative area reaches the pick, so a zero-area face that repeats its predecessor's value is never chosen), then
// sample_point with (u1, u2).
__global__ void k_mesh_sample(const float *verts, const int32_t *faces, int n_f, const double *cdf, const float *uniforms,
                              int n, float *points, int32_t *face_index) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float *u = uniforms + 3 * (size_t)i;
  double pick = (double)u[0] * cdf[n_f - 1];
  int lo = 0, hi = n_f;  // first f in [0, n_f) with cdf[f] >= pick; n_f if none (a non-finite cdf), clamped below
  while (lo < hi) {
    int mid = lo + (hi - lo) / 2;
    if (cdf[mid] < pick) lo = mid + 1; else hi = mid;
  }
  int f = lo < n_f - 1 ? lo : n_f - 1;
  const int32_t *t = faces + 3 * (size_t)f;
  P3 p = geo::sample_point(ld3(verts, t[0]), ld3(verts, t[1]), ld3(verts, t[2]), u[1], u[2]);
  points[3 * (size_t)i] = p.x; points[3 * (size_t)i + 1] = p.y; points[3 * (size_t)i + 2] = p.z;
  if (face_index) face_index[i] = f;
}

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
__global__ __launch_bounds__(TPB) void k_nn_d2(const float *__restrict__ src, int n_src, const float *__restrict__ dst,
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

__global__ void k_nn_unpack(const unsigned long long *best, int n, float *dist2, int32_t *index) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned long long b = best[i];
  dist2[i] = __uint_as_float((unsigned)(b >> 32));
  if (index) index[i] = (int32_t)(unsigned)(b & 0xffffffffull);
}

// First level of the reduction: workgroup (x, array y) sums d2 in fp64 and counts d2 <= tau over its elements
// x * TPB + tid, + RED_BLOCKS * TPB, ... in that order, then folds its lanes pairwise in LDS (a fixed tree), and writes
// its partial to scratch[(y * RED_BLOCKS + x) * 2 + {0, 1}].  No floating-point atomics anywhere: the same input gives
// the same bits.
__global__ __launch_bounds__(TPB) void k_geo_partial(const float *d12, int n1, const float *d21, int n2, double tau,
                                                     double *scratch) {
  __shared__ double s_sum[TPB], s_cnt[TPB];
  const float *d = blockIdx.y ? d21 : d12;
  const int n = blockIdx.y ? n2 : n1;
  double sum = 0.0, cnt = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)RED_BLOCKS * TPB) {
    float v = d[i];
    sum += (double)v;
    cnt += geo::below(v, tau) ? 1.0 : 0.0;
  }
  s_sum[threadIdx.x] = sum; s_cnt[threadIdx.x] = cnt;
  __syncthreads();
  for (int w = TPB / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) { s_sum[threadIdx.x] += s_sum[threadIdx.x + w]; s_cnt[threadIdx.x] += s_cnt[threadIdx.x + w]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double *o = scratch + ((size_t)blockIdx.y * RED_BLOCKS + blockIdx.x) * 2;
    o[0] = s_sum[0]; o[1] = s_cnt[0];
  }
}

// Second level: one lane adds the partials in index order and applies the reference's formulas.
__global__ void k_geo_final(const double *scratch, int n1, int n2, double *out) {
  double sum[2] = {0.0, 0.0}, cnt[2] = {0.0, 0.0};
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < RED_BLOCKS; ++b) {
      sum[a] += scratch[((size_t)a * RED_BLOCKS + b) * 2];
      cnt[a] += scratch[((size_t)a * RED_BLOCKS + b) * 2 + 1];
    }
  geo::FScore f = geo::fscore_from_counts(cnt[0], (double)n1, cnt[1], (double)n2);
  out[0] = f.fscore;
  out[1] = geo::chamfer_from_sums(sum[0], (double)n1, sum[1], (double)n2);
  out[2] = f.precision;
  out[3] = f.recall;
}

}  // namespace

extern "C" {

int mpmhip_face_areas(int32_t device, void *stream, const float *verts, const int32_t *faces, int32_t n_faces, float *area) {
  if (n_faces <= 0 || !verts || !faces || !area) return MPMHIP_ERR_INVALID;
  if (int rc = select_device(device)) return rc;
  hipLaunchKernelGGL(k_face_areas, blocks(n_faces, TPB), TPB, 0, (hipStream_t)stream, verts, faces, n_faces, area);
  return check(hipGetLastError());
}

int mpmhip_mesh_sample(int32_t device, void *stream, const float *verts, const int32_t *faces, int32_t n_faces,
                       const double *area_cdf, const float *uniforms, int32_t n_samples, float *points,
                       int32_t *face_index) {
  if (n_faces <= 0 || n_samples <= 0 || !verts || !faces || !area_cdf || !uniforms || !points) return MPMHIP_ERR_INVALID;
  if (int rc = select_device(device)) return rc;
  hipLaunchKernelGGL(k_mesh_sample, blocks(n_samples, TPB), TPB, 0, (hipStream_t)stream, verts, faces, n_faces, area_cdf, uniforms,
                     n_samples, points, face_index);
  return check(hipGetLastError());
}

int mpmhip_nn_dist2(int32_t device, void *stream, const float *src, int32_t n_src, const float *dst, int32_t n_dst,
                    int32_t slices, uint64_t *best_scratch, float *dist2, int32_t *index) {
  if (n_src <= 0 || n_dst <= 0 || slices < 0 || !src || !dst || !best_scratch || !dist2) return MPMHIP_ERR_INVALID;
  if (int rc = select_device(device)) return rc;
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
  hipStream_t s = (hipStream_t)stream;
  ENTRY_CHECK(hipMemsetAsync(best_scratch, 0xff, (size_t)n_src * sizeof(uint64_t), s));
  hipLaunchKernelGGL(k_nn_d2, dim3((unsigned)tiles, (unsigned)slices), TPB, 0, s, src, n_src, dst, n_dst, slice_len,
                     (unsigned long long *)best_scratch);
  hipLaunchKernelGGL(k_nn_unpack, blocks(n_src, TPB), TPB, 0, s, (const unsigned long long *)best_scratch, n_src, dist2, index);
  return check(hipGetLastError());
}

int mpmhip_geo_reduce(int32_t device, void *stream, const float *dist2_12, int32_t n1, const float *dist2_21, int32_t n2,
                      double tau, double *scratch, double *out) {
  if (n1 <= 0 || n2 <= 0 || !dist2_12 || !dist2_21 || !scratch || !out) return MPMHIP_ERR_INVALID;
  if (int rc = select_device(device)) return rc;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_geo_partial, dim3(RED_BLOCKS, 2), TPB, 0, s, dist2_12, n1, dist2_21, n2, tau, scratch);
  hipLaunchKernelGGL(k_geo_final, 1, 1, 0, s, (const double *)scratch, n1, n2, out);
  return check(hipGetLastError());
}

}  // extern "C"
