// geo.hip -- the geometry evaluation every run of the reference ends with (/root/reference/eval.py:30-56 ->
// metric.all_mesh_metrics, metric.py:56-63): area-weighted surface samples on both meshes, nearest neighbours in both
// directions, Chamfer distance and F-score.  Stand-alone maps on [dev] arrays like frames.hip: no solver context, no
// allocation and no synchronisation on the per-frame path; every buffer, scratch included, is the caller's.
//
// The hot path is k_nn_d2 (nn_device.hpp, which track.hip launches too): brute force, exact, no worst case.
// 2 * n_src * n_dst point pairs per frame (2e10 at the reference's 100,000 samples), VALU-bound: per pair of targets and per query 3 packed subtracts, 1 packed multiply,
// 2 packed FMAs and one three-way minimum.  Measured numbers: DESIGN.md section 8, profiles/geo_metrics_bench.*.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "entry.hpp"
#include "geo_math.hpp"
#include "nn_device.hpp"

namespace {

using namespace entry;
using geo::P3;

constexpr int TPB = nn::TPB;
constexpr int RED_BLOCKS = MPMHIP_GEO_REDUCE_SCRATCH / 4;  // workgroups per distance array in k_geo_partial

using nn::ld3;

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
  hipStream_t s = (hipStream_t)stream;
  if (int rc = nn::launch_nearest(s, src, n_src, dst, n_dst, slices, best_scratch)) return rc;
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
