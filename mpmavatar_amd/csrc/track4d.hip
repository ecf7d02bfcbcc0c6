// track4d.hip -- the two terms the 4D-DRESS tracking script adds to the tracking step (preprocess/train_mesh_lbs_4ddress.py): the
// uniform Laplacian of :363 without the dense [V, V] matrix of :212-214, and scale_ratio_loss (:279-292).  The math is
// track4d_math.hpp; the kernels here are one thread per vertex or face over it.
//   laplacian forward   k_lap_rows: a gather over the CSR vertex adjacency, Lv [V, 3] and one double per workgroup; k_lap_finish
//   its backward        k_lap_backward: the same gather over the saved Lv; reads neither the vertices nor anything that depends on them
//   scale ratio         k_scale_rows (four doubles per workgroup: the two hinges, q and q^2) + k_scale_finish (one workgroup)
//   its backward        k_scale_stencil writes d_stencil[f, 3, 3] and d_scales[f, 3]; k_corner_sum walks each vertex's CSR segment of
//                       those rows in ascending order, as track.hip does
// No floating-point atomics: sums are wave shuffles, then LDS in wave order, then doubles per workgroup in the caller's scratch, then
// a single workgroup that adds those in index order.  Nothing here allocates or synchronises.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "block_sum.hpp"
#include "entry.hpp"
#include "track4d_math.hpp"

namespace {

using namespace entry;
constexpr int TPB = MPMHIP_TRACK_TPB;  // the scratch-size macros of mpmhip.h count workgroups of this size
constexpr int WAVES = TPB / 64;
static_assert(TPB == 256, "block_sum folds four waves");

// partials [gridDim.x] doubles (NULL: Lv alone); lv may be NULL (the value alone)
__global__ __launch_bounds__(TPB) void k_lap_rows(int n_v, const float *__restrict__ verts, const int32_t *__restrict__ start,
                                                  const int32_t *__restrict__ nbr, float *__restrict__ lv, double *__restrict__ partials) {
  __shared__ double red[1][WAVES];
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  double v[1] = {0.0};
  if (i < n_v) {
    float norm;
    const trk::V3 l = trk4::laplacian_row(i, n_v, verts, start, nbr, norm);
    if (lv) trk::st3(lv, i, l);
    v[0] = (double)norm;
  }
  if (!partials) return;  // uniform over the grid
  block_sum(v, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = v[0];
}

// One workgroup.  Lane t adds the partials t, t + TPB, ... in that order (more than one pass above TPB * TPB vertices).
__global__ __launch_bounds__(TPB) void k_lap_finish(int n_v, int n_partials, const double *__restrict__ partials, float *__restrict__ value) {
  __shared__ double red[1][WAVES];
  double v[1] = {0.0};
  for (int t = threadIdx.x; t < n_partials; t += TPB) v[0] += partials[t];
  block_sum(v, red);
  if (threadIdx.x == 0) value[0] = (float)(v[0] / (double)n_v);
}

__global__ __launch_bounds__(TPB) void k_lap_backward(int n_v, const float *__restrict__ lv, const int32_t *__restrict__ start,
                                                      const int32_t *__restrict__ nbr, const float *__restrict__ g, float *__restrict__ d_verts) {
  const int64_t j = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (j >= n_v) return;
  trk4::laplacian_backward(j, n_v, lv, start, nbr, g, d_verts);
}

// partials [gridDim.x * 4] doubles: the workgroup's sums of the two hinges, of q and of q^2 (the square of an fp32 is exact in fp64)
__global__ __launch_bounds__(TPB) void k_scale_rows(int n_f, int n_v, const float *__restrict__ verts, const int32_t *__restrict__ faces,
                                                    const float *__restrict__ scales, float th_ratio, float th_edge,
                                                    double *__restrict__ partials) {
  __shared__ double red[4][WAVES];
  const int64_t f = (int64_t)blockIdx.x * TPB + threadIdx.x;
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  if (f < n_f) {
    const trk4::ScaleTerms t = trk4::scale_terms_forward(f, n_v, verts, faces, scales, th_ratio, th_edge);
    v[0] = (double)t.ratio; v[1] = (double)t.edge; v[2] = (double)t.q; v[3] = (double)t.q * (double)t.q;
  }
  block_sum(v, red);
  if (threadIdx.x == 0) {
    double *o = partials + (size_t)blockIdx.x * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = v[k];
  }
}

// One workgroup.  terms [4]: the two hinge means, the unbiased variance of q (0 / 0 = NaN for one face, as torch.var) and the mean of
// q, which the backward reads.
__global__ __launch_bounds__(TPB) void k_scale_finish(int n_f, int n_partials, const double *__restrict__ partials, float *__restrict__ terms) {
  __shared__ double red[4][WAVES];
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (int t = threadIdx.x; t < n_partials; t += TPB)
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] += partials[4 * (size_t)t + k];
  block_sum(v, red);
  if (threadIdx.x == 0) {
    const double n = (double)n_f;
    terms[0] = (float)(v[0] / n);
    terms[1] = (float)(v[1] / n);
    terms[2] = (float)((v[3] - v[2] * v[2] / n) / (n - 1.0));
    terms[3] = (float)(v[2] / n);
  }
}

__global__ __launch_bounds__(TPB) void k_scale_stencil(int n_f, int n_v, const float *__restrict__ verts, const int32_t *__restrict__ faces,
                                                       const float *__restrict__ scales, float th_ratio, float th_edge,
                                                       const float *__restrict__ terms, const float *__restrict__ g,
                                                       float *__restrict__ d_stencil, float *__restrict__ d_scales) {
  const int64_t f = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (f >= n_f) return;
  trk4::scale_terms_backward(f, n_f, n_v, verts, faces, scales, th_ratio, th_edge, terms[3], g, d_stencil, d_scales);
}

__global__ __launch_bounds__(TPB) void k_corner_sum(int n_v, const int32_t *__restrict__ start, const int32_t *__restrict__ items,
                                                    const float *__restrict__ d_stencil, float *__restrict__ d_verts) {
  const int64_t v = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (v >= n_v) return;
  fgrad::vertex_gather(v, start, items, d_stencil, d_verts);
}

bool table_ok(int32_t n_verts, const int32_t *nbr_start, const int32_t *nbr, int32_t n_nbr) {
  if (n_verts <= 0 || n_nbr < 0 || !nbr_start) return false;
  return n_nbr == 0 || nbr;
}

bool faces_ok(const float *verts, int32_t n_verts, const int32_t *faces, int32_t n_faces, const float *scales) {
  if (n_verts <= 0 || n_faces <= 0 || (int64_t)n_faces * 3 > INT32_MAX) return false;
  return verts && faces && scales;
}

}  // namespace

extern "C" {

int mpmhip_track4d_laplacian_forward(int32_t device, void *stream, const float *verts, int32_t n_verts, const int32_t *nbr_start,
                                     const int32_t *nbr, int32_t n_nbr, double *scratch, int32_t n_scratch, float *out_lv, float *out_value) {
  if (!table_ok(n_verts, nbr_start, nbr, n_nbr) || !verts) return MPMHIP_ERR_INVALID;
  if (out_value && (!scratch || (int64_t)n_scratch < MPMHIP_TRACK4D_LAPLACIAN_SCRATCH(n_verts))) return MPMHIP_ERR_INVALID;
  if (int rc = device_in_range(device)) return rc;
  if (!out_lv && !out_value) return MPMHIP_OK;
  ENTRY_CHECK(hipSetDevice(device));
  const unsigned n_wg = blocks(n_verts, TPB);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_lap_rows, n_wg, TPB, 0, s, n_verts, verts, nbr_start, nbr, out_lv, out_value ? scratch : nullptr);
  ENTRY_CHECK(hipGetLastError());
  if (out_value) hipLaunchKernelGGL(k_lap_finish, 1, TPB, 0, s, n_verts, (int)n_wg, (const double *)scratch, out_value);
  return check(hipGetLastError());
}

int mpmhip_track4d_laplacian_backward(int32_t device, void *stream, const float *lv, int32_t n_verts, const int32_t *nbr_start,
                                      const int32_t *nbr, int32_t n_nbr, const float *g, float *d_verts) {
  if (!table_ok(n_verts, nbr_start, nbr, n_nbr) || !lv || !g) return MPMHIP_ERR_INVALID;
  if (int rc = device_in_range(device)) return rc;
  if (!d_verts) return MPMHIP_OK;
  ENTRY_CHECK(hipSetDevice(device));
  hipLaunchKernelGGL(k_lap_backward, blocks(n_verts, TPB), TPB, 0, (hipStream_t)stream, n_verts, lv, nbr_start, nbr, g, d_verts);
  return check(hipGetLastError());
}

int mpmhip_track4d_scale_ratio_forward(int32_t device, void *stream, const float *verts, int32_t n_verts, const int32_t *faces, int32_t n_faces,
                                       const float *scales, float th_ratio, float th_edge, double *scratch, int32_t n_scratch,
                                       float *out_terms) {
  if (!faces_ok(verts, n_verts, faces, n_faces, scales) || !scratch || !out_terms) return MPMHIP_ERR_INVALID;
  if ((int64_t)n_scratch < MPMHIP_TRACK4D_SCALE_RATIO_SCRATCH(n_faces)) return MPMHIP_ERR_INVALID;
  if (int rc = device_in_range(device)) return rc;
  ENTRY_CHECK(hipSetDevice(device));
  const unsigned n_wg = blocks(n_faces, TPB);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_scale_rows, n_wg, TPB, 0, s, n_faces, n_verts, verts, faces, scales, th_ratio, th_edge, scratch);
  ENTRY_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_scale_finish, 1, TPB, 0, s, n_faces, (int)n_wg, (const double *)scratch, out_terms);
  return check(hipGetLastError());
}

int mpmhip_track4d_scale_ratio_backward(int32_t device, void *stream, const float *verts, int32_t n_verts, const int32_t *faces,
                                        int32_t n_faces, const float *scales, float th_ratio, float th_edge, const float *terms,
                                        const float *g_terms, const int32_t *vert_start, const int32_t *vert_items, float *d_stencil,
                                        float *d_verts, float *d_scales) {
  if (!faces_ok(verts, n_verts, faces, n_faces, scales) || !terms || !g_terms) return MPMHIP_ERR_INVALID;
  if (d_verts && (!vert_start || !vert_items || !d_stencil)) return MPMHIP_ERR_INVALID;
  if (int rc = device_in_range(device)) return rc;
  if (!d_verts && !d_scales) return MPMHIP_OK;
  ENTRY_CHECK(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_scale_stencil, blocks(n_faces, TPB), TPB, 0, s, n_faces, n_verts, verts, faces, scales, th_ratio, th_edge, terms,
                     g_terms, d_verts ? d_stencil : nullptr, d_scales);
  ENTRY_CHECK(hipGetLastError());
  if (d_verts) hipLaunchKernelGGL(k_corner_sum, blocks(n_verts, TPB), TPB, 0, s, n_verts, vert_start, vert_items, (const float *)d_stencil, d_verts);
  return check(hipGetLastError());
}

}  // extern "C"
