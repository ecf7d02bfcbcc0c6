// reg.hip -- the regularisation terms of the appearance loop on the device (train_appearance.py:136-150): mpmhip_mesh_reg_forward /
// _backward (normal_loss, iso_loss, area_loss of scene/mesh_gaussian_model.py:203-246) and mpmhip_gauss_reg_forward / _backward
// (opacity_loss, and the xyz and scale lines of train_appearance.py:147-148).  The math is reg_math.hpp; the kernels here are one
// thread per face, vertex or Gaussian over it.
// Mesh forward, two launches: k_mesh_rows (a face gathers its own three vertices and its K neighbours' nine -- the vertex array is
// L2-resident, so a neighbour's normal and centre are recomputed rather than stored: 12 B of faces + 12 B of nb + 24 B of nd, nw in,
// 4 B of area out per face, the 144 B of vertices from cache) and k_mesh_finish (one workgroup: the three sums, then mean(a), then
// the sums of |a_f - mean| and sign(a_f - mean) over the stored areas).  Mesh backward, two launches: k_mesh_stencil writes the
// 144 B row d_stencil[f, 1 + K, 3, 3] per face, k_vertex_sum walks each vertex's CSR segment of those rows in ascending order.
// Gaussians, 28 B in per row forward (+ 4 B radii or 1 B mask) and 28 B out backward: k_gauss_rows + k_gauss_finish, then one
// elementwise k_gauss_backward.
// No floating-point atomics: every sum is wave shuffles, then LDS in wave order, then one double per workgroup in the caller's
// scratch, then a single workgroup that adds those in index order.  The same input gives the same bits.  Nothing here allocates or
// synchronises; the upstream gradients and the visible count are read from device memory.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "block_sum.hpp"
#include "entry.hpp"
#include "reg_math.hpp"

namespace {

using namespace entry;
constexpr int TPB = MPMHIP_REG_TPB;  // the scratch-size macros of mpmhip.h count workgroups of this size
constexpr int WAVES = TPB / 64;
static_assert(TPB == 256 && TPB % 64 == 0, "block_sum folds four waves");

// partials [gridDim.x * 3] doubles: the workgroup's sums of |m_f - 1|, the iso terms and a_f; area [F]
__global__ __launch_bounds__(TPB) void k_mesh_rows(int n_f, int n_v, const float *__restrict__ verts, const int32_t *__restrict__ faces,
                                                   const int32_t *__restrict__ nb, const float *__restrict__ nd, const float *__restrict__ nw,
                                                   float *__restrict__ sq_dist, float *__restrict__ area, double *__restrict__ partials) {
  __shared__ double red[3][WAVES];
  const int64_t f = (int64_t)blockIdx.x * TPB + threadIdx.x;
  double v[3] = {0.0, 0.0, 0.0};
  if (f < n_f) {
    const reg::FaceTerms t = reg::face_forward(f, n_f, n_v, verts, faces, nb, nd, nw, sq_dist);
    area[f] = t.area;
    v[0] = (double)t.normal; v[1] = (double)t.iso; v[2] = (double)t.area;
  }
  block_sum(v, red);
  if (threadIdx.x == 0) {
    double *o = partials + (size_t)blockIdx.x * 3;
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
  }
}

// One workgroup.  Lane t adds the partial triples t, t + TPB, ... in that order (more than one pass above TPB * TPB faces), the
// lanes are folded as in block_sum; the mean area leaves as fp32 and every lane then walks area[t], area[t + TPB], ...
// terms [3] = normal, iso, area; stats [2] = mean(a), mean(sign(a - mean(a))).
__global__ __launch_bounds__(TPB) void k_mesh_finish(int n_f, int n_partials, const double *__restrict__ partials, const float *__restrict__ area,
                                                     float *__restrict__ terms, float *__restrict__ stats) {
  __shared__ double red[3][WAVES];
  __shared__ float s_mean;
  double v[3] = {0.0, 0.0, 0.0};
  for (int t = threadIdx.x; t < n_partials; t += TPB) { v[0] += partials[3 * (size_t)t]; v[1] += partials[3 * (size_t)t + 1]; v[2] += partials[3 * (size_t)t + 2]; }
  block_sum(v, red);
  if (threadIdx.x == 0) {
    terms[0] = (float)(v[0] / (double)n_f);
    terms[1] = (float)(v[1] / ((double)n_f * reg::K));
    s_mean = (float)(v[2] / (double)n_f);
  }
  __syncthreads();
  const float mean = s_mean;
  double w[2] = {0.0, 0.0};
  for (int f = threadIdx.x; f < n_f; f += TPB) {
    const float d = area[f] - mean;
    w[0] += (double)__builtin_fabsf(d);
    w[1] += (double)reg::sign(d);
  }
  block_sum(w, red);
  if (threadIdx.x == 0) {
    terms[2] = (float)(w[0] / (double)n_f);
    stats[0] = mean;
    stats[1] = (float)(w[1] / (double)n_f);
  }
}

__global__ __launch_bounds__(TPB) void k_mesh_stencil(int n_f, int n_v, const float *__restrict__ verts, const int32_t *__restrict__ faces,
                                                      const int32_t *__restrict__ nb, const float *__restrict__ nd, const float *__restrict__ nw,
                                                      const float *__restrict__ stats, const float *__restrict__ g, float *__restrict__ d_stencil) {
  const int64_t f = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (f >= n_f) return;
  reg::face_backward(f, n_f, n_v, verts, faces, nb, nd, nw, stats, g, d_stencil);
}

__global__ __launch_bounds__(TPB) void k_vertex_sum(int n_v, const int32_t *__restrict__ start, const int32_t *__restrict__ items,
                                                    const float *__restrict__ d_stencil, float *__restrict__ d_verts) {
  const int64_t v = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (v >= n_v) return;
  fgrad::vertex_gather(v, start, items, d_stencil, d_verts);
}

// partials [gridDim.x * 4] doubles: the workgroup's sums of the three summands and its count of visible rows
__global__ __launch_bounds__(TPB) void k_gauss_rows(int n, const float *__restrict__ opacity, const float *__restrict__ xyz,
                                                    const float *__restrict__ scaling, const int32_t *__restrict__ radii,
                                                    const uint8_t *__restrict__ mask, float t_xyz, float t_scale, double *__restrict__ partials) {
  __shared__ double red[4][WAVES];
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  if (i < n) {
    const reg::GaussTerms t = reg::gauss_forward(i, opacity, xyz, scaling, radii, mask, t_xyz, t_scale);
    v[0] = (double)t.opacity; v[1] = (double)t.xyz; v[2] = (double)t.scale; v[3] = t.visible ? 1.0 : 0.0;
  }
  block_sum(v, red);
  if (threadIdx.x == 0) {
    double *o = partials + (size_t)blockIdx.x * 4;
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = v[3];
  }
}

// One workgroup.  No visible row: 0 / 0 = NaN for xyz and scale, as the reference's mean of an empty tensor.
__global__ __launch_bounds__(TPB) void k_gauss_finish(int n, int n_partials, const double *__restrict__ partials, float *__restrict__ terms,
                                                      int32_t *__restrict__ n_visible) {
  __shared__ double red[4][WAVES];
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (int t = threadIdx.x; t < n_partials; t += TPB)
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] += partials[4 * (size_t)t + k];
  block_sum(v, red);
  if (threadIdx.x == 0) {
    terms[0] = (float)(v[0] / (double)n);
    terms[1] = (float)(v[1] / v[3]);
    terms[2] = (float)(v[2] / v[3]);
    n_visible[0] = (int32_t)v[3];
  }
}

__global__ __launch_bounds__(TPB) void k_gauss_backward(int n, const float *__restrict__ opacity, const float *__restrict__ xyz,
                                                        const float *__restrict__ scaling, const int32_t *__restrict__ radii,
                                                        const uint8_t *__restrict__ mask, float t_xyz, float t_scale,
                                                        const int32_t *__restrict__ n_visible, const float *__restrict__ g,
                                                        float *__restrict__ d_opacity, float *__restrict__ d_xyz, float *__restrict__ d_scaling) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  reg::gauss_backward(i, n, opacity, xyz, scaling, radii, mask, t_xyz, t_scale, n_visible, g, d_opacity, d_xyz, d_scaling);
}

// what both mesh entry points require of the inputs they share; 12 * n_faces stencil items must stay an int32
bool mesh_ok(const float *verts, int32_t n_verts, const int32_t *faces, int32_t n_faces, const int32_t *nb, const float *nd, const float *nw) {
  if (n_verts < 0 || n_faces < 0 || (int64_t)n_faces * reg::ROW > INT32_MAX) return false;
  if (n_faces > 0 && (!verts || !faces || !nb || !nd || !nw)) return false;
  return true;
}

// exactly one of radii / visible names the visible rows
bool gauss_ok(int32_t n, const float *opacity, const float *xyz, const float *scaling, const int32_t *radii, const uint8_t *visible) {
  if (n < 0 || (radii != nullptr) == (visible != nullptr)) return false;
  if (n > 0 && (!opacity || !xyz || !scaling)) return false;
  return true;
}

}  // namespace

extern "C" {

int mpmhip_mesh_reg_forward(int32_t device, void *stream, const float *verts, int32_t n_verts, const int32_t *faces, int32_t n_faces,
                            const int32_t *face_neighbors, const float *neighbor_dist, const float *neighbor_weight, double *scratch,
                            float *out_terms, float *out_stats, float *out_sq_dist) {
  if (!mesh_ok(verts, n_verts, faces, n_faces, face_neighbors, neighbor_dist, neighbor_weight)) return MPMHIP_ERR_INVALID;
  if (!scratch || !out_terms || !out_stats) return MPMHIP_ERR_INVALID;
  if (int rc = device_in_range(device)) return rc;
  if (n_faces == 0) return MPMHIP_OK;
  ENTRY_CHECK(hipSetDevice(device));
  const unsigned n_wg = blocks(n_faces, TPB);
  float *area = (float *)(scratch + 3 * (size_t)n_wg);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_mesh_rows, n_wg, TPB, 0, s, n_faces, n_verts, verts, faces, face_neighbors, neighbor_dist, neighbor_weight, out_sq_dist,
                     area, scratch);
  ENTRY_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_mesh_finish, 1, TPB, 0, s, n_faces, (int)n_wg, (const double *)scratch, (const float *)area, out_terms, out_stats);
  return check(hipGetLastError());
}

int mpmhip_mesh_reg_backward(int32_t device, void *stream, const float *verts, int32_t n_verts, const int32_t *faces, int32_t n_faces,
                             const int32_t *face_neighbors, const float *neighbor_dist, const float *neighbor_weight, const float *stats,
                             const float *g_terms, const int32_t *vert_start, const int32_t *vert_items, float *d_stencil, float *d_verts) {
  if (!mesh_ok(verts, n_verts, faces, n_faces, face_neighbors, neighbor_dist, neighbor_weight)) return MPMHIP_ERR_INVALID;
  if (!stats || !g_terms || !vert_start || (n_faces > 0 && (!vert_items || !d_stencil))) return MPMHIP_ERR_INVALID;
  if (int rc = device_in_range(device)) return rc;
  if (!d_verts || n_verts == 0) return MPMHIP_OK;
  ENTRY_CHECK(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  if (n_faces > 0) {
    hipLaunchKernelGGL(k_mesh_stencil, blocks(n_faces, TPB), TPB, 0, s, n_faces, n_verts, verts, faces, face_neighbors, neighbor_dist,
                       neighbor_weight, stats, g_terms, d_stencil);
    ENTRY_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_vertex_sum, blocks(n_verts, TPB), TPB, 0, s, n_verts, vert_start, vert_items, (const float *)d_stencil, d_verts);
  return check(hipGetLastError());
}

int mpmhip_gauss_reg_forward(int32_t device, void *stream, int32_t n, const float *opacity, const float *xyz, const float *scaling,
                             const int32_t *radii, const uint8_t *visible, float threshold_xyz, float threshold_scale, double *scratch,
                             float *out_terms, int32_t *out_n_visible) {
  if (!gauss_ok(n, opacity, xyz, scaling, radii, visible) || !scratch || !out_terms || !out_n_visible) return MPMHIP_ERR_INVALID;
  if (int rc = device_in_range(device)) return rc;
  if (n == 0) return MPMHIP_OK;
  ENTRY_CHECK(hipSetDevice(device));
  const unsigned n_wg = blocks(n, TPB);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_gauss_rows, n_wg, TPB, 0, s, n, opacity, xyz, scaling, radii, visible, threshold_xyz, threshold_scale, scratch);
  ENTRY_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_gauss_finish, 1, TPB, 0, s, n, (int)n_wg, (const double *)scratch, out_terms, out_n_visible);
  return check(hipGetLastError());
}

int mpmhip_gauss_reg_backward(int32_t device, void *stream, int32_t n, const float *opacity, const float *xyz, const float *scaling,
                              const int32_t *radii, const uint8_t *visible, float threshold_xyz, float threshold_scale,
                              const int32_t *n_visible, const float *g_terms, float *d_opacity, float *d_xyz, float *d_scaling) {
  if (!gauss_ok(n, opacity, xyz, scaling, radii, visible) || !n_visible || !g_terms) return MPMHIP_ERR_INVALID;
  if (int rc = device_in_range(device)) return rc;
  if (n == 0 || (!d_opacity && !d_xyz && !d_scaling)) return MPMHIP_OK;
  ENTRY_CHECK(hipSetDevice(device));
  hipLaunchKernelGGL(k_gauss_backward, blocks(n, TPB), TPB, 0, (hipStream_t)stream, n, opacity, xyz, scaling, radii, visible, threshold_xyz,
                     threshold_scale, n_visible, g_terms, d_opacity, d_xyz, d_scaling);
  return check(hipGetLastError());
}

}  // extern "C"
