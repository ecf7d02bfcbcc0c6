// track.hip -- the mesh tracking step on the device (preprocess/train_mesh_lbs_actorshq.py:209-279): everything between the trained
// vertices and the rasteriser's argument list (params2rendervar: one Gaussian per face), the loss terms area, scale and opacity,
// compute_vertex_normals, and collision_penalty without the [n_cloth, n_body] distance matrix.  The math is track_math.hpp; the
// kernels here are one thread per face, vertex or cloth point over it.
//   render_vars      one launch: 12 B of faces + 16 B of parameters in, 44 B out per face, the 36 B of vertices from cache
//   its backward     k_render_stencil writes d_stencil[f, 3, 3] (36 B) and the two elementwise gradients per face; k_vertex_sum walks
//                    each vertex's CSR segment of those rows in ascending order
//   terms            k_terms_rows (one double triple per workgroup) + k_terms_finish (one workgroup); backward as above
//   vertex normals   a gather over the same CSR table, ascending faces: not an index_add, so the bits repeat
//   collision        k_nn_d2 (nn_device.hpp, the kernel of mpmhip_nn_dist2), then k_collision_rows (gathers vb[j] and nb[j], the
//                    distance, the hinge, one double per workgroup) and k_collision_finish
// No floating-point atomics: sums are wave shuffles, then LDS in wave order, then one double per workgroup in the caller's scratch,
// then a single workgroup that adds those in index order.  Nothing here allocates or synchronises; upstream gradients are read from
// device memory.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "block_sum.hpp"
#include "entry.hpp"
#include "nn_device.hpp"
#include "track_math.hpp"

namespace {

using namespace entry;
constexpr int TPB = MPMHIP_TRACK_TPB;  // the scratch-size macros of mpmhip.h count workgroups of this size
constexpr int WAVES = TPB / 64;
static_assert(TPB == 256 && TPB == nn::TPB, "block_sum folds four waves");

__global__ __launch_bounds__(TPB) void k_render_vars(int n_f, int n_v, const float *__restrict__ verts, const int32_t *__restrict__ faces,
                                                     const float *__restrict__ log_scales, const float *__restrict__ logit_opac,
                                                     float *__restrict__ means, float *__restrict__ rot, float *__restrict__ scales,
                                                     float *__restrict__ opac) {
  const int64_t f = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (f >= n_f) return;
  trk::render_vars_forward(f, n_v, verts, faces, log_scales, logit_opac, means, rot, scales, opac);
}

__global__ __launch_bounds__(TPB) void k_render_stencil(int n_f, int n_v, const float *__restrict__ verts, const int32_t *__restrict__ faces,
                                                        const float *__restrict__ log_scales, const float *__restrict__ logit_opac,
                                                        const float *__restrict__ g_means, const float *__restrict__ g_rot,
                                                        const float *__restrict__ g_scales, const float *__restrict__ g_opac,
                                                        float *__restrict__ d_stencil, float *__restrict__ d_log_scales,
                                                        float *__restrict__ d_logit_opac) {
  const int64_t f = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (f >= n_f) return;
  trk::render_vars_backward(f, n_v, verts, faces, log_scales, logit_opac, g_means, g_rot, g_scales, g_opac, d_stencil, d_log_scales,
                            d_logit_opac);
}

__global__ __launch_bounds__(TPB) void k_vertex_sum(int n_v, const int32_t *__restrict__ start, const int32_t *__restrict__ items,
                                                    const float *__restrict__ d_stencil, float *__restrict__ d_verts) {
  const int64_t v = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (v >= n_v) return;
  fgrad::vertex_gather(v, start, items, d_stencil, d_verts);
}

__global__ __launch_bounds__(TPB) void k_face_geometry(int n_f, int n_v, const float *__restrict__ verts, const int32_t *__restrict__ faces,
                                                       float *__restrict__ normals, float *__restrict__ areas) {
  const int64_t f = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (f >= n_f) return;
  trk::face_geometry(f, n_v, verts, faces, normals, areas);
}

// partials [gridDim.x * 3] doubles: the workgroup's sums of | a_f - pi s0 s1 |, s2 and 1 - sigmoid
__global__ __launch_bounds__(TPB) void k_terms_rows(int n_f, int n_v, const float *__restrict__ verts, const int32_t *__restrict__ faces,
                                                    const float *__restrict__ log_scales, const float *__restrict__ logit_opac,
                                                    double *__restrict__ partials) {
  __shared__ double red[3][WAVES];
  const int64_t f = (int64_t)blockIdx.x * TPB + threadIdx.x;
  double v[3] = {0.0, 0.0, 0.0};
  if (f < n_f) {
    const trk::Terms t = trk::terms_forward(f, n_v, verts, faces, log_scales, logit_opac);
    v[0] = (double)t.area; v[1] = (double)t.scale; v[2] = (double)t.opacity;
  }
  block_sum(v, red);
  if (threadIdx.x == 0) {
    double *o = partials + (size_t)blockIdx.x * 3;
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
  }
}

// One workgroup.  Lane t adds the partial triples t, t + TPB, ... in that order (more than one pass above TPB * TPB faces).
__global__ __launch_bounds__(TPB) void k_terms_finish(int n_f, int n_partials, const double *__restrict__ partials, float *__restrict__ terms) {
  __shared__ double red[3][WAVES];
  double v[3] = {0.0, 0.0, 0.0};
  for (int t = threadIdx.x; t < n_partials; t += TPB)
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] += partials[3 * (size_t)t + k];
  block_sum(v, red);
  if (threadIdx.x == 0)
#pragma unroll
    for (int k = 0; k < 3; ++k) terms[k] = (float)(v[k] / (double)n_f);
}

__global__ __launch_bounds__(TPB) void k_terms_stencil(int n_f, int n_v, const float *__restrict__ verts, const int32_t *__restrict__ faces,
                                                       const float *__restrict__ log_scales, const float *__restrict__ logit_opac,
                                                       const float *__restrict__ g, float *__restrict__ d_stencil,
                                                       float *__restrict__ d_log_scales, float *__restrict__ d_logit_opac) {
  const int64_t f = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (f >= n_f) return;
  trk::terms_backward(f, n_f, n_v, verts, faces, log_scales, logit_opac, g, d_stencil, d_log_scales, d_logit_opac);
}

__global__ __launch_bounds__(TPB) void k_vertex_normals(int n_v, const float *__restrict__ verts, const int32_t *__restrict__ faces,
                                                        const int32_t *__restrict__ start, const int32_t *__restrict__ items,
                                                        float *__restrict__ normals) {
  const int64_t v = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (v >= n_v) return;
  trk::vertex_normal(v, n_v, verts, faces, start, items, normals);
}

// Point i: the index k_nn_d2 left in best[i]; with nb, the signed distance and the workgroup's sum of the hinge in partials[blockIdx.x].
__global__ __launch_bounds__(TPB) void k_collision_rows(int n, int n_body, const float *__restrict__ va, const float *__restrict__ vb,
                                                        const float *__restrict__ nb, const unsigned long long *__restrict__ best, float eps,
                                                        int mode, int32_t *__restrict__ index, float *__restrict__ dist,
                                                        double *__restrict__ partials) {
  __shared__ double red[1][WAVES];
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  double v[1] = {0.0};
  if (i < n) {
    int32_t j = (int32_t)(unsigned)(best[i] & 0xffffffffull);
    if (j < 0 || j >= n_body) j = 0;  // k_nn_d2 writes indices of [0, n_body) only
    index[i] = j;
    if (nb) {
      const float d = trk::signed_distance(i, va, vb, nb, j);
      dist[i] = d;
      v[0] = (double)trk::penalty(d, eps, mode);
    }
  }
  if (!nb || mode == trk::MODE_DISTANCE) return;  // uniform over the grid
  block_sum(v, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = v[0];
}

__global__ __launch_bounds__(TPB) void k_collision_finish(int n, int n_partials, int mode, const double *__restrict__ partials,
                                                          float *__restrict__ value) {
  __shared__ double red[1][WAVES];
  double v[1] = {0.0};
  for (int t = threadIdx.x; t < n_partials; t += TPB) v[0] += partials[t];
  block_sum(v, red);
  if (threadIdx.x == 0) value[0] = (float)(mode == trk::MODE_AVERAGE ? v[0] / (double)n : v[0]);
}

__global__ __launch_bounds__(TPB) void k_collision_backward(int n, const float *__restrict__ nb, int n_body, const int32_t *__restrict__ index,
                                                            const float *__restrict__ dist, float eps, int mode, const float *__restrict__ g,
                                                            float *__restrict__ d_va) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  trk::collision_backward(i, n, nb, n_body, index, dist, eps, mode, g, d_va);
}

// what the face entry points require of the inputs they share; the 3 * n_faces corner items must stay an int32
bool mesh_ok(const float *verts, int32_t n_verts, const int32_t *faces, int32_t n_faces) {
  if (n_verts < 0 || n_faces < 0 || (int64_t)n_faces * 3 > INT32_MAX) return false;
  if (n_faces > 0 && (!verts || !faces)) return false;
  return true;
}

bool mode_ok(int32_t mode) { return mode == trk::MODE_DISTANCE || mode == trk::MODE_AVERAGE || mode == trk::MODE_CUBED; }

}  // namespace

extern "C" {

int mpmhip_track_render_vars(int32_t device, void *stream, const float *verts, int32_t n_verts, const int32_t *faces, int32_t n_faces,
                             const float *log_scales, const float *logit_opacities, float *out_means3D, float *out_rotations,
                             float *out_scales, float *out_opacities) {
  if (!mesh_ok(verts, n_verts, faces, n_faces)) return MPMHIP_ERR_INVALID;
  if (n_faces > 0 && (!log_scales || !logit_opacities || !out_means3D || !out_rotations || !out_scales || !out_opacities)) return MPMHIP_ERR_INVALID;
  if (int rc = device_in_range(device)) return rc;
  if (n_faces == 0) return MPMHIP_OK;
  ENTRY_CHECK(hipSetDevice(device));
  hipLaunchKernelGGL(k_render_vars, blocks(n_faces, TPB), TPB, 0, (hipStream_t)stream, n_faces, n_verts, verts, faces, log_scales,
                     logit_opacities, out_means3D, out_rotations, out_scales, out_opacities);
  return check(hipGetLastError());
}

int mpmhip_track_render_vars_backward(int32_t device, void *stream, const float *verts, int32_t n_verts, const int32_t *faces, int32_t n_faces,
                                      const float *log_scales, const float *logit_opacities, const float *g_means3D, const float *g_rotations,
                                      const float *g_scales, const float *g_opacities, const int32_t *vert_start, const int32_t *vert_items,
                                      float *d_stencil, float *d_verts, float *d_log_scales, float *d_logit_opacities) {
  if (!mesh_ok(verts, n_verts, faces, n_faces)) return MPMHIP_ERR_INVALID;
  if (n_faces > 0 && (!log_scales || !logit_opacities)) return MPMHIP_ERR_INVALID;
  if (d_verts && (!vert_start || (n_faces > 0 && (!vert_items || !d_stencil)))) return MPMHIP_ERR_INVALID;
  if (int rc = device_in_range(device)) return rc;
  if (!d_verts && !d_log_scales && !d_logit_opacities) return MPMHIP_OK;
  ENTRY_CHECK(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  if (n_faces > 0) {
    hipLaunchKernelGGL(k_render_stencil, blocks(n_faces, TPB), TPB, 0, s, n_faces, n_verts, verts, faces, log_scales, logit_opacities,
                       g_means3D, g_rotations, g_scales, g_opacities, d_verts ? d_stencil : nullptr, d_log_scales, d_logit_opacities);
    ENTRY_CHECK(hipGetLastError());
  }
  if (d_verts && n_verts > 0)
    hipLaunchKernelGGL(k_vertex_sum, blocks(n_verts, TPB), TPB, 0, s, n_verts, vert_start, vert_items, (const float *)d_stencil, d_verts);
  return check(hipGetLastError());
}

int mpmhip_track_face_geometry(int32_t device, void *stream, const float *verts, int32_t n_verts, const int32_t *faces, int32_t n_faces,
                               float *out_normals, float *out_areas) {
  if (!mesh_ok(verts, n_verts, faces, n_faces)) return MPMHIP_ERR_INVALID;
  if (int rc = device_in_range(device)) return rc;
  if (n_faces == 0 || (!out_normals && !out_areas)) return MPMHIP_OK;
  ENTRY_CHECK(hipSetDevice(device));
  hipLaunchKernelGGL(k_face_geometry, blocks(n_faces, TPB), TPB, 0, (hipStream_t)stream, n_faces, n_verts, verts, faces, out_normals, out_areas);
  return check(hipGetLastError());
}

int mpmhip_track_terms_forward(int32_t device, void *stream, const float *verts, int32_t n_verts, const int32_t *faces, int32_t n_faces,
                               const float *log_scales, const float *logit_opacities, double *scratch, float *out_terms) {
  if (!mesh_ok(verts, n_verts, faces, n_faces) || !scratch || !out_terms) return MPMHIP_ERR_INVALID;
  if (n_faces > 0 && (!log_scales || !logit_opacities)) return MPMHIP_ERR_INVALID;
  if (int rc = device_in_range(device)) return rc;
  if (n_faces == 0) return MPMHIP_OK;
  ENTRY_CHECK(hipSetDevice(device));
  const unsigned n_wg = blocks(n_faces, TPB);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_terms_rows, n_wg, TPB, 0, s, n_faces, n_verts, verts, faces, log_scales, logit_opacities, scratch);
  ENTRY_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_terms_finish, 1, TPB, 0, s, n_faces, (int)n_wg, (const double *)scratch, out_terms);
  return check(hipGetLastError());
}

int mpmhip_track_terms_backward(int32_t device, void *stream, const float *verts, int32_t n_verts, const int32_t *faces, int32_t n_faces,
                                const float *log_scales, const float *logit_opacities, const float *g_terms, const int32_t *vert_start,
                                const int32_t *vert_items, float *d_stencil, float *d_verts, float *d_log_scales, float *d_logit_opacities) {
  if (!mesh_ok(verts, n_verts, faces, n_faces) || !g_terms) return MPMHIP_ERR_INVALID;
  if (n_faces > 0 && (!log_scales || !logit_opacities)) return MPMHIP_ERR_INVALID;
  if (d_verts && (!vert_start || (n_faces > 0 && (!vert_items || !d_stencil)))) return MPMHIP_ERR_INVALID;
  if (int rc = device_in_range(device)) return rc;
  if (!d_verts && !d_log_scales && !d_logit_opacities) return MPMHIP_OK;
  ENTRY_CHECK(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  if (n_faces > 0) {
    hipLaunchKernelGGL(k_terms_stencil, blocks(n_faces, TPB), TPB, 0, s, n_faces, n_verts, verts, faces, log_scales, logit_opacities, g_terms,
                       d_verts ? d_stencil : nullptr, d_log_scales, d_logit_opacities);
    ENTRY_CHECK(hipGetLastError());
  }
  if (d_verts && n_verts > 0)
    hipLaunchKernelGGL(k_vertex_sum, blocks(n_verts, TPB), TPB, 0, s, n_verts, vert_start, vert_items, (const float *)d_stencil, d_verts);
  return check(hipGetLastError());
}

int mpmhip_track_vertex_normals(int32_t device, void *stream, const float *verts, int32_t n_verts, const int32_t *faces, int32_t n_faces,
                                const int32_t *vert_start, const int32_t *vert_items, float *out_normals) {
  if (!mesh_ok(verts, n_verts, faces, n_faces) || !vert_start || !out_normals) return MPMHIP_ERR_INVALID;
  if (n_verts > 0 && !verts) return MPMHIP_ERR_INVALID;
  if (n_faces > 0 && !vert_items) return MPMHIP_ERR_INVALID;
  if (int rc = device_in_range(device)) return rc;
  if (n_verts == 0) return MPMHIP_OK;
  ENTRY_CHECK(hipSetDevice(device));
  hipLaunchKernelGGL(k_vertex_normals, blocks(n_verts, TPB), TPB, 0, (hipStream_t)stream, n_verts, verts, faces, vert_start, vert_items,
                     out_normals);
  return check(hipGetLastError());
}

int mpmhip_track_collision_forward(int32_t device, void *stream, const float *va, int32_t n, const float *vb, const float *nb, int32_t n_body,
                                   float eps, int32_t mode, uint64_t *best_scratch, double *scratch, int32_t *out_index, float *out_distance,
                                   float *out_value) {
  if (n < 0 || n_body <= 0 || !vb || !mode_ok(mode)) return MPMHIP_ERR_INVALID;
  if (n > 0 && (!va || !best_scratch || !out_index)) return MPMHIP_ERR_INVALID;
  if (nb && n > 0 && !out_distance) return MPMHIP_ERR_INVALID;
  const bool reduce = nb && mode != trk::MODE_DISTANCE;
  if (reduce && (!scratch || !out_value)) return MPMHIP_ERR_INVALID;
  if (int rc = device_in_range(device)) return rc;
  if (n == 0) return MPMHIP_OK;
  ENTRY_CHECK(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  if (int rc = nn::launch_nearest(s, va, n, vb, n_body, 0, best_scratch)) return rc;
  const unsigned n_wg = blocks(n, TPB);
  hipLaunchKernelGGL(k_collision_rows, n_wg, TPB, 0, s, n, n_body, va, vb, nb, (const unsigned long long *)best_scratch, eps, (int)mode,
                     out_index, out_distance, scratch);
  ENTRY_CHECK(hipGetLastError());
  if (reduce) hipLaunchKernelGGL(k_collision_finish, 1, TPB, 0, s, n, (int)n_wg, (int)mode, (const double *)scratch, out_value);
  return check(hipGetLastError());
}

int mpmhip_track_collision_backward(int32_t device, void *stream, int32_t n, const float *nb, int32_t n_body, const int32_t *index,
                                    const float *distance, float eps, int32_t mode, const float *g, float *d_va) {
  if (n < 0 || n_body <= 0 || !nb || !mode_ok(mode) || !g) return MPMHIP_ERR_INVALID;
  if (n > 0 && (!index || !distance)) return MPMHIP_ERR_INVALID;
  if (int rc = device_in_range(device)) return rc;
  if (n == 0 || !d_va) return MPMHIP_OK;
  ENTRY_CHECK(hipSetDevice(device));
  hipLaunchKernelGGL(k_collision_backward, blocks(n, TPB), TPB, 0, (hipStream_t)stream, n, nb, n_body, index, distance, eps, (int)mode, g, d_va);
  return check(hipGetLastError());
}

}  // extern "C"
