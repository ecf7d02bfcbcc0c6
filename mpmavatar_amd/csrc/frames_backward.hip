// frames_backward.hip -- gradients through frames.hip: from the rasteriser's arguments back to the raw Gaussian parameters and the
// face frames (mpmhip_render_inputs_backward), and from the face frames back to the vertices (mpmhip_face_frames_backward).  The
// math is frames_grad_math.hpp; the kernels here are one thread per item over it.  HBM-bound rows, no LDS.  Per Gaussian: 36 B of
// parameters + 44 B of upstream + 56 B of gathered frame in, 44 B out.  Per face: its Gaussians' 44 B of index and parameters + 40 B of
// upstream each (gathered through the face -> Gaussian table) in, 68 B out.  Per face (frames): 12 B of indices + 36 B of gathered
// vertices + 52 B of saved frame + 68 B of upstream in, 36 B out.  Per vertex: 12 B per incident corner in, 12 B out.
// No floating-point atomics: the two reductions (Gaussians of a face, corners of a vertex) are serial walks of a CSR segment
// in ascending index, so two runs give the same bits.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "entry.hpp"
#include "frames_grad_math.hpp"

namespace {

using namespace entry;
constexpr int TPB = 256;

__global__ void k_gaussian_backward(int n_g, const int32_t *binding, const float *rot_raw, const float *scaling_raw,
                                    const float *opacity_raw, const float *mat, const float *quat, const float *fscale,
                                    const float *g_mean, const float *g_rot, const float *g_scale, const float *g_opac, float *d_xyz,
                                    float *d_rot, float *d_scaling, float *d_opacity) {
  int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_g) return;
  fgrad::gaussian_backward(g, binding, rot_raw, scaling_raw, opacity_raw, mat, quat, fscale, g_mean, g_rot, g_scale, g_opac, d_xyz, d_rot,
                           d_scaling, d_opacity);
}

__global__ void k_face_accumulate(int n_f, const int32_t *start, const int32_t *items, const float *xyz_local, const float *rot_raw,
                                  const float *scaling_raw, const float *mat, const float *quat, const float *fscale, const float *g_mean,
                                  const float *g_rot, const float *g_scale, float *d_center, float *d_mat, float *d_quat, float *d_fscale) {
  int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_f) return;
  fgrad::face_accumulate(f, start, items, xyz_local, rot_raw, scaling_raw, mat, quat, fscale, g_mean, g_rot, g_scale, d_center, d_mat, d_quat,
                         d_fscale);
}

__global__ void k_face_frames_backward(int n_f, const float *verts, const int32_t *faces, const float *mat, const float *quat,
                                       const float *g_center, const float *g_mat, const float *g_quat, const float *g_fscale,
                                       float *d_corner) {
  int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_f) return;
  fgrad::face_frames_backward(f, verts, faces, mat, quat, g_center, g_mat, g_quat, g_fscale, d_corner);
}

__global__ void k_vertex_gather(int n_v, const int32_t *start, const int32_t *corners, const float *d_corner, float *d_verts) {
  int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n_v) return;
  fgrad::vertex_gather(v, start, corners, d_corner, d_verts);
}

}  // namespace

extern "C" {

int mpmhip_render_inputs_backward(int32_t device, void *stream, int32_t n_gaussians, int32_t n_faces, const int32_t *binding,
                                  const float *xyz_local, const float *rotation_raw, const float *scaling_raw, const float *opacity_raw,
                                  const float *face_orien_mat, const float *face_orien_quat, const float *face_scaling,
                                  const float *g_means3D, const float *g_opacities, const float *g_scales, const float *g_rotations,
                                  float *d_xyz, float *d_rotation, float *d_scaling, float *d_opacity, const int32_t *face_start,
                                  const int32_t *face_items, float *d_face_center, float *d_face_orien_mat, float *d_face_orien_quat,
                                  float *d_face_scaling) {
  if (n_gaussians < 0 || n_faces < 0) return MPMHIP_ERR_INVALID;
  const bool params = d_xyz || d_rotation || d_scaling || d_opacity;
  const bool any_face = d_face_center || d_face_orien_mat || d_face_orien_quat || d_face_scaling;
  const bool all_face = d_face_center && d_face_orien_mat && d_face_orien_quat && d_face_scaling;
  if (any_face && !all_face) return MPMHIP_ERR_INVALID;  // the four frame gradients come from one walk: all or none
  if (n_faces > 0 && all_face && (!face_start || (n_gaussians > 0 && !face_items))) return MPMHIP_ERR_INVALID;
  if (n_gaussians > 0 && (params || all_face)) {
    if (!binding || !face_scaling) return MPMHIP_ERR_INVALID;
    if (g_means3D && (!face_orien_mat || (all_face && !xyz_local))) return MPMHIP_ERR_INVALID;
    if (g_rotations && (!rotation_raw || !face_orien_quat)) return MPMHIP_ERR_INVALID;
    if (g_scales && !scaling_raw) return MPMHIP_ERR_INVALID;
    if (g_opacities && d_opacity && !opacity_raw) return MPMHIP_ERR_INVALID;
  }
  if (int rc = device_in_range(device)) return rc;
  const bool run1 = params && n_gaussians > 0, run2 = all_face && n_faces > 0;
  if (!run1 && !run2) return MPMHIP_OK;
  ENTRY_CHECK(hipSetDevice(device));
  if (run1) {
    hipLaunchKernelGGL(k_gaussian_backward, blocks(n_gaussians, TPB), TPB, 0, (hipStream_t)stream, n_gaussians, binding, rotation_raw,
                       scaling_raw, opacity_raw, face_orien_mat, face_orien_quat, face_scaling, g_means3D, g_rotations, g_scales,
                       g_opacities, d_xyz, d_rotation, d_scaling, d_opacity);
    ENTRY_CHECK(hipGetLastError());
  }
  if (run2) {
    hipLaunchKernelGGL(k_face_accumulate, blocks(n_faces, TPB), TPB, 0, (hipStream_t)stream, n_faces, face_start, face_items, xyz_local,
                       rotation_raw, scaling_raw, face_orien_mat, face_orien_quat, face_scaling, g_means3D, g_rotations, g_scales,
                       d_face_center, d_face_orien_mat, d_face_orien_quat, d_face_scaling);
    ENTRY_CHECK(hipGetLastError());
  }
  return MPMHIP_OK;
}

int mpmhip_face_frames_backward(int32_t device, void *stream, const float *verts, const int32_t *faces, int32_t n_faces, int32_t n_verts,
                                const float *face_orien_mat, const float *face_orien_quat, const float *g_face_center,
                                const float *g_face_orien_mat, const float *g_face_orien_quat, const float *g_face_scaling,
                                const int32_t *vert_start, const int32_t *vert_corners, float *d_corners, float *d_verts) {
  if (n_faces < 0 || n_verts < 0) return MPMHIP_ERR_INVALID;
  if (n_faces > 0 && (!verts || !faces || !face_orien_mat || !face_orien_quat || !d_corners || !vert_corners)) return MPMHIP_ERR_INVALID;
  if (n_verts > 0 && (!vert_start || !d_verts)) return MPMHIP_ERR_INVALID;
  if (int rc = device_in_range(device)) return rc;
  if (n_verts == 0) return MPMHIP_OK;
  ENTRY_CHECK(hipSetDevice(device));
  if (n_faces > 0) {
    hipLaunchKernelGGL(k_face_frames_backward, blocks(n_faces, TPB), TPB, 0, (hipStream_t)stream, n_faces, verts, faces, face_orien_mat,
                       face_orien_quat, g_face_center, g_face_orien_mat, g_face_orien_quat, g_face_scaling, d_corners);
    ENTRY_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_vertex_gather, blocks(n_verts, TPB), TPB, 0, (hipStream_t)stream, n_verts, vert_start, vert_corners, d_corners, d_verts);
  return check(hipGetLastError());
}

}  // extern "C"
