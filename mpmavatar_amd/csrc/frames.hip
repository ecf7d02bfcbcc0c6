// frames.hip -- the step right after the solver in the reference's render loop: simulated vertices
// -> per-face frames (MeshGaussianModel.set_mesh_by_verts, /root/reference/scene/mesh_gaussian_model.py:137-146 with
// compute_face_orientation, utils/graphics_utils.py:88-106) -> position / rotation / scale of the Gaussians bound to the
// faces (GaussianModel.get_xyz / get_rotation / get_scaling, scene/gaussian_model.py:112-151).  Pure per-face and
// per-Gaussian maps, HBM-bound: 24 B of indices + gathered vertices in, 68 B out per face; 36 B in + 32 B of gathered
// frame, 44 B out per Gaussian.  Keeps the simulated vertices on the device instead of the reference's
// OBJ -> disk -> Blender -> reload detour for everything but the AO map.
// k_face_frames is one thread per item over frames_math.hpp (shared with the backward and the host build).  The bodies of
// k_bind_gaussians, k_render_inputs and k_cov_from_F are NOT in that header yet, on purpose: their outputs feed every golden
// comparison downstream, and the instructions the compiler emits for them follow the shape of the source, not only its expression
// trees.  Tried, each compared against this file's device listing: the two per-Gaussian bodies as one shared row function
// (rotations moved by up to 65536 ulp on random unit-scale inputs, means and scales stayed bitwise equal), the bodies moved
// verbatim into inline functions (listing differs in scheduling and address code), and the Hamilton product alone as a shared
// function (listing differs).  Only the vector type and the clamp constant are shared here; that leaves the listing identical.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "entry.hpp"
#include "frames_math.hpp"

namespace {

using namespace entry;
constexpr int TPB = 256;

using frm::V3;
using frm::ld3;

__global__ void k_face_frames(const float *verts, const int32_t *faces, int n_f, float *center, float *mat, float *quat,
                              float *scale) {
  int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_f) return;
  frm::face_frame_row(f, verts, faces, center, mat, quat, scale);
}

// torch.nn.functional.normalize(q, dim=-1): q / max(|q|, 1e-12)
__device__ __forceinline__ void normalize4(float q[4]) {
  float n = fmaxf(sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]), frm::NORM_EPS);
  for (int k = 0; k < 4; ++k) q[k] = q[k] / n;
}

__global__ void k_bind_gaussians(int n_g, const int32_t *binding, const float *xyz_local, const float *rot_raw,
                                 const float *scaling_raw, const float *center, const float *mat, const float *quat,
                                 const float *fscale, float *xyz, float *rot, float *scaling) {
  int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_g) return;
  int f = binding[g];
  float s = fscale[f];
  if (xyz) {  // bmm(face_orien_mat[binding], _xyz) * face_scaling + face_center, gaussian_model.py:149-150
    const float *m = mat + 9 * (size_t)f;
    V3 p = ld3(xyz_local, g), c = ld3(center, f);
    xyz[3 * (size_t)g] = (m[0] * p.x + m[1] * p.y + m[2] * p.z) * s + c.x;
    xyz[3 * (size_t)g + 1] = (m[3] * p.x + m[4] * p.y + m[5] * p.z) * s + c.y;
    xyz[3 * (size_t)g + 2] = (m[6] * p.x + m[7] * p.y + m[8] * p.z) * s + c.z;
  }
  if (rot) {  // quat_product(normalize(face quat), normalize(_rotation)), WXYZ in and out, :133-136
    float a[4], b[4];
    for (int k = 0; k < 4; ++k) { a[k] = quat[4 * (size_t)f + k]; b[k] = rot_raw[4 * (size_t)g + k]; }
    normalize4(a);
    normalize4(b);
    float pw = a[0], px = a[1], py = a[2], pz = a[3], qw = b[0], qx = b[1], qy = b[2], qz = b[3];
    float *o = rot + 4 * (size_t)g;
    o[0] = pw * qw - px * qx - py * qy - pz * qz;
    o[1] = pw * qx + px * qw + py * qz - pz * qy;
    o[2] = pw * qy - px * qz + py * qw + pz * qx;
    o[3] = pw * qz + px * qy - py * qx + pz * qw;
  }
  if (scaling)  // exp(_scaling) * face_scaling[binding], :121-122
    for (int k = 0; k < 3; ++k) scaling[3 * (size_t)g + k] = expf(scaling_raw[3 * (size_t)g + k]) * s;
}

// The argument lists of the rasteriser call (gaussian_renderer/__init__.py:52-103), assembled in ONE launch: rows [0, n_g) are the
// mesh-bound Gaussians -- means3D = get_xyz, rotations = get_rotation, scales = get_scaling (as k_bind_gaussians), opacities =
// sigmoid(_opacity) (gaussian_model.py:39,158-160) -- rows [n_g, n_g + n_x) the caller's `extra` primitives copied behind them
// (:84-91: the five torch.cat of the render call); means2D (zeros, :27) is cleared here too.
__global__ void k_render_inputs(int n_g, int n_x, const int32_t *binding, const float *xyz_local, const float *rot_raw,
                                const float *scaling_raw, const float *opacity_raw, const float *center, const float *mat,
                                const float *quat, const float *fscale, const float *x_xyz, const float *x_opacity,
                                const float *x_scales, const float *x_rot, float *means3D, float *means2D, float *opacities,
                                float *scales, float *rotations) {
  int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_g + n_x) return;
  for (int k = 0; k < 3; ++k) means2D[3 * (size_t)g + k] = 0.0f;
  if (g >= n_g) {
    int e = g - n_g;
    for (int k = 0; k < 3; ++k) { means3D[3 * (size_t)g + k] = x_xyz[3 * (size_t)e + k]; scales[3 * (size_t)g + k] = x_scales[3 * (size_t)e + k]; }
    for (int k = 0; k < 4; ++k) rotations[4 * (size_t)g + k] = x_rot[4 * (size_t)e + k];
    opacities[g] = x_opacity[e];
    return;
  }
  int f = binding[g];
  float s = fscale[f];
  const float *m = mat + 9 * (size_t)f;
  V3 p = ld3(xyz_local, g), c = ld3(center, f);
  means3D[3 * (size_t)g] = (m[0] * p.x + m[1] * p.y + m[2] * p.z) * s + c.x;
  means3D[3 * (size_t)g + 1] = (m[3] * p.x + m[4] * p.y + m[5] * p.z) * s + c.y;
  means3D[3 * (size_t)g + 2] = (m[6] * p.x + m[7] * p.y + m[8] * p.z) * s + c.z;
  float a[4], b[4];
  for (int k = 0; k < 4; ++k) { a[k] = quat[4 * (size_t)f + k]; b[k] = rot_raw[4 * (size_t)g + k]; }
  normalize4(a);
  normalize4(b);
  float pw = a[0], px = a[1], py = a[2], pz = a[3], qw = b[0], qx = b[1], qy = b[2], qz = b[3];
  float *o = rotations + 4 * (size_t)g;
  o[0] = pw * qw - px * qx - py * qy - pz * qz;
  o[1] = pw * qx + px * qw + py * qz - pz * qy;
  o[2] = pw * qy - px * qz + py * qw + pz * qx;
  o[3] = pw * qz + px * qy - py * qx + pz * qw;
  for (int k = 0; k < 3; ++k) scales[3 * (size_t)g + k] = expf(scaling_raw[3 * (size_t)g + k]) * s;
  opacities[g] = 1.0f / (1.0f + expf(-opacity_raw[g]));  // torch.sigmoid
}

// compute_cov_from_F (/root/reference/warp_mpm/mpm_utils.py:1108-1132): cov = F_trial * sym(cov0) * F_trial^T per
// particle, upper triangle out (xx, xy, xz, yy, yz, zz).  Products summed left to right as Warp's mat33 product does.
__global__ void k_cov_from_F(const float *F_trial, const float *cov0, int n, float *out) {
  int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  float F[3][3], S[3][3], T[3][3];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) F[r][c] = F_trial[9 * (size_t)p + 3 * r + c];
  const float *q = cov0 + 6 * (size_t)p;
  S[0][0] = q[0]; S[0][1] = q[1]; S[0][2] = q[2];
  S[1][0] = q[1]; S[1][1] = q[3]; S[1][2] = q[4];
  S[2][0] = q[2]; S[2][1] = q[4]; S[2][2] = q[5];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) T[r][c] = F[r][0] * S[0][c] + F[r][1] * S[1][c] + F[r][2] * S[2][c];
  float *o = out + 6 * (size_t)p;
  int k = 0;
  for (int r = 0; r < 3; ++r)
    for (int c = r; c < 3; ++c) o[k++] = T[r][0] * F[c][0] + T[r][1] * F[c][1] + T[r][2] * F[c][2];
}

}  // namespace

extern "C" {

int mpmhip_cov_from_F(int32_t device, void *stream, const float *particle_F_trial, const float *particle_cov, int32_t n,
                      float *new_cov) {
  if (n < 0 || (n > 0 && (!particle_F_trial || !particle_cov || !new_cov))) return MPMHIP_ERR_INVALID;
  if (int rc = device_in_range(device)) return rc;
  if (n == 0) return MPMHIP_OK;
  ENTRY_CHECK(hipSetDevice(device));
  hipLaunchKernelGGL(k_cov_from_F, blocks(n, TPB), TPB, 0, (hipStream_t)stream, particle_F_trial, particle_cov, n,
                     new_cov);
  return check(hipGetLastError());
}

int mpmhip_face_frames(int32_t device, void *stream, const float *verts, const int32_t *faces, int32_t n_faces,
                       float *face_center, float *face_orien_mat, float *face_orien_quat, float *face_scaling) {
  if (n_faces < 0 || (n_faces > 0 && (!verts || !faces || !face_center || !face_orien_mat || !face_orien_quat || !face_scaling)))
    return MPMHIP_ERR_INVALID;
  if (int rc = device_in_range(device)) return rc;
  if (n_faces == 0) return MPMHIP_OK;
  ENTRY_CHECK(hipSetDevice(device));
  hipLaunchKernelGGL(k_face_frames, blocks(n_faces, TPB), TPB, 0, (hipStream_t)stream, verts, faces, n_faces,
                     face_center, face_orien_mat, face_orien_quat, face_scaling);
  return check(hipGetLastError());
}

int mpmhip_bind_gaussians(int32_t device, void *stream, int32_t n_gaussians, const int32_t *binding, const float *xyz_local,
                          const float *rotation_raw, const float *scaling_raw, const float *face_center,
                          const float *face_orien_mat, const float *face_orien_quat, const float *face_scaling, float *xyz,
                          float *rotation, float *scaling) {
  if (n_gaussians < 0) return MPMHIP_ERR_INVALID;
  if (n_gaussians > 0 && (!binding || !face_scaling || (xyz && (!xyz_local || !face_center || !face_orien_mat)) ||
                          (rotation && (!rotation_raw || !face_orien_quat)) || (scaling && !scaling_raw)))
    return MPMHIP_ERR_INVALID;
  if (int rc = device_in_range(device)) return rc;
  if (n_gaussians == 0) return MPMHIP_OK;
  ENTRY_CHECK(hipSetDevice(device));
  hipLaunchKernelGGL(k_bind_gaussians, blocks(n_gaussians, TPB), TPB, 0, (hipStream_t)stream, n_gaussians,
                     binding, xyz_local, rotation_raw, scaling_raw, face_center, face_orien_mat, face_orien_quat,
                     face_scaling, xyz, rotation, scaling);
  return check(hipGetLastError());
}

int mpmhip_render_inputs(int32_t device, void *stream, int32_t n_gaussians, int32_t n_extra, const int32_t *binding,
                         const float *xyz_local, const float *rotation_raw, const float *scaling_raw, const float *opacity_raw,
                         const float *face_center, const float *face_orien_mat, const float *face_orien_quat,
                         const float *face_scaling, const float *extra_xyz, const float *extra_opacity, const float *extra_scales,
                         const float *extra_rotations, float *means3D, float *means2D, float *opacities, float *scales,
                         float *rotations) {
  if (n_gaussians < 0 || n_extra < 0) return MPMHIP_ERR_INVALID;
  if (n_gaussians + n_extra > 0 && (!means3D || !means2D || !opacities || !scales || !rotations)) return MPMHIP_ERR_INVALID;
  if (n_gaussians > 0 && (!binding || !xyz_local || !rotation_raw || !scaling_raw || !opacity_raw || !face_center || !face_orien_mat ||
                          !face_orien_quat || !face_scaling))
    return MPMHIP_ERR_INVALID;
  if (n_extra > 0 && (!extra_xyz || !extra_opacity || !extra_scales || !extra_rotations)) return MPMHIP_ERR_INVALID;
  if (int rc = device_in_range(device)) return rc;
  if (n_gaussians + n_extra == 0) return MPMHIP_OK;
  ENTRY_CHECK(hipSetDevice(device));
  hipLaunchKernelGGL(k_render_inputs, blocks(n_gaussians + n_extra, TPB), TPB, 0, (hipStream_t)stream, n_gaussians,
                     n_extra, binding, xyz_local, rotation_raw, scaling_raw, opacity_raw, face_center, face_orien_mat, face_orien_quat,
                     face_scaling, extra_xyz, extra_opacity, extra_scales, extra_rotations, means3D, means2D, opacities, scales,
                     rotations);
  return check(hipGetLastError());
}

}  // extern "C"
