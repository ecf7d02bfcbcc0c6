// frames_math.hpp -- the per-face frames of the mesh binding (k_face_frames of frames.hip), per work item, and the 3-vector the
// appearance chain's mesh stages share (frames_grad_math.hpp, reg_math.hpp, track_math.hpp).  The reference: compute_face_orientation
// (utils/graphics_utils.py:82-106) under MeshGaussianModel.set_mesh_by_verts (scene/mesh_gaussian_model.py:137-146).
// Plain C++ for the device (frames.hip, frames_backward.hip) and the host (tests/hostframes/) alike: one function per work item, so
// the kernels and the host loops are the same statements.  The backward (frames_grad_math.hpp) takes the forward's values from
// face_chain, quat_branch, quat_numerators, norm4 and normalize4 here.  All arithmetic is fp32.
//
// The device code of k_face_frames follows the SHAPE of this source, not only its expression trees.  With rotmat_to_quat_xyzw split
// into quat_branch + quat_numerators + norm4 (in any of: two functions, one function returning the branch, one function with the
// numerators and the norm as extra outputs, the division moved to the caller) the vectoriser pairs the chain's products differently
// and the back end fuses other products into the sums: 98 fused multiply-adds instead of 96, 45 multiplies instead of 48 in the
// kernel's listing.  A build of that shape against the build of the previous source, on an MI355X, same inputs: face_orien_mat
// differed by up to 202 ulp and face_orien_quat by up to 40 ulp on tests/golden/binding_grad.npz (34 and 181 ulp on
// render_inputs.npz), the scale by 1-2 ulp.  Those outputs feed every golden comparison downstream, so face_frame_row keeps the
// map in one piece -- with it the kernel's listing is instruction for instruction the previous one -- and quat_branch /
// quat_numerators state the same rule a second time for the backward, which reads the branch off the SAVED matrix and the unit
// quaternion from the saved one.  tests/test_frames_host.py holds the two statements to the same bits without contraction; on the
// device the backward's figures are bitwise those of the previous build (same comparison, a million random faces).
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

namespace frm {

struct V3 {
  float x, y, z;
};

__host__ __device__ __forceinline__ V3 ld3(const float *p, int64_t i) { return V3{p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }
__host__ __device__ __forceinline__ void st3(float *p, int64_t i, V3 v) { p[3 * i] = v.x; p[3 * i + 1] = v.y; p[3 * i + 2] = v.z; }
__host__ __device__ __forceinline__ V3 add(V3 a, V3 b) { return V3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__host__ __device__ __forceinline__ V3 sub(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__host__ __device__ __forceinline__ V3 mul(V3 a, float s) { return V3{a.x * s, a.y * s, a.z * s}; }
__host__ __device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__host__ __device__ __forceinline__ V3 cross(V3 a, V3 b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
// the same functions spelt as operators (reg_math.hpp); s * a and a * s are the same bits
__host__ __device__ __forceinline__ V3 operator+(V3 a, V3 b) { return add(a, b); }
__host__ __device__ __forceinline__ V3 operator-(V3 a, V3 b) { return sub(a, b); }
__host__ __device__ __forceinline__ V3 operator*(float s, V3 a) { return V3{s * a.x, s * a.y, s * a.z}; }
__host__ __device__ __forceinline__ float sign(float x) { return (float)(x > 0.f) - (float)(x < 0.f); }

constexpr float LEN_EPS = 1e-20f;   // graphics_utils.py:82-86, length(): sqrt(clamp(dot(x, x), min = 1e-20))
constexpr float NORM_EPS = 1e-12f;  // torch.nn.functional.normalize: x / max(|x|, 1e-12)

__host__ __device__ __forceinline__ float length(V3 a) { return sqrtf(fmaxf(dot(a, a), LEN_EPS)); }

// e1, e2 -> a0 = e1 / |e1| -> c1 = a0 x e2, a1 = c1 / |c1| -> c2 = a1 x a0, a2 = -(c2 / |c2|), with the three clamped lengths
struct FaceChain {
  V3 e1, e2, a0, c1, a1, c2, a2;
  float l1, lc1, lc2;
};

__host__ __device__ __forceinline__ FaceChain face_chain(V3 v0, V3 v1, V3 v2) {
  FaceChain t;
  t.e1 = sub(v1, v0);
  t.e2 = sub(v2, v0);
  t.l1 = length(t.e1);
  t.a0 = V3{t.e1.x / t.l1, t.e1.y / t.l1, t.e1.z / t.l1};
  t.c1 = cross(t.a0, t.e2);
  t.lc1 = length(t.c1);
  t.a1 = V3{t.c1.x / t.lc1, t.c1.y / t.lc1, t.c1.z / t.lc1};
  t.c2 = cross(t.a1, t.a0);
  t.lc2 = length(t.c2);
  t.a2 = V3{-(t.c2.x / t.lc2), -(t.c2.y / t.lc2), -(t.c2.z / t.lc2)};  // "will have artifacts without negation", graphics_utils.py:99
  return t;
}

// roma.rotmat_to_unitquat (= SciPy's Rotation.from_matrix): XYZW, the largest of (R00, R11, R22, trace) picks the
// branch (first maximum wins, like argmax), no sign canonicalisation
__host__ __device__ __forceinline__ void rotmat_to_quat_xyzw(const float R[3][3], float q[4]) {
  float d[4] = {R[0][0], R[1][1], R[2][2], 0.0f};
  d[3] = d[0] + d[1] + d[2];
  int c = 0;
  for (int k = 1; k < 4; ++k)
    if (d[k] > d[c]) c = k;
  if (c != 3) {
    int i = c, j = (i + 1) % 3, k = (j + 1) % 3;
    q[i] = 1.0f - d[3] + 2.0f * R[i][i];
    q[j] = R[j][i] + R[i][j];
    q[k] = R[k][i] + R[i][k];
    q[3] = R[k][j] - R[j][k];
  } else {
    q[0] = R[2][1] - R[1][2];
    q[1] = R[0][2] - R[2][0];
    q[2] = R[1][0] - R[0][1];
    q[3] = 1.0f + d[3];
  }
  float n = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int k = 0; k < 4; ++k) q[k] = q[k] / n;
}

// The same map in the pieces the backward needs.  The branch:
__host__ __device__ __forceinline__ int quat_branch(const float R[3][3]) {
  const float d[4] = {R[0][0], R[1][1], R[2][2], R[0][0] + R[1][1] + R[2][2]};
  int b = 0;
  for (int k = 1; k < 4; ++k)
    if (d[k] > d[b]) b = k;
  return b;
}

// the four XYZW numerators of branch b, before the division by their norm
__host__ __device__ __forceinline__ void quat_numerators(const float R[3][3], int b, float q[4]) {
  const float trace = R[0][0] + R[1][1] + R[2][2];
  if (b != 3) {
    const int i = b, j = (i + 1) % 3, k = (j + 1) % 3;
    q[i] = 1.0f - trace + 2.0f * R[i][i];
    q[j] = R[j][i] + R[i][j];
    q[k] = R[k][i] + R[i][k];
    q[3] = R[k][j] - R[j][k];
  } else {
    q[0] = R[2][1] - R[1][2];
    q[1] = R[0][2] - R[2][0];
    q[2] = R[1][0] - R[0][1];
    q[3] = 1.0f + trace;
  }
}

__host__ __device__ __forceinline__ float norm4(const float q[4]) { return sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]); }

// u = q / n, n = max(|q|, 1e-12) (torch.nn.functional.normalize); bound: the clamp binds
__host__ __device__ __forceinline__ void normalize4(const float q[4], float u[4], float &n, bool &bound) {
  const float len = norm4(q);
  bound = len < NORM_EPS;
  n = fmaxf(len, NORM_EPS);
  for (int k = 0; k < 4; ++k) u[k] = q[k] / n;
}

// Row f of face_center [F, 3], face_orien_mat [F, 3, 3] (columns a0 a1 a2), face_orien_quat [F, 4] (WXYZ, quat_xyzw_to_wxyz) and
// face_scaling [F].
__host__ __device__ __forceinline__ void face_frame_row(int64_t f, const float *verts, const int32_t *faces, float *center, float *mat,
                                                        float *quat, float *scale) {
  int i0 = faces[3 * (size_t)f], i1 = faces[3 * (size_t)f + 1], i2 = faces[3 * (size_t)f + 2];
  V3 v0 = ld3(verts, i0), v1 = ld3(verts, i1), v2 = ld3(verts, i2);
  // triangles.mean(dim=-2): ((v0 + v1) + v2) / 3
  center[3 * (size_t)f] = ((v0.x + v1.x) + v2.x) / 3.0f;
  center[3 * (size_t)f + 1] = ((v0.y + v1.y) + v2.y) / 3.0f;
  center[3 * (size_t)f + 2] = ((v0.z + v1.z) + v2.z) / 3.0f;
  const FaceChain t = face_chain(v0, v1, v2);
  float R[3][3] = {{t.a0.x, t.a1.x, t.a2.x}, {t.a0.y, t.a1.y, t.a2.y}, {t.a0.z, t.a1.z, t.a2.z}};
  float *m = mat + 9 * (size_t)f;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) m[3 * r + c] = R[r][c];
  scale[f] = (t.l1 + fabsf(dot(t.a2, t.e2))) / 2.0f;
  float q[4];
  rotmat_to_quat_xyzw(R, q);
  float *o = quat + 4 * (size_t)f;
  o[0] = q[3]; o[1] = q[0]; o[2] = q[1]; o[3] = q[2];
}

}  // namespace frm
