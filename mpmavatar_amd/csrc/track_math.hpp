// track_math.hpp -- the mesh tracking step (preprocess/train_mesh_lbs_actorshq.py:209-279), per work item:
//   params2rendervar (:209-225), one Gaussian per face with v1, v2, v3 = vertices[faces[f]]
//     means3D = (v1 + v2 + v3) / 3                                              compute_face_barycenters (utils/geo_utils.py:32-38)
//     rotations = quaternion WXYZ of the matrix with columns x, y, z             compute_q_from_faces (:40-75)
//       e1 = v2 - v1, e2 = v3 - v2, e3 = v1 - v3;  x = the longest / its length (the first of the longest, as torch.max)
//       z = fn / |fn|, fn = n / |n|, n = e1 x e2 (compute_face_normals :21-30, normalised twice);  y = z x x, normalised
//     scales = exp(log_scales), opacities = sigmoid(logit_opacities)
//   losses (:242, :254, :263-268)
//     area = mean_f | |n| / 2 - pi s0 s1 |,  scale = mean_f s2,  opacity = mean_f (1 - sigmoid(logit_opacities))
//   compute_vertex_normals (utils/geo_utils.py:8-19): the sum over a vertex's faces of (v0 - v1) x (v2 - v1), normalised
//   collision_penalty (preprocess/losses/physics.py:6-20): d = -nb[j] . (va - vb[j]) with j the nearest body vertex, pen = max(eps - d, 0)
// and the exact derivative of those expressions with every discrete decision held fixed: the longest edge, the quaternion's branch
// and sign, sign(0) = 0 inside abs, and the hinge (slope 1 / 0, exactly 1/2 where eps - d == 0, as torch.maximum).
//
// The matrix -> quaternion map is this project's restatement of pytorch3d.transforms.matrix_to_quaternion (UNCONFIRMED against
// pytorch3d itself, which is not installed where the fixtures are made): the four roots r_k = sqrt(max(0, 1 +- m00 +- m11 +- m22)),
// the four candidate rows divided by 2 max(r_k, 0.1), the row of the largest root, then the sign that makes w >= 0.  The roots'
// squares sum to 4, so the largest is at least 1: the floor of 0.1 and the clamp at 0 never bind on the row that is taken, and the
// backward has no case for them.  q and -q are the same rotation.
//
// Plain C++ for the device (track.hip) and the host (tests/hosttrack/) alike: one function per work item.  All arithmetic is fp32;
// the sums over faces and points are the caller's (double, fixed order).  A zero-area face gives NaN, as in the reference; an index
// outside its range reads nothing and gives NaN.
#pragma once
#include "frames_grad_math.hpp"

#include <math.h>
#include <stdint.h>

namespace trk {

using frm::V3;
using frm::add;
using frm::cross;
using frm::dot;
using frm::ld3;
using frm::mul;
using frm::sign;
using frm::st3;
using frm::sub;

constexpr float PI_F = 3.14159265358979323846f;
constexpr int MODE_DISTANCE = 0, MODE_AVERAGE = 1, MODE_CUBED = 2;  // collision_penalty's three returns

__host__ __device__ __forceinline__ float sigmoid(float x) { return 1.f / (1.f + expf(-x)); }
__host__ __device__ __forceinline__ V3 nan3() { return V3{NAN, NAN, NAN}; }

// the three corners of face f; false (and NaN corners) where an index is outside [0, n_verts)
__host__ __device__ __forceinline__ bool corners(const float *verts, int32_t n_verts, const int32_t *faces, int64_t f, V3 v[3]) {
  bool ok = true;
  for (int c = 0; c < 3; ++c) {
    const int32_t i = faces[3 * f + c];
    const bool in = i >= 0 && i < n_verts;
    v[c] = in ? ld3(verts, i) : nan3();
    ok = ok && in;
  }
  return ok;
}

// u / |u| and the length
__host__ __device__ __forceinline__ V3 unit(V3 u, float &len) {
  len = sqrtf(u.x * u.x + u.y * u.y + u.z * u.z);
  return V3{u.x / len, u.y / len, u.z / len};
}
// u = w / len: d w from d u
__host__ __device__ __forceinline__ V3 unit_backward(V3 u, float len, V3 du) {
  const float along = dot(u, du);
  return V3{(du.x - u.x * along) / len, (du.y - u.y * along) / len, (du.z - u.z * along) / len};
}

struct Frame {
  V3 e[3];                 // e1, e2, e3
  V3 n, fn, x, y, z;       // e1 x e2, n / |n|, and the three columns
  float n_len, fn_len, x_len, y_len;
  int longest;             // which edge x is
};

// No FMA contraction in what the decisions are taken on (the edge lengths, the matrix, the roots): the forward and the backward
// kernel then see the same bits and take the same edge and the same branch, wherever the compiler inlines this.
__host__ __device__ __forceinline__ Frame face_frame(const V3 v[3]) {
#pragma clang fp contract(off)
  Frame t;
  t.e[0] = sub(v[1], v[0]);
  t.e[1] = sub(v[2], v[1]);
  t.e[2] = sub(v[0], v[2]);
  float len[3];
  for (int k = 0; k < 3; ++k) len[k] = sqrtf(t.e[k].x * t.e[k].x + t.e[k].y * t.e[k].y + t.e[k].z * t.e[k].z);
  t.longest = 0;
  if (len[1] > len[t.longest]) t.longest = 1;
  if (len[2] > len[t.longest]) t.longest = 2;
  const V3 l = t.e[t.longest];
  t.x_len = len[t.longest];
  t.x = V3{l.x / t.x_len, l.y / t.x_len, l.z / t.x_len};
  t.n = cross(t.e[0], t.e[1]);
  t.fn = unit(t.n, t.n_len);
  t.z = unit(t.fn, t.fn_len);
  t.y = unit(cross(t.z, t.x), t.y_len);
  return t;
}

struct Quat {
  float q[4];     // WXYZ, w >= 0
  float num[4];   // the taken row before the division
  float root;     // the largest of the four roots
  float sgn;      // the sign applied
  int branch;     // which root it was
};

// the row of candidate `b`: num[b] = r_b^2, the others a difference or a sum of two off-diagonal entries
__host__ __device__ __forceinline__ void quat_row(const float m[3][3], int b, float r2, float num[4]) {
#pragma clang fp contract(off)
  switch (b) {
    case 0: num[0] = r2; num[1] = m[2][1] - m[1][2]; num[2] = m[0][2] - m[2][0]; num[3] = m[1][0] - m[0][1]; break;
    case 1: num[0] = m[2][1] - m[1][2]; num[1] = r2; num[2] = m[1][0] + m[0][1]; num[3] = m[0][2] + m[2][0]; break;
    case 2: num[0] = m[0][2] - m[2][0]; num[1] = m[1][0] + m[0][1]; num[2] = r2; num[3] = m[1][2] + m[2][1]; break;
    default: num[0] = m[1][0] - m[0][1]; num[1] = m[2][0] + m[0][2]; num[2] = m[2][1] + m[1][2]; num[3] = r2; break;
  }
}

// d m += from d num (entry b of gnum is not read) and the gradient gx of the root's argument 1 +- m00 +- m11 +- m22
__host__ __device__ __forceinline__ void quat_row_backward(int b, const float g[4], float gx, float dm[3][3]) {
  switch (b) {
    case 0:
      dm[0][0] += gx; dm[1][1] += gx; dm[2][2] += gx;
      dm[2][1] += g[1]; dm[1][2] -= g[1]; dm[0][2] += g[2]; dm[2][0] -= g[2]; dm[1][0] += g[3]; dm[0][1] -= g[3];
      break;
    case 1:
      dm[0][0] += gx; dm[1][1] -= gx; dm[2][2] -= gx;
      dm[2][1] += g[0]; dm[1][2] -= g[0]; dm[1][0] += g[2]; dm[0][1] += g[2]; dm[0][2] += g[3]; dm[2][0] += g[3];
      break;
    case 2:
      dm[0][0] -= gx; dm[1][1] += gx; dm[2][2] -= gx;
      dm[0][2] += g[0]; dm[2][0] -= g[0]; dm[1][0] += g[1]; dm[0][1] += g[1]; dm[1][2] += g[3]; dm[2][1] += g[3];
      break;
    default:
      dm[0][0] -= gx; dm[1][1] -= gx; dm[2][2] += gx;
      dm[1][0] += g[0]; dm[0][1] -= g[0]; dm[2][0] += g[1]; dm[0][2] += g[1]; dm[2][1] += g[2]; dm[1][2] += g[2];
      break;
  }
}

__host__ __device__ __forceinline__ Quat matrix_to_quat(const float m[3][3]) {
#pragma clang fp contract(off)
  const float arg[4] = {1.f + m[0][0] + m[1][1] + m[2][2], 1.f + m[0][0] - m[1][1] - m[2][2], 1.f - m[0][0] + m[1][1] - m[2][2],
                        1.f - m[0][0] - m[1][1] + m[2][2]};
  float root[4];
  for (int k = 0; k < 4; ++k) root[k] = arg[k] > 0.f ? sqrtf(arg[k]) : (arg[k] == arg[k] ? 0.f : arg[k]);  // NaN stays NaN
  Quat t;
  t.branch = 0;
  for (int k = 1; k < 4; ++k)
    if (root[k] > root[t.branch]) t.branch = k;  // the first of the largest
  t.root = root[t.branch];
  quat_row(m, t.branch, t.root * t.root, t.num);
  const float den = 2.f * fmaxf(t.root, 0.1f);
  float q[4];
  for (int k = 0; k < 4; ++k) q[k] = t.num[k] / den;
  t.sgn = q[0] < 0.f ? -1.f : 1.f;
  for (int k = 0; k < 4; ++k) t.q[k] = t.sgn * q[k];
  return t;
}

// d m (overwritten) from d q = G, branch and sign as the forward took them; root >= 1 on the taken row
__host__ __device__ __forceinline__ void matrix_to_quat_backward(const Quat &t, const float G[4], float dm[3][3]) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) dm[r][c] = 0.f;
  const float den = 2.f * t.root;
  float g[4], along = 0.f;
  for (int k = 0; k < 4; ++k) {
    g[k] = t.sgn * G[k] / den;   // d num_k
    along += g[k] * t.num[k];
  }
  // num_b = r^2 and every entry is divided by 2 r: d r = 2 r g_b - (sum_k g_k num_k) / r, and d arg = d r / (2 r)
  const float g_root = 2.f * t.root * g[t.branch] - along / t.root;
  quat_row_backward(t.branch, g, g_root / (2.f * t.root), dm);
}

__host__ __device__ __forceinline__ void frame_matrix(const Frame &t, float m[3][3]) {
  m[0][0] = t.x.x; m[1][0] = t.x.y; m[2][0] = t.x.z;
  m[0][1] = t.y.x; m[1][1] = t.y.y; m[2][1] = t.y.z;
  m[0][2] = t.z.x; m[1][2] = t.z.y; m[2][2] = t.z.z;
}

// the gradient of the three corners from d x, d y, d z (the matrix's columns), d |n| (through the area) and d centre
__host__ __device__ __forceinline__ void frame_backward(const Frame &t, V3 gx, V3 gy, V3 gz, float g_nlen, V3 gc, V3 out[3]) {
  const V3 g_yu = unit_backward(t.y, t.y_len, gy);          // y = (z x x) / |z x x|
  gz = add(gz, cross(t.x, g_yu));
  gx = add(gx, cross(g_yu, t.z));
  const V3 g_fn = unit_backward(t.z, t.fn_len, gz);         // z = fn / |fn|
  V3 g_n = unit_backward(t.fn, t.n_len, g_fn);              // fn = n / |n|
  g_n = add(g_n, mul(t.fn, g_nlen));
  V3 ge[3] = {cross(t.e[1], g_n), cross(g_n, t.e[0]), V3{0.f, 0.f, 0.f}};   // n = e1 x e2
  ge[t.longest] = add(ge[t.longest], unit_backward(t.x, t.x_len, gx));
  const V3 third = mul(gc, 1.f / 3.f);
  out[0] = add(third, sub(ge[2], ge[0]));
  out[1] = add(third, sub(ge[0], ge[1]));
  out[2] = add(third, sub(ge[1], ge[2]));
}

// ---- params2rendervar ------------------------------------------------------------------------------------------------------------

// row f of means3D [F, 3], rotations [F, 4], scales [F, 3], opacities [F]
__host__ __device__ __forceinline__ void render_vars_forward(int64_t f, int32_t n_verts, const float *verts, const int32_t *faces,
                                                             const float *log_scales, const float *logit_opac, float *means, float *rot,
                                                             float *scales, float *opac) {
  V3 v[3];
  corners(verts, n_verts, faces, f, v);
  st3(means, f, V3{(v[0].x + v[1].x + v[2].x) / 3.f, (v[0].y + v[1].y + v[2].y) / 3.f, (v[0].z + v[1].z + v[2].z) / 3.f});
  const Frame t = face_frame(v);
  float m[3][3];
  frame_matrix(t, m);
  const Quat q = matrix_to_quat(m);
  for (int k = 0; k < 4; ++k) rot[4 * f + k] = q.q[k];
  for (int k = 0; k < 3; ++k) scales[3 * f + k] = expf(log_scales[3 * f + k]);
  opac[f] = sigmoid(logit_opac[f]);
}

// Row f of the backward: d_stencil[f, c, :] (9 floats, if wanted) from g_means and g_rot (either may be NULL = zeros), and the two
// elementwise gradients where wanted.
__host__ __device__ __forceinline__ void render_vars_backward(int64_t f, int32_t n_verts, const float *verts, const int32_t *faces,
                                                              const float *log_scales, const float *logit_opac, const float *g_means,
                                                              const float *g_rot, const float *g_scales, const float *g_opac,
                                                              float *d_stencil, float *d_log_scales, float *d_logit_opac) {
  if (d_stencil) {
    V3 v[3], out[3];
    corners(verts, n_verts, faces, f, v);
    const V3 gc = g_means ? ld3(g_means, f) : V3{0.f, 0.f, 0.f};
    if (g_rot) {
      const Frame t = face_frame(v);
      float m[3][3], dm[3][3];
      frame_matrix(t, m);
      const Quat q = matrix_to_quat(m);
      const float G[4] = {g_rot[4 * f], g_rot[4 * f + 1], g_rot[4 * f + 2], g_rot[4 * f + 3]};
      matrix_to_quat_backward(q, G, dm);
      frame_backward(t, V3{dm[0][0], dm[1][0], dm[2][0]}, V3{dm[0][1], dm[1][1], dm[2][1]}, V3{dm[0][2], dm[1][2], dm[2][2]}, 0.f, gc, out);
    } else {
      const bool ok = v[0].x == v[0].x && v[1].x == v[1].x && v[2].x == v[2].x;   // an index out of range: NaN, as the forward
      out[0] = out[1] = out[2] = ok ? mul(gc, 1.f / 3.f) : nan3();
    }
    for (int c = 0; c < 3; ++c) st3(d_stencil, 3 * f + c, out[c]);
  }
  if (d_log_scales)
    for (int k = 0; k < 3; ++k) d_log_scales[3 * f + k] = g_scales ? g_scales[3 * f + k] * expf(log_scales[3 * f + k]) : 0.f;
  if (d_logit_opac) {
    const float s = sigmoid(logit_opac[f]);
    d_logit_opac[f] = g_opac ? g_opac[f] * s * (1.f - s) : 0.f;
  }
}

// compute_face_normals and compute_face_areas for row f (either output may be NULL)
__host__ __device__ __forceinline__ void face_geometry(int64_t f, int32_t n_verts, const float *verts, const int32_t *faces, float *normals,
                                                       float *areas) {
  V3 v[3];
  corners(verts, n_verts, faces, f, v);
  const Frame t = face_frame(v);
  if (normals) st3(normals, f, t.fn);
  if (areas) areas[f] = t.n_len / 2.f;
}

// ---- the three loss terms --------------------------------------------------------------------------------------------------------

struct Terms {
  float area, scale, opacity;  // row f's summands
};

__host__ __device__ __forceinline__ float area_gap(const Frame &t, const float *log_scales, int64_t f, float &s01) {
#pragma clang fp contract(off)
  s01 = expf(log_scales[3 * f]) * expf(log_scales[3 * f + 1]) * PI_F;
  return t.n_len / 2.f - s01;
}

__host__ __device__ __forceinline__ Terms terms_forward(int64_t f, int32_t n_verts, const float *verts, const int32_t *faces,
                                                        const float *log_scales, const float *logit_opac) {
  V3 v[3];
  corners(verts, n_verts, faces, f, v);
  float s01;
  const float gap = area_gap(face_frame(v), log_scales, f, s01);
  return Terms{fabsf(gap), expf(log_scales[3 * f + 2]), 1.f - sigmoid(logit_opac[f])};
}

// g [3]: upstream of (area, scale, opacity).  Each output is written in full where wanted.
__host__ __device__ __forceinline__ void terms_backward(int64_t f, int32_t n_faces, int32_t n_verts, const float *verts, const int32_t *faces,
                                                        const float *log_scales, const float *logit_opac, const float *g, float *d_stencil,
                                                        float *d_log_scales, float *d_logit_opac) {
  const float inv = 1.f / (float)n_faces;
  float s01 = 0.f, sg = 0.f;
  if (d_stencil || d_log_scales) {
    V3 v[3], out[3];
    corners(verts, n_verts, faces, f, v);
    const Frame t = face_frame(v);
    sg = sign(area_gap(t, log_scales, f, s01)) * g[0] * inv;
    if (t.n_len != t.n_len) sg = NAN;
    if (d_stencil) {
      const V3 zero{0.f, 0.f, 0.f};
      // |n| alone: the gradient of n is (sg / 2) n / |n|, which frame_backward adds as g_nlen * fn
      const V3 g_n = mul(t.fn, 0.5f * sg);
      out[0] = sub(zero, cross(t.e[1], g_n));                          // e1 = v2 - v1, e2 = v3 - v2
      out[1] = sub(cross(t.e[1], g_n), cross(g_n, t.e[0]));
      out[2] = cross(g_n, t.e[0]);
      for (int c = 0; c < 3; ++c) st3(d_stencil, 3 * f + c, out[c]);
    }
  }
  if (d_log_scales) {
    d_log_scales[3 * f] = d_log_scales[3 * f + 1] = -sg * s01;
    d_log_scales[3 * f + 2] = g[1] * inv * expf(log_scales[3 * f + 2]);
  }
  if (d_logit_opac) {
    const float s = sigmoid(logit_opac[f]);
    d_logit_opac[f] = -(g[2] * inv) * s * (1.f - s);
  }
}

// ---- compute_vertex_normals ------------------------------------------------------------------------------------------------------

// vertex v: its corners items[start[v] .. start[v + 1]) (item = 3 face + position) in ascending order, each face's (v0 - v1) x (v2 - v1)
__host__ __device__ __forceinline__ void vertex_normal(int64_t v, int32_t n_verts, const float *verts, const int32_t *faces, const int32_t *start,
                                                       const int32_t *items, float *normals) {
  V3 s{0.f, 0.f, 0.f};
  for (int32_t i = start[v]; i < start[v + 1]; ++i) {
    V3 p[3];
    corners(verts, n_verts, faces, items[i] / 3, p);
    s = add(s, cross(sub(p[0], p[1]), sub(p[2], p[1])));
  }
  float len;
  st3(normals, v, unit(s, len));
}

// ---- collision_penalty -----------------------------------------------------------------------------------------------------------

// d = -nb[j] . (va[i] - vb[j]); j must be in range
__host__ __device__ __forceinline__ float signed_distance(int64_t i, const float *va, const float *vb, const float *nb, int64_t j) {
#pragma clang fp contract(off)
  const V3 o = sub(ld3(va, i), ld3(vb, j)), n = ld3(nb, j);
  return -n.x * o.x + -n.y * o.y + -n.z * o.z;
}

// the summand of point i from its distance
__host__ __device__ __forceinline__ float penalty(float d, float eps, int mode) {
  const float pen = fmaxf(eps - d, 0.f);
  return mode == MODE_CUBED ? pen * pen * pen : pen;
}

// d va[i] from the saved distance and index (of n_body).  g: [n] in the distance mode, [1] in the two penalty modes.
__host__ __device__ __forceinline__ void collision_backward(int64_t i, int32_t n, const float *nb, int32_t n_body, const int32_t *index,
                                                            const float *dist, float eps, int mode, const float *g, float *d_va) {
  const int32_t j = index[i];
  if (j < 0 || j >= n_body) {  // not an index the forward wrote: reads nothing
    st3(d_va, i, nan3());
    return;
  }
  const V3 nj = ld3(nb, j);
  float c;
  if (mode == MODE_DISTANCE) {
    c = -g[i];
  } else {
    const float gap = eps - dist[i];
    const float slope = gap > 0.f ? 1.f : (gap < 0.f ? 0.f : (gap == gap ? 0.5f : gap));
    c = mode == MODE_AVERAGE ? g[0] * slope / (float)n : g[0] * 3.f * (gap * gap) * slope;
  }
  st3(d_va, i, mul(nj, c));
}

}  // namespace trk
