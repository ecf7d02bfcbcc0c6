// frames_grad_math.hpp -- the backward pass of frames.hip: the exact derivative of frm::face_frame_row (frames_math.hpp, whose
// pieces it calls where it needs the per-face forward's values) and of the binding expressions of k_bind_gaussians /
// k_render_inputs as those kernels compute them, with every discrete decision held fixed
// (the rasteriser's policy, raster_grad_math.hpp): the quaternion branch, the sign inside fabsf (sign(0) = 0), and the three
// clamps -- max(dot, 1e-20) inside length(), max(|q|, 1e-12) inside normalize4() -- which pass zero slope to the clamped
// quantity where they bind.  Plain C++ for the device (frames_backward.hip) and the host (tests/hostframes_grad/) alike: one
// function per work item, so the kernels and the host loops are the same statements.  All arithmetic is fp32.
//
// Forward, per Gaussian g bound to face f (M, Q, s, c = the face's matrix, quaternion WXYZ, scale, centre):
//   mean = (M p) s + c,  rotation = normalize(Q) (x) normalize(r),  scale_k = exp(sigma_k) s,  opacity = 1 / (1 + exp(-o))
// so with the upstream Gm, Gr, Gs, Go
//   d p = s M^T Gm,  d sigma_k = Gs_k exp(sigma_k) s,  d o = Go y (1 - y),  d r through the product and x / max(|x|, 1e-12)
//   d c = sum Gm,  d M = sum s Gm p^T,  d s = sum [Gm . (M p) + sum_k Gs_k exp(sigma_k)],  d Q through the product and the
//   normalisation of Q; the sums run over the face's Gaussians in ascending Gaussian index.
// Forward, per face: e1 = v1 - v0, e2 = v2 - v0, a0 = e1 / |e1|, a1 = (a0 x e2) / |.|, a2 = -(a1 x a0) / |.|, M = [a0 a1 a2],
// s = (|e1| + |a2 . e2|) / 2, c = (v0 + v1 + v2) / 3, Q = rotmat_to_unitquat(M).  The backward walks that chain in reverse.
#pragma once
#include "frames_math.hpp"

namespace fgrad {

using frm::V3;
using frm::add;
using frm::cross;
using frm::dot;
using frm::ld3;
using frm::mul;
using frm::sub;
using frm::LEN_EPS;
using frm::normalize4;

// u = x / l with l = sqrt(max(x . x, 1e-20)): d x from d u.  Free clamp: (d u - u (u . d u)) / l; bound clamp: l is a constant.
__host__ __device__ __forceinline__ V3 safe_normalize_backward(V3 x, V3 du, V3 &u, float &l) {
  float d = dot(x, x);
  l = sqrtf(fmaxf(d, LEN_EPS));
  u = V3{x.x / l, x.y / l, x.z / l};
  if (d < LEN_EPS) return V3{du.x / l, du.y / l, du.z / l};
  float along = dot(u, du);
  return V3{(du.x - u.x * along) / l, (du.y - u.y * along) / l, (du.z - u.z * along) / l};
}

// u = q / n (frm::normalize4, or the unclamped q / |q| of the matrix -> quaternion map): d q from d u
__host__ __device__ __forceinline__ void normalize4_backward(const float u[4], float n, bool bound, const float du[4], float dq[4]) {
  float along = bound ? 0.0f : u[0] * du[0] + u[1] * du[1] + u[2] * du[2] + u[3] * du[3];
  for (int k = 0; k < 4; ++k) dq[k] = (du[k] - u[k] * along) / n;
}

// o = p (x) q, Hamilton product in WXYZ as k_bind_gaussians writes it: d p and d q from d o = G
__host__ __device__ __forceinline__ void quat_product_backward(const float p[4], const float q[4], const float G[4], float dp[4], float dq[4]) {
  dp[0] = G[0] * q[0] + G[1] * q[1] + G[2] * q[2] + G[3] * q[3];
  dp[1] = -G[0] * q[1] + G[1] * q[0] - G[2] * q[3] + G[3] * q[2];
  dp[2] = -G[0] * q[2] + G[1] * q[3] + G[2] * q[0] - G[3] * q[1];
  dp[3] = -G[0] * q[3] - G[1] * q[2] + G[2] * q[1] + G[3] * q[0];
  dq[0] = G[0] * p[0] + G[1] * p[1] + G[2] * p[2] + G[3] * p[3];
  dq[1] = -G[0] * p[1] + G[1] * p[0] + G[2] * p[3] - G[3] * p[2];
  dq[2] = -G[0] * p[2] - G[1] * p[3] + G[2] * p[0] + G[3] * p[1];
  dq[3] = -G[0] * p[3] + G[1] * p[2] - G[2] * p[1] + G[3] * p[0];
}

// ---- kernel 1: one Gaussian, the four parameter gradients --------------------------------------------------------------------
// A null upstream counts as zero, a null output is not wanted.  g_* are rows of the rasteriser's argument lists (row g of each).
__host__ __device__ __forceinline__ void gaussian_backward(int64_t g, const int32_t *binding, const float *rot_raw, const float *scaling_raw,
                                                           const float *opacity_raw, const float *mat, const float *quat, const float *fscale,
                                                           const float *g_mean, const float *g_rot, const float *g_scale, const float *g_opac,
                                                           float *d_xyz, float *d_rot, float *d_scaling, float *d_opacity) {
  const int64_t f = binding[g];
  const float s = fscale[f];
  if (d_xyz) {
    V3 o{0.0f, 0.0f, 0.0f};
    if (g_mean) {
      const float *m = mat + 9 * f;
      V3 G = ld3(g_mean, g);
      o = V3{(m[0] * G.x + m[3] * G.y + m[6] * G.z) * s, (m[1] * G.x + m[4] * G.y + m[7] * G.z) * s, (m[2] * G.x + m[5] * G.y + m[8] * G.z) * s};
    }
    d_xyz[3 * g] = o.x; d_xyz[3 * g + 1] = o.y; d_xyz[3 * g + 2] = o.z;
  }
  if (d_rot) {
    float db[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (g_rot) {
      float a[4], b[4], G[4], ua[4], ub[4], na, nb, da[4], dub[4];
      bool ba, bb;
      for (int k = 0; k < 4; ++k) { a[k] = quat[4 * f + k]; b[k] = rot_raw[4 * g + k]; G[k] = g_rot[4 * g + k]; }
      normalize4(a, ua, na, ba);
      normalize4(b, ub, nb, bb);
      quat_product_backward(ua, ub, G, da, dub);
      normalize4_backward(ub, nb, bb, dub, db);
    }
    for (int k = 0; k < 4; ++k) d_rot[4 * g + k] = db[k];
  }
  if (d_scaling)
    for (int k = 0; k < 3; ++k) d_scaling[3 * g + k] = g_scale ? g_scale[3 * g + k] * expf(scaling_raw[3 * g + k]) * s : 0.0f;
  if (d_opacity) {
    float o = 0.0f;
    if (g_opac) {
      float y = 1.0f / (1.0f + expf(-opacity_raw[g]));
      o = g_opac[g] * (y * (1.0f - y));
    }
    d_opacity[g] = o;
  }
}

// ---- kernel 2: one face, the sums over its Gaussians items[start[f] .. start[f + 1]) in that (ascending) order --------------------
__host__ __device__ __forceinline__ void face_accumulate(int64_t f, const int32_t *start, const int32_t *items, const float *xyz_local,
                                                         const float *rot_raw, const float *scaling_raw, const float *mat, const float *quat,
                                                         const float *fscale, const float *g_mean, const float *g_rot, const float *g_scale,
                                                         float *d_center, float *d_mat, float *d_quat, float *d_fscale) {
  float dc[3] = {0.0f, 0.0f, 0.0f}, dm[9], da[4] = {0.0f, 0.0f, 0.0f, 0.0f}, ds = 0.0f;
  for (int k = 0; k < 9; ++k) dm[k] = 0.0f;
  const int32_t lo = start[f], hi = start[f + 1];
  float dq[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (hi > lo) {
    const float *m = mat + 9 * f;
    const float s = fscale[f];
    float a[4], ua[4], na;
    bool ba;
    for (int k = 0; k < 4; ++k) a[k] = quat[4 * f + k];
    normalize4(a, ua, na, ba);
    for (int32_t i = lo; i < hi; ++i) {
      const int64_t g = items[i];
      if (g_mean) {
        V3 G = ld3(g_mean, g), p = ld3(xyz_local, g);
        dc[0] += G.x; dc[1] += G.y; dc[2] += G.z;
        const float Gv[3] = {G.x, G.y, G.z}, pv[3] = {p.x, p.y, p.z};
        for (int r = 0; r < 3; ++r)
          for (int c = 0; c < 3; ++c) dm[3 * r + c] += s * Gv[r] * pv[c];
        ds += G.x * (m[0] * p.x + m[1] * p.y + m[2] * p.z) + G.y * (m[3] * p.x + m[4] * p.y + m[5] * p.z) +
              G.z * (m[6] * p.x + m[7] * p.y + m[8] * p.z);
      }
      if (g_scale)
        ds += g_scale[3 * g] * expf(scaling_raw[3 * g]) + g_scale[3 * g + 1] * expf(scaling_raw[3 * g + 1]) +
              g_scale[3 * g + 2] * expf(scaling_raw[3 * g + 2]);
      if (g_rot) {
        float b[4], G[4], ub[4], nb, dua[4], dub[4];
        bool bb;
        for (int k = 0; k < 4; ++k) { b[k] = rot_raw[4 * g + k]; G[k] = g_rot[4 * g + k]; }
        normalize4(b, ub, nb, bb);
        quat_product_backward(ua, ub, G, dua, dub);
        for (int k = 0; k < 4; ++k) da[k] += dua[k];
      }
    }
    normalize4_backward(ua, na, ba, da, dq);  // the normalisation of Q is the face's own: once, after the sum
  }
  for (int k = 0; k < 3; ++k) d_center[3 * f + k] = dc[k];
  for (int k = 0; k < 9; ++k) d_mat[9 * f + k] = dm[k];
  for (int k = 0; k < 4; ++k) d_quat[4 * f + k] = dq[k];
  d_fscale[f] = ds;
}

// ---- kernel 3: one face, from the upstream of its four outputs to the gradients of its three corners [3][3] ------------------
// mat_saved / quat_saved are the forward's outputs: the branch of the matrix -> quaternion map is the first maximum of
// (R00, R11, R22, trace) of THOSE floats, the ones the forward chose from, and the unit quaternion is the one it wrote.
// Everything else is recomputed from the vertices.  A null upstream counts as zero.
__host__ __device__ __forceinline__ void face_frames_backward(int64_t f, const float *verts, const int32_t *faces, const float *mat_saved,
                                                              const float *quat_saved, const float *g_center, const float *g_mat,
                                                              const float *g_quat, const float *g_fscale, float *d_corner) {
  const int64_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
  V3 v0 = ld3(verts, i0), v1 = ld3(verts, i1), v2 = ld3(verts, i2);
  float dR[3][3];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) dR[r][c] = g_mat ? g_mat[9 * f + 3 * r + c] : 0.0f;
  if (g_quat) {
    float R[3][3];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) R[r][c] = mat_saved[9 * f + 3 * r + c];
    const int b = frm::quat_branch(R);
    const int i = b, j = (i + 1) % 3, k = (j + 1) % 3;
    float q[4];  // XYZW before the normalisation
    frm::quat_numerators(R, b, q);
    const float n = frm::norm4(q);
    const float *qs = quat_saved + 4 * f, *gq = g_quat + 4 * f;
    float u[4] = {qs[1], qs[2], qs[3], qs[0]}, du[4] = {gq[1], gq[2], gq[3], gq[0]}, dq[4];  // WXYZ -> XYZW
    normalize4_backward(u, n, false, du, dq);  // q / n, no clamp in this one
    if (b != 3) {
      dR[i][i] += dq[i]; dR[j][j] -= dq[i]; dR[k][k] -= dq[i];
      dR[j][i] += dq[j]; dR[i][j] += dq[j];
      dR[k][i] += dq[k]; dR[i][k] += dq[k];
      dR[k][j] += dq[3]; dR[j][k] -= dq[3];
    } else {
      dR[2][1] += dq[0]; dR[1][2] -= dq[0];
      dR[0][2] += dq[1]; dR[2][0] -= dq[1];
      dR[1][0] += dq[2]; dR[0][1] -= dq[2];
      dR[0][0] += dq[3]; dR[1][1] += dq[3]; dR[2][2] += dq[3];
    }
  }
  V3 da0{dR[0][0], dR[1][0], dR[2][0]}, da1{dR[0][1], dR[1][1], dR[2][1]}, da2{dR[0][2], dR[1][2], dR[2][2]};
  const frm::FaceChain ch = frm::face_chain(v0, v1, v2);  // the forward's own values; the walk back starts here
  const V3 e1 = ch.e1, e2 = ch.e2, a0 = ch.a0, c1 = ch.c1, a1 = ch.a1, c2 = ch.c2, a2 = ch.a2;
  // s = (|e1| + |t|) / 2, t = a2 . e2
  float dl1 = 0.0f;
  V3 de2{0.0f, 0.0f, 0.0f};
  if (g_fscale) {
    float h = 0.5f * g_fscale[f];
    float t = dot(a2, e2);
    float dt = t > 0.0f ? h : (t < 0.0f ? -h : 0.0f);
    dl1 = h;
    da2 = add(da2, mul(e2, dt));
    de2 = mul(a2, dt);
  }
  // a2 = -n2, n2 = c2 / |c2|, c2 = a1 x a0
  V3 un, dc2;
  float ln;
  dc2 = safe_normalize_backward(c2, V3{-da2.x, -da2.y, -da2.z}, un, ln);
  da1 = add(da1, cross(a0, dc2));
  da0 = add(da0, cross(dc2, a1));
  // a1 = c1 / |c1|, c1 = a0 x e2
  V3 dc1 = safe_normalize_backward(c1, da1, un, ln);
  da0 = add(da0, cross(e2, dc1));
  de2 = add(de2, cross(dc1, a0));
  // a0 = e1 / |e1|, and |e1| inside the scale
  V3 de1 = safe_normalize_backward(e1, da0, un, ln);
  if (!(dot(e1, e1) < LEN_EPS)) de1 = add(de1, mul(a0, dl1));
  V3 gc{0.0f, 0.0f, 0.0f};
  if (g_center) gc = V3{g_center[3 * f] / 3.0f, g_center[3 * f + 1] / 3.0f, g_center[3 * f + 2] / 3.0f};
  float *o = d_corner + 9 * f;
  o[0] = gc.x - de1.x - de2.x; o[1] = gc.y - de1.y - de2.y; o[2] = gc.z - de1.z - de2.z;
  o[3] = gc.x + de1.x; o[4] = gc.y + de1.y; o[5] = gc.z + de1.z;
  o[6] = gc.x + de2.x; o[7] = gc.y + de2.y; o[8] = gc.z + de2.z;
}

// ---- kernel 4: one vertex, the sum of its corners corners[start[v] .. start[v + 1]) (corner = 3 face + position) in that order ---
__host__ __device__ __forceinline__ void vertex_gather(int64_t v, const int32_t *start, const int32_t *corners, const float *d_corner,
                                                       float *d_verts) {
  float x = 0.0f, y = 0.0f, z = 0.0f;
  for (int32_t i = start[v]; i < start[v + 1]; ++i) {
    const int64_t c = corners[i];
    x += d_corner[3 * c]; y += d_corner[3 * c + 1]; z += d_corner[3 * c + 2];
  }
  d_verts[3 * v] = x; d_verts[3 * v + 1] = y; d_verts[3 * v + 2] = z;
}

}  // namespace fgrad
