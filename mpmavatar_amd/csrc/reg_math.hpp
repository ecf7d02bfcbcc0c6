// reg_math.hpp -- the regularisation terms of the appearance loop (train_appearance.py:136-150), per work item:
//   mesh (scene/mesh_gaussian_model.py:203-246, set-up :88-98), F faces, K = 3 neighbours nb[f, k] per face
//     normal = mean_f | mean_k(n_f . n_nb) - 1 |              n_f = d3 / |d3|, d3 = (v2 - v1) x (v3 - v1)
//     iso    = mean_fk sqrt((sqrt(|c_nb - c_f|^2 + 1e-20) - nd[f, k])^2 nw[f, k] + 1e-20)        c_f the face centre
//     area   = mean_f | a_f - mean(a) |                        a_f = |d3| / 2
//   Gaussians (train_appearance.py:138,147,148, scene/gaussian_model.py:158), n rows, visible = radii > 0
//     opacity = mean(1 - sigmoid(_opacity));  xyz = mean over visible of relu(|_xyz| - t_xyz)
//     scale   = mean over visible of | relu(exp(_scaling) - t_scale) |_2
// and the exact derivative of those expressions with every discrete decision held fixed: sign(0) = 0 inside abs, a relu that
// binds has zero slope, the norm of an all-zero row has zero slope.  A row of nb may name its own face (the reference pads
// boundary faces that way, utils/general_utils.py:309-311): n_f . n_f is identically 1 and the offset identically 0, so such a slot
// receives exactly nothing and sends exactly nothing.  A zero-area face gives NaN in `normal`, as in the reference; not clamped.
// nb need not be symmetric.  An index outside its range reads nothing and gives NaN.
// Plain C++ for the device (reg.hip) and the host (tests/hostreg/) alike: one function per work item.  All arithmetic is fp32;
// the sums over faces and Gaussians are the caller's (double, fixed order).
//
// Mesh backward: row f of the loss touches a stencil of 1 + K faces x 3 corners, S[f, s, c] = faces[nbx[f, s], c] with
// nbx[f, 0] = f.  face_backward writes the gradient of row f's terms to each stencil corner, d_stencil[f, s, c, :]; a vertex then
// sums its CSR segment of those rows in ascending item order (fgrad::vertex_gather).  No floating-point atomics anywhere.
#pragma once
#include "frames_grad_math.hpp"

#include <math.h>
#include <stdint.h>

namespace reg {

constexpr int K = 3;             // neighbours per face
constexpr int STENCIL = 1 + K;   // faces a row touches
constexpr int ROW = STENCIL * 9; // floats of d_stencil per face

using frm::V3;  // with its operators + - *, found through the type
using frm::cross;
using frm::dot;
using frm::sign;

struct Face {
  V3 d1, d2, n, c;  // the two edges from v1, the unit normal, the centre
  float len, a;     // |d3| and the area
};

// No FMA contraction in the geometry: the forward pass, the backward pass and the set-up (which measures neighbor_dist with this
// very function) then see the same bits for a_f and for the squared distances, wherever the compiler inlines them.
__host__ __device__ __forceinline__ Face face_geom(const float *verts, int32_t n_verts, const int32_t *faces, int64_t f) {
#pragma clang fp contract(off)
  const int32_t i1 = faces[3 * f], i2 = faces[3 * f + 1], i3 = faces[3 * f + 2];
  if (i1 < 0 || i1 >= n_verts || i2 < 0 || i2 >= n_verts || i3 < 0 || i3 >= n_verts) {
    const V3 q{NAN, NAN, NAN};
    return Face{q, q, q, q, NAN, NAN};
  }
  const V3 v1{verts[3 * (int64_t)i1], verts[3 * (int64_t)i1 + 1], verts[3 * (int64_t)i1 + 2]};
  const V3 v2{verts[3 * (int64_t)i2], verts[3 * (int64_t)i2 + 1], verts[3 * (int64_t)i2 + 2]};
  const V3 v3{verts[3 * (int64_t)i3], verts[3 * (int64_t)i3 + 1], verts[3 * (int64_t)i3 + 2]};
  Face g;
  g.d1 = v2 - v1;
  g.d2 = v3 - v1;
  const V3 d3 = cross(g.d1, g.d2);
  g.len = sqrtf(d3.x * d3.x + d3.y * d3.y + d3.z * d3.z);
  g.n = V3{d3.x / g.len, d3.y / g.len, d3.z / g.len};
  g.a = 0.5f * g.len;
  g.c = V3{(v1.x + v2.x + v3.x) / 3.f, (v1.y + v2.y + v3.y) / 3.f, (v1.z + v2.z + v3.z) / 3.f};
  return g;
}

__host__ __device__ __forceinline__ float sq_norm(V3 o) {
#pragma clang fp contract(off)
  return o.x * o.x + o.y * o.y + o.z * o.z;
}

struct FaceTerms {
  float normal, iso, area;  // | m_f - 1 |, the sum over k of the iso term, a_f
};

// Row f of the three sums.  sq_dist [F * K] or NULL: |c_nb - c_f|^2 of every slot, which the set-up turns into neighbor_dist and
// neighbor_weight (nd and nw play no part in it).
__host__ __device__ __forceinline__ FaceTerms face_forward(int64_t f, int32_t n_faces, int32_t n_verts, const float *verts, const int32_t *faces,
                                                           const int32_t *nb, const float *nd, const float *nw, float *sq_dist) {
  const Face own = face_geom(verts, n_verts, faces, f);
  float dots = 0.f, iso = 0.f;
  for (int k = 0; k < K; ++k) {
    const int32_t j = nb[K * f + k];
    if (j < 0 || j >= n_faces) {
      dots = NAN; iso = NAN;
      if (sq_dist) sq_dist[K * f + k] = NAN;
      continue;
    }
    const Face h = j == f ? own : face_geom(verts, n_verts, faces, j);
    dots += dot(own.n, h.n);
    const float sq = sq_norm(h.c - own.c);
    if (sq_dist) sq_dist[K * f + k] = sq;
    const float r = sqrtf(sq + 1e-20f) - nd[K * f + k];
    iso += sqrtf(r * r * nw[K * f + k] + 1e-20f);
  }
  return FaceTerms{fabsf(dots / (float)K - 1.f), iso, own.a};
}

// the gradient of one stencil face's three corners from the gradients of its unit normal (gn), area (ga) and centre (gc)
__host__ __device__ __forceinline__ void corner_rows(const Face &h, V3 gn, float ga, V3 gc, float *rows) {
  const V3 gd3 = (1.f / h.len) * (gn - dot(h.n, gn) * h.n) + (0.5f * ga) * h.n;
  const V3 gd1 = cross(h.d2, gd3), gd2 = cross(gd3, h.d1), third = (1.f / 3.f) * gc;
  const V3 r1 = third - gd1 - gd2, r2 = third + gd1, r3 = third + gd2;
  rows[0] = r1.x; rows[1] = r1.y; rows[2] = r1.z;
  rows[3] = r2.x; rows[4] = r2.y; rows[5] = r2.z;
  rows[6] = r3.x; rows[7] = r3.y; rows[8] = r3.z;
}

// d_stencil[f, :, :, :] (ROW floats, all written).  stats = {mean(a), mean(sign(a - mean(a)))} of the forward pass; g [3] the upstream
// gradients of (normal, iso, area).  d area / d a_f = (s_f - mean(s)) / F: the mean is a function of every face.
__host__ __device__ __forceinline__ void face_backward(int64_t f, int32_t n_faces, int32_t n_verts, const float *verts, const int32_t *faces,
                                                       const int32_t *nb, const float *nd, const float *nw, const float *stats, const float *g,
                                                       float *d_stencil) {
  const Face own = face_geom(verts, n_verts, faces, f);
  const float inv_f = 1.f / (float)n_faces;
  Face h[K];
  bool live[K];  // a slot that is neither the face itself nor out of range
  float dots = 0.f;
  for (int k = 0; k < K; ++k) {
    const int32_t j = nb[K * f + k];
    const bool in = j >= 0 && j < n_faces;
    live[k] = in && j != f;
    h[k] = live[k] ? face_geom(verts, n_verts, faces, j) : own;
    dots += in ? dot(own.n, h[k].n) : NAN;
  }
  const float s_n = sign(dots / (float)K - 1.f) * g[0] * inv_f / (float)K, c_iso = g[1] * inv_f / (float)K;
  V3 gn_own{0.f, 0.f, 0.f}, gc_own{0.f, 0.f, 0.f};
  float *row = d_stencil + (int64_t)ROW * f;
  for (int k = 0; k < K; ++k) {
    float *out = row + 9 * (1 + k);
    if (!live[k]) {
      for (int i = 0; i < 9; ++i) out[i] = 0.f;
      continue;
    }
    const V3 o = h[k].c - own.c;
    const float mag = sqrtf(sq_norm(o) + 1e-20f), r = mag - nd[K * f + k], w = nw[K * f + k];
    const float q = sqrtf(r * r * w + 1e-20f);
    const V3 gc = (c_iso * (r * w / q) / mag) * o;
    gn_own = gn_own + s_n * h[k].n;
    gc_own = gc_own - gc;
    corner_rows(h[k], s_n * own.n, 0.f, gc, out);
  }
  const float ga = g[2] * inv_f * (sign(own.a - stats[0]) - stats[1]);
  corner_rows(own, gn_own, ga, gc_own, row);
}

// ---- the Gaussian terms ------------------------------------------------------------------------------------------------------

__host__ __device__ __forceinline__ bool is_visible(const int32_t *radii, const uint8_t *mask, int64_t i) {
  return radii ? radii[i] > 0 : mask[i] != 0;
}

struct GaussTerms {
  float opacity, xyz, scale;  // row i's summands; the last two are zero outside the visible rows
  bool visible;
};

__host__ __device__ __forceinline__ GaussTerms gauss_forward(int64_t i, const float *opacity, const float *xyz, const float *scaling,
                                                             const int32_t *radii, const uint8_t *mask, float t_xyz, float t_scale) {
  GaussTerms t{1.f - 1.f / (1.f + expf(-opacity[i])), 0.f, 0.f, is_visible(radii, mask, i)};
  if (!t.visible) return t;
  const float nrm = sqrtf(sq_norm(V3{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]}));
  t.xyz = fmaxf(nrm - t_xyz, 0.f);
  const V3 u{fmaxf(expf(scaling[3 * i]) - t_scale, 0.f), fmaxf(expf(scaling[3 * i + 1]) - t_scale, 0.f), fmaxf(expf(scaling[3 * i + 2]) - t_scale, 0.f)};
  t.scale = sqrtf(sq_norm(u));
  return t;
}

// Row i of the three gradients, each written in full where wanted.  g [3]: upstream of (opacity, xyz, scale); n_visible [1]: the
// forward's count.  A row outside the visible set gets exact zeros for the two filtered terms, whatever the count.
__host__ __device__ __forceinline__ void gauss_backward(int64_t i, int32_t n, const float *opacity, const float *xyz, const float *scaling,
                                                        const int32_t *radii, const uint8_t *mask, float t_xyz, float t_scale,
                                                        const int32_t *n_visible, const float *g, float *d_opacity, float *d_xyz, float *d_scaling) {
  if (d_opacity) {
    const float s = 1.f / (1.f + expf(-opacity[i]));
    d_opacity[i] = -(g[0] / (float)n) * s * (1.f - s);
  }
  if (!d_xyz && !d_scaling) return;
  const bool vis = is_visible(radii, mask, i);
  const float inv = vis ? 1.f / (float)n_visible[0] : 0.f;
  if (d_xyz) {
    V3 d{0.f, 0.f, 0.f};
    if (vis) {
      const V3 x{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
      const float nrm = sqrtf(sq_norm(x));
      if (nrm - t_xyz > 0.f && nrm > 0.f) d = (g[1] * inv / nrm) * x;
    }
    d_xyz[3 * i] = d.x; d_xyz[3 * i + 1] = d.y; d_xyz[3 * i + 2] = d.z;
  }
  if (d_scaling) {
    V3 d{0.f, 0.f, 0.f};
    if (vis) {
      const V3 e{expf(scaling[3 * i]), expf(scaling[3 * i + 1]), expf(scaling[3 * i + 2])};
      const V3 u{fmaxf(e.x - t_scale, 0.f), fmaxf(e.y - t_scale, 0.f), fmaxf(e.z - t_scale, 0.f)};
      const float nrm = sqrtf(sq_norm(u));
      if (nrm > 0.f) {
        const float c = g[2] * inv / nrm;  // a component at its relu has u = 0: zero slope
        d = V3{c * u.x * e.x, c * u.y * e.y, c * u.z * e.z};
      }
    }
    d_scaling[3 * i] = d.x; d_scaling[3 * i + 1] = d.y; d_scaling[3 * i + 2] = d.z;
  }
}

}  // namespace reg
