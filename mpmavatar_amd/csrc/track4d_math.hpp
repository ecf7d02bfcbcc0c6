// track4d_math.hpp -- the two terms of the 4D-DRESS tracking script (preprocess/train_mesh_lbs_4ddress.py) that the ActorsHQ one does
// not have, per work item:
//   losses['laplacian'] (:363, the matrix of :212-214) as a gather over the vertex adjacency instead of a dense [V, V] product
//     (Lv)_i = (sum_{j in N(i)} v_j) / deg(i) - v_i,  -v_i for a vertex in no face;  laplacian = mean_i |(Lv)_i|
//     N(i) in ascending j; the sum is DIVIDED by the degree (a correctly rounded fp32 division), so a vertex whose neighbours sum to
//     exactly deg * v_i gives exactly zero.  pytorch3d stores 1 / deg in the matrix; the difference is at rounding level.
//     This restates pytorch3d's uniform laplacian(verts, edges_packed) and is UNCONFIRMED against pytorch3d itself.
//     backward: u_i = (g / V) (Lv)_i / |(Lv)_i| (0 where the norm is 0, torch's subgradient of norm), d v_j = sum_{i in N(j)} u_i / deg(i) - u_j:
//     a gather over the same table, which is symmetric although L is not.
//   scale_ratio_loss (:279-292, used at :361), per face with v = verts[faces[f]] and s = scale[f]:
//     m = max_k |v_k - v_{(k + 1) mod 3}|,  a = max(s0, s1),  b = min(s0, s1),  r = a / (b + 1e-8),  q = a / (m + 1e-8)
//     scale_ratio = mean(max(r, th_r) - th_r),  scale_edge_ratio = mean(max(q, th_e) - th_e),  scale_edge_ratio_var = var(q) (F - 1)
//     and the exact derivative with every discrete decision held fixed as torch decides it on the CPU: the first of equal maxima
//     (edges and scales), the first of equal minima, clamp's slope 1 at x == th, zero gradient through a zero-length longest edge.
// Plain C++ for the device (track4d.hip) and the host (tests/hosttrack4d/) alike.  All arithmetic is fp32; the sums over vertices and
// faces are the caller's (double, fixed order).  An index outside its range reads nothing and gives NaN.
#pragma once
#include "track_math.hpp"

namespace trk4 {

using trk::V3;
using trk::ld3;
using trk::st3;

constexpr float RATIO_EPS = 1e-8f;

// ---- the uniform Laplacian ---------------------------------------------------------------------------------------------------------

// row i of Lv and its norm.  start [n_verts + 1], nbr [start[n_verts]] ascending within a row.
__host__ __device__ __forceinline__ V3 laplacian_row(int64_t i, int32_t n_verts, const float *verts, const int32_t *start, const int32_t *nbr,
                                                     float &norm) {
#pragma clang fp contract(off)
  const int32_t lo = start[i], hi = start[i + 1];
  V3 s{0.f, 0.f, 0.f};
  for (int32_t k = lo; k < hi; ++k) {
    const int32_t j = nbr[k];
    const V3 p = j >= 0 && j < n_verts ? ld3(verts, j) : trk::nan3();
    s.x += p.x; s.y += p.y; s.z += p.z;
  }
  const V3 v = ld3(verts, i);
  V3 l{-v.x, -v.y, -v.z};
  if (hi > lo) {
    const float deg = (float)(hi - lo);
    l = V3{s.x / deg - v.x, s.y / deg - v.y, s.z / deg - v.z};
  }
  norm = sqrtf(l.x * l.x + l.y * l.y + l.z * l.z);
  return l;
}

// u_i / c from the saved row i of Lv: scale * (Lv)_i / (|(Lv)_i| c), zero where the norm is zero
__host__ __device__ __forceinline__ V3 laplacian_unit(const float *lv, int64_t i, float scale, float c) {
#pragma clang fp contract(off)
  const V3 l = ld3(lv, i);
  const float norm = sqrtf(l.x * l.x + l.y * l.y + l.z * l.z);
  if (norm == 0.f) return V3{0.f, 0.f, 0.f};
  return V3{scale * l.x / norm / c, scale * l.y / norm / c, scale * l.z / norm / c};
}

// d vertices[j] from the saved Lv, the table and the upstream scalar g[0]
__host__ __device__ __forceinline__ void laplacian_backward(int64_t j, int32_t n_verts, const float *lv, const int32_t *start,
                                                            const int32_t *nbr, const float *g, float *d_verts) {
#pragma clang fp contract(off)
  const float scale = g[0] / (float)n_verts;
  V3 s{0.f, 0.f, 0.f};
  for (int32_t k = start[j]; k < start[j + 1]; ++k) {
    const int32_t i = nbr[k];
    V3 u = trk::nan3();
    if (i >= 0 && i < n_verts) {
      const int32_t deg = start[i + 1] - start[i];      // >= 1: j is among them
      u = laplacian_unit(lv, i, scale, (float)(deg > 0 ? deg : 1));
    }
    s.x += u.x; s.y += u.y; s.z += u.z;
  }
  const V3 own = laplacian_unit(lv, j, scale, 1.f);
  st3(d_verts, j, V3{s.x - own.x, s.y - own.y, s.z - own.z});
}

// ---- scale_ratio_loss ----------------------------------------------------------------------------------------------------------------

struct ScaleFace {
  V3 e;                    // the longest edge v_k - v_{k + 1}, the first of the longest
  float m;                 // its length
  float den_r, den_q;      // b + 1e-8, m + 1e-8
  float r, q;
  int longest, ia, ib;     // which edge, which of s0 and s1 is the maximum, which the minimum
};

// No FMA contraction in what the decisions are taken on: the forward and the backward kernel see the same bits.
__host__ __device__ __forceinline__ ScaleFace scale_face(int64_t f, int32_t n_verts, const float *verts, const int32_t *faces,
                                                         const float *scales) {
#pragma clang fp contract(off)
  V3 v[3];
  trk::corners(verts, n_verts, faces, f, v);
  ScaleFace t;
  V3 e[3];
  float len[3];
  for (int k = 0; k < 3; ++k) {
    e[k] = trk::sub(v[k], v[(k + 1) % 3]);
    len[k] = sqrtf(e[k].x * e[k].x + e[k].y * e[k].y + e[k].z * e[k].z);
  }
  t.longest = 0;
  if (len[1] > len[t.longest]) t.longest = 1;
  if (len[2] > len[t.longest]) t.longest = 2;
  t.e = e[t.longest];
  t.m = len[t.longest];
  const float s0 = scales[3 * f], s1 = scales[3 * f + 1];
  t.ia = s1 > s0 ? 1 : 0;
  t.ib = s1 < s0 ? 1 : 0;
  const float a = t.ia ? s1 : s0, b = t.ib ? s1 : s0;
  t.den_r = b + RATIO_EPS;
  t.den_q = t.m + RATIO_EPS;
  t.r = a / t.den_r;
  t.q = a / t.den_q;
  return t;
}

struct ScaleTerms {
  float ratio, edge, q;    // face f's summands of the two hinges, and q itself for the variance
};

__host__ __device__ __forceinline__ ScaleTerms scale_terms_forward(int64_t f, int32_t n_verts, const float *verts, const int32_t *faces,
                                                                   const float *scales, float th_ratio, float th_edge) {
  const ScaleFace t = scale_face(f, n_verts, verts, faces, scales);
  // clamp(min = th) - th; a NaN stays a NaN
  const float hr = t.r >= th_ratio ? t.r - th_ratio : (t.r == t.r ? 0.f : t.r);
  const float hq = t.q >= th_edge ? t.q - th_edge : (t.q == t.q ? 0.f : t.q);
  return ScaleTerms{hr, hq, t.q};
}

// Row f of the backward.  g [3]: upstream of the three terms; an entry that is exactly zero leaves no trace (the variance of a single
// face is 0 / 0, which only a non-zero g[2] hands on).  mean_q: terms[3] of the forward.  d_stencil[f, c, :] and d_scales[f, :] are
// written in full where wanted; d_scales[f, 2] is exactly zero.
__host__ __device__ __forceinline__ void scale_terms_backward(int64_t f, int32_t n_faces, int32_t n_verts, const float *verts,
                                                              const int32_t *faces, const float *scales, float th_ratio, float th_edge,
                                                              float mean_q, const float *g, float *d_stencil, float *d_scales) {
#pragma clang fp contract(off)
  const ScaleFace t = scale_face(f, n_verts, verts, faces, scales);
  const float n = (float)n_faces;
  const float dr = t.r >= th_ratio ? g[0] / n : (t.r == t.r ? 0.f : t.r);
  float dq = t.q >= th_edge ? g[1] / n : (t.q == t.q ? 0.f : t.q);
  if (g[2] != 0.f) dq += g[2] * (2.f * (t.q - mean_q) / (n - 1.f));
  if (d_scales) {
    float ds[3] = {0.f, 0.f, 0.f};
    ds[t.ia] += dr / t.den_r + dq / t.den_q;
    ds[t.ib] += -(dr * t.r) / t.den_r;
    for (int k = 0; k < 3; ++k) d_scales[3 * f + k] = ds[k];
  }
  if (d_stencil) {
    const float dm = -(dq * t.q) / t.den_q;
    V3 out[3] = {V3{0.f, 0.f, 0.f}, V3{0.f, 0.f, 0.f}, V3{0.f, 0.f, 0.f}};
    if (t.m != 0.f) {                                   // torch's subgradient of norm at zero
      const V3 d{dm * t.e.x / t.m, dm * t.e.y / t.m, dm * t.e.z / t.m};
      out[t.longest] = d;
      out[(t.longest + 1) % 3] = V3{-d.x, -d.y, -d.z};
    }
    for (int c = 0; c < 3; ++c) st3(d_stencil, 3 * f + c, out[c]);
  }
}

}  // namespace trk4
