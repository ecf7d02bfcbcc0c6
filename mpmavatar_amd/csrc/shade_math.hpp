// shade_math.hpp -- the colours handed to the render call of the appearance loop (train_appearance.py:120-123):
//   colors[i] = shadow[binding[i]] * clamp_min(eval_sh(deg, features[i], normalize(means3D[i] - campos)) + 0.5, 0)
// with shadow[f] = grid_sample(shadow_map, uv[f], bilinear, align_corners = False, zeros padding), and the exact derivative
// of that expression with every discrete decision held fixed: the bilinear cell, a tap outside the map, and the SH clamp, which
// passes zero slope where it binds (rast::sh_backward's own `> 0` test).  The SH arithmetic is rast::sh_colour / rast::sh_backward;
// what is added here is the sampler, the product and the two reductions into the shadow map.  Plain C++ for the device (shade.hip)
// and the host (tests/hostshade/) alike: one function per work item, so the kernels and the host loops are the same statements.
// All arithmetic is fp32.
//
// Backward, with g = dL/dcolors[i], s = shadow of the Gaussian's face, c = its clamped SH colour:
//   1. per Gaussian   d features, d means3D = sh_backward(s g);  ds[i] = g . c
//   2. per face       dS[f] = sum ds[i] over the face's Gaussians in ascending Gaussian index
//   3. per texel      d map[t] = sum w dS[f] over the texel's taps in ascending (4 face + corner)
// No floating-point atomics: the sums of 2 and 3 are serial walks of a CSR segment, so two runs give the same bits.
#pragma once
#include "raster_grad_math.hpp"
#include "raster_math.hpp"

#include <math.h>
#include <stdint.h>

namespace shade {

using rast::V3;

constexpr int MAX_COEFFS = 16;  // degree 3

// torch's grid_sample rule for one location (u, v) in [-1, 1]^2 of an H x W map: bilinear, align_corners = False, zeros padding.
// idx[k] = y * W + x of the tap, -1 for a tap outside the map (it contributes nothing and receives nothing); w[k] = its weight.
// k = 0 .. 3: north-west, north-east, south-west, south-east, torch's own order.  The forward and the backward pass both call
// this function, so their weights carry the same bits.  No FMA contraction here: the cell is then the one that the same fp32
// operations give anywhere else, which is what lets the texel -> tap table be built outside this code (shading.ShadowSampler).
__host__ __device__ __forceinline__ void shadow_taps(float u, float v, int H, int W, int32_t idx[4], float w[4]) {
#pragma clang fp contract(off)
  float ix = ((u + 1.f) * (float)W - 1.f) / 2.f, iy = ((v + 1.f) * (float)H - 1.f) / 2.f;
  float x0 = floorf(ix), y0 = floorf(iy), x1 = x0 + 1.f, y1 = y0 + 1.f;
  w[0] = (x1 - ix) * (y1 - iy);
  w[1] = (ix - x0) * (y1 - iy);
  w[2] = (x1 - ix) * (iy - y0);
  w[3] = (ix - x0) * (iy - y0);
  // decided on the floats: a location far outside (or a NaN) never becomes an integer
  bool in_x0 = x0 >= 0.f && x0 <= (float)(W - 1), in_x1 = x1 >= 0.f && x1 <= (float)(W - 1);
  bool in_y0 = y0 >= 0.f && y0 <= (float)(H - 1), in_y1 = y1 >= 0.f && y1 <= (float)(H - 1);
  idx[0] = in_x0 && in_y0 ? (int32_t)y0 * W + (int32_t)x0 : -1;
  idx[1] = in_x1 && in_y0 ? (int32_t)y0 * W + (int32_t)x1 : -1;
  idx[2] = in_x0 && in_y1 ? (int32_t)y1 * W + (int32_t)x0 : -1;
  idx[3] = in_x1 && in_y1 ? (int32_t)y1 * W + (int32_t)x1 : -1;
}

// shadow of face f: sum of the taps inside the map, in torch's order.  A binding entry outside [0, n_faces) reads nothing and
// gives NaN: loud in the image, and no access out of bounds.
__host__ __device__ __forceinline__ float sample_shadow(const float *map, int H, int W, const float *face_uv, int32_t n_faces, int32_t f) {
  if (f < 0 || f >= n_faces) return NAN;
  int32_t idx[4];
  float w[4];
  shadow_taps(face_uv[2 * (int64_t)f], face_uv[2 * (int64_t)f + 1], H, W, idx, w);
  float s = 0.f;
  for (int k = 0; k < 4; ++k)
    if (idx[k] >= 0) s += map[idx[k]] * w[k];
  return s;
}

// the (deg + 1)^2 coefficients in use of Gaussian i, coefficient-major [k][3], from features_dc [n, 1, 3] and features_rest
// [n, n_coeffs - 1, 3]: no cat; the rows above the active degree are not read
__host__ __device__ __forceinline__ void load_coeffs(int deg, int n_coeffs, const float *dc, const float *rest, int64_t i, float *sh) {
  const int used = (deg + 1) * (deg + 1);
  for (int c = 0; c < 3; ++c) sh[c] = dc[3 * i + c];
  const float *row = rest + 3 * i * (int64_t)(n_coeffs - 1);
  for (int j = 0; j < 3 * (used - 1); ++j) sh[3 + j] = row[j];
}

// colors[i].  map == nullptr: shadow = 1 (plain convert_SH); dc == nullptr: the colour before the shadow is (1, 1, 1).
__host__ __device__ __forceinline__ void forward(int64_t i, int32_t n_faces, const int32_t *binding, const float *means3D, const float *campos, int deg,
                                                 int n_coeffs, const float *dc, const float *rest, const float *map, int H, int W,
                                                 const float *face_uv, float *colors) {
  float s = map ? sample_shadow(map, H, W, face_uv, n_faces, binding[i]) : 1.f;
  V3 c{1.f, 1.f, 1.f};
  if (dc) {
    float sh[3 * MAX_COEFFS];
    load_coeffs(deg, n_coeffs, dc, rest, i, sh);
    c = rast::sh_colour(deg, sh, V3{means3D[3 * i], means3D[3 * i + 1], means3D[3 * i + 2]}, V3{campos[0], campos[1], campos[2]});
  }
  colors[3 * i] = s * c.x; colors[3 * i + 1] = s * c.y; colors[3 * i + 2] = s * c.z;
}

// Stage 1 for Gaussian i.  g_colors == nullptr counts as zero.  d_dc [n, 1, 3], d_rest [n, n_coeffs - 1, 3] (zero above the active
// degree), d_means3D [n, 3], ds [n]: each written in full where given.
__host__ __device__ __forceinline__ void backward_gaussian(int64_t i, int32_t n_faces, const int32_t *binding, const float *means3D, const float *campos,
                                                           int deg, int n_coeffs, const float *dc, const float *rest, const float *map,
                                                           int H, int W, const float *face_uv, const float *g_colors, float *d_dc,
                                                           float *d_rest, float *d_means3D, float *ds) {
  V3 g{0.f, 0.f, 0.f};
  if (g_colors) g = V3{g_colors[3 * i], g_colors[3 * i + 1], g_colors[3 * i + 2]};
  const int used = (deg + 1) * (deg + 1);
  V3 c{1.f, 1.f, 1.f}, dmean{0.f, 0.f, 0.f};
  float dsh[3 * MAX_COEFFS];
  for (int j = 0; j < 3 * MAX_COEFFS; ++j) dsh[j] = 0.f;
  if (dc) {
    float s = map ? sample_shadow(map, H, W, face_uv, n_faces, binding[i]) : 1.f;
    float sh[3 * MAX_COEFFS];
    load_coeffs(deg, n_coeffs, dc, rest, i, sh);
    V3 mean{means3D[3 * i], means3D[3 * i + 1], means3D[3 * i + 2]}, cam{campos[0], campos[1], campos[2]};
    if (ds) c = rast::sh_colour(deg, sh, mean, cam);
    if (d_dc || d_rest || d_means3D) rast::sh_backward(deg, sh, used, mean, cam, V3{s * g.x, s * g.y, s * g.z}, dsh, dmean);
  }
  if (d_dc)
    for (int c3 = 0; c3 < 3; ++c3) d_dc[3 * i + c3] = dsh[c3];
  if (d_rest) {
    float *row = d_rest + 3 * i * (int64_t)(n_coeffs - 1);
    for (int j = 0; j < 3 * (used - 1); ++j) row[j] = dsh[3 + j];
    for (int j = 3 * (used - 1); j < 3 * (n_coeffs - 1); ++j) row[j] = 0.f;
  }
  if (d_means3D) { d_means3D[3 * i] = dmean.x; d_means3D[3 * i + 1] = dmean.y; d_means3D[3 * i + 2] = dmean.z; }
  if (ds) ds[i] = g.x * c.x + g.y * c.y + g.z * c.z;
}

// Stage 2 for face f: the sum of ds over the face's Gaussians, ascending
__host__ __device__ __forceinline__ void face_sum(int32_t f, const int32_t *face_start, const int32_t *face_items, const float *ds, float *dS) {
  float a = 0.f;
  for (int32_t j = face_start[f]; j < face_start[f + 1]; ++j) a += ds[face_items[j]];
  dS[f] = a;
}

// Stage 3 for texel t: texel_items holds 4 face + corner of every tap that lands on t, ascending
__host__ __device__ __forceinline__ void texel_sum(int32_t t, const int32_t *texel_start, const int32_t *texel_items, int H, int W,
                                                   const float *face_uv, const float *dS, float *d_map) {
  float a = 0.f;
  for (int32_t j = texel_start[t]; j < texel_start[t + 1]; ++j) {
    int32_t f = texel_items[j] >> 2, k = texel_items[j] & 3;
    int32_t idx[4];
    float w[4];
    shadow_taps(face_uv[2 * (int64_t)f], face_uv[2 * (int64_t)f + 1], H, W, idx, w);
    a += w[k] * dS[f];
  }
  d_map[t] = a;
}

}  // namespace shade
