// raster_math.hpp -- the per-Gaussian and per-pixel math of the forward Gaussian rasteriser (raster.hip), the published
// 3D Gaussian splatting forward pass that the reference calls as diff_gauss.GaussianRasterizer
// (/root/reference/gaussian_renderer/__init__.py:14,36-103; the extension's source is not vendored there).  Plain C++ for
// the device and the host alike: tests/hostraster/ compiles it with g++ over the stand-in for <hip/hip_runtime.h>, the
// way tests/hostgeo/ compiles geo_math.hpp.  All arithmetic is fp32.
//
// Matrices are stored as the reference stores them (scene/cameras.py:26-39): world_view_transform is the TRANSPOSE of the
// world-to-camera matrix and full_proj_transform = world_view_transform . projection, both row-major [16], so a point
// multiplies from the left as a row vector: p' = (x, y, z, 1) . M.
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>

namespace rast {

constexpr int TILE = 16;              // pixels per tile edge
constexpr float NEAR_Z = 0.2f;        // view depths at or below this are culled
constexpr float LOW_PASS = 0.3f;      // added to the diagonal of the 2D covariance (one pixel of anti-aliasing)
constexpr float FRUSTUM_PAD = 1.3f;   // x/z and y/z are clamped to this many half-widths in the Jacobian
constexpr float ALPHA_MAX = 0.99f;
constexpr float ALPHA_MIN = 1.0f / 255.0f;
constexpr float T_MIN = 1e-4f;        // a pixel is finished before the Gaussian that would take T below this
constexpr float MAX_RADIUS = 1073741824.0f;  // 2^30: keeps the conversion to int defined whatever the covariance holds

struct V3 {
  float x, y, z;
};
struct V4 {
  float x, y, z, w;
};
struct Sym3 {  // xx xy xz yy yz zz: the order of cov3Ds_precomp
  float xx, xy, xz, yy, yz, zz;
};

// (x, y, z, 1) . M, first three components
__host__ __device__ __forceinline__ V3 xform43(const float *M, V3 p) {
  return V3{p.x * M[0] + p.y * M[4] + p.z * M[8] + M[12], p.x * M[1] + p.y * M[5] + p.z * M[9] + M[13],
            p.x * M[2] + p.y * M[6] + p.z * M[10] + M[14]};
}
__host__ __device__ __forceinline__ V4 xform44(const float *M, V3 p) {
  return V4{p.x * M[0] + p.y * M[4] + p.z * M[8] + M[12], p.x * M[1] + p.y * M[5] + p.z * M[9] + M[13],
            p.x * M[2] + p.y * M[6] + p.z * M[10] + M[14], p.x * M[3] + p.y * M[7] + p.z * M[11] + M[15]};
}

// Sigma3 = R S S^T R^T, R from the normalised quaternion (WXYZ), S = diag(mod * scale)
__host__ __device__ __forceinline__ Sym3 cov3d(V3 scale, float mod, V4 q_wxyz) {
  float n = sqrtf(q_wxyz.x * q_wxyz.x + q_wxyz.y * q_wxyz.y + q_wxyz.z * q_wxyz.z + q_wxyz.w * q_wxyz.w);
  float r = q_wxyz.x / n, x = q_wxyz.y / n, y = q_wxyz.z / n, z = q_wxyz.w / n;
  float R[3][3] = {{1.f - 2.f * (y * y + z * z), 2.f * (x * y - r * z), 2.f * (x * z + r * y)},
                   {2.f * (x * y + r * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z - r * x)},
                   {2.f * (x * z - r * y), 2.f * (y * z + r * x), 1.f - 2.f * (x * x + y * y)}};
  float s[3] = {mod * scale.x, mod * scale.y, mod * scale.z};
  float M[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) M[i][j] = R[i][j] * s[j];
  auto dot = [&](int a, int b) { return M[a][0] * M[b][0] + M[a][1] * M[b][1] + M[a][2] * M[b][2]; };
  return Sym3{dot(0, 0), dot(0, 1), dot(0, 2), dot(1, 1), dot(1, 2), dot(2, 2)};
}

struct Cov2 {
  float a, b, c;  // [[a, b], [b, c]]
};

// Sigma2 = J W Sigma3 W^T J^T + LOW_PASS I.  t = view position; W = rotation part of the view matrix (as a column-vector
// matrix W[j][i] = V[4 i + j]); J = perspective Jacobian at t with x/z, y/z clamped to +-FRUSTUM_PAD tanfov.
__host__ __device__ __forceinline__ Cov2 cov2d(V3 t, float fx, float fy, float tanfovx, float tanfovy, Sym3 S, const float *V) {
  float limx = FRUSTUM_PAD * tanfovx, limy = FRUSTUM_PAD * tanfovy;
  float tx = fminf(limx, fmaxf(-limx, t.x / t.z)) * t.z, ty = fminf(limy, fmaxf(-limy, t.y / t.z)) * t.z;
  float J[2][3] = {{fx / t.z, 0.f, -(fx * tx) / (t.z * t.z)}, {0.f, fy / t.z, -(fy * ty) / (t.z * t.z)}};
  float T[2][3];  // J W
  for (int r = 0; r < 2; ++r)
    for (int i = 0; i < 3; ++i) T[r][i] = J[r][0] * V[4 * i + 0] + J[r][1] * V[4 * i + 1] + J[r][2] * V[4 * i + 2];
  float C[3][3] = {{S.xx, S.xy, S.xz}, {S.xy, S.yy, S.yz}, {S.xz, S.yz, S.zz}};
  float TC[2][3];
  for (int r = 0; r < 2; ++r)
    for (int j = 0; j < 3; ++j) TC[r][j] = T[r][0] * C[0][j] + T[r][1] * C[1][j] + T[r][2] * C[2][j];
  auto dot = [&](int r, int s) { return TC[r][0] * T[s][0] + TC[r][1] * T[s][1] + TC[r][2] * T[s][2]; };
  return Cov2{dot(0, 0) + LOW_PASS, dot(0, 1), dot(1, 1) + LOW_PASS};
}

// clamp to [0, hi] in float first (NaN -> 0), so that the conversion to int is defined for every input
__host__ __device__ __forceinline__ int clamp_tile(float v, int hi) { return (int)fminf((float)hi, fmaxf(0.f, floorf(v))); }

struct Splat {
  float px, py;            // pixel centre
  float A, B, C;           // conic: power = -1/2 (A dx^2 + C dy^2) - B dx dy
  float depth;             // view z
  int radius;              // 0 = culled: nothing else is meaningful then
  int x0, y0, x1, y1;      // tile rectangle [x0, x1) x [y0, y1)
};

// Steps 1-7 for one Gaussian.  gx, gy = tiles per row / column.
__host__ __device__ __forceinline__ Splat project(V3 mean, Sym3 S, const float *view, const float *proj, int W, int H,
                                                  float tanfovx, float tanfovy, int gx, int gy) {
  Splat o{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0, 0, 0, 0, 0};
  V3 t = xform43(view, mean);
  if (!(t.z > NEAR_Z)) return o;  // also culls a NaN depth
  o.depth = t.z;
  float fx = (float)W / (2.f * tanfovx), fy = (float)H / (2.f * tanfovy);
  Cov2 c = cov2d(t, fx, fy, tanfovx, tanfovy, S, view);
  float det = c.a * c.c - c.b * c.b;
  if (!(det != 0.f) || det != det) return o;
  o.A = c.c / det; o.B = -c.b / det; o.C = c.a / det;
  float mid = 0.5f * (c.a + c.c);
  float lam = mid + sqrtf(fmaxf(0.1f, mid * mid - det));
  float radius = fminf(MAX_RADIUS, ceilf(3.f * sqrtf(lam)));
  V4 h = xform44(proj, mean);
  float w = h.w + 1e-7f;
  o.px = ((h.x / w + 1.f) * (float)W - 1.f) * 0.5f;
  o.py = ((h.y / w + 1.f) * (float)H - 1.f) * 0.5f;
  o.x0 = clamp_tile((o.px - radius) / TILE, gx); o.x1 = clamp_tile((o.px + radius + (TILE - 1)) / TILE, gx);
  o.y0 = clamp_tile((o.py - radius) / TILE, gy); o.y1 = clamp_tile((o.py + radius + (TILE - 1)) / TILE, gy);
  if (!(radius > 0.f) || o.x1 <= o.x0 || o.y1 <= o.y0) return o;  // NaN radius or empty rectangle: radius stays 0
  o.radius = (int)radius;
  return o;
}

// clamp_min(eval_sh(deg, sh, dir) + 0.5, 0) with the constants and signs of utils/sh_utils.py:26-100; sh = [n_coeffs][3]
// (coefficient-major, the layout of GaussianModel.get_features), dir = normalize(mean - campos).
__host__ __device__ __forceinline__ V3 sh_colour(int deg, const float *sh, V3 mean, V3 campos) {
  const float C0 = 0.28209479177387814f, C1 = 0.4886025119029199f;
  const float C2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f, -1.0925484305920792f, 0.5462742152960396f};
  const float C3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f, 0.3731763325901154f,
                       -0.4570457994644658f, 1.445305721320277f, -0.5900435899266435f};
  float dx = mean.x - campos.x, dy = mean.y - campos.y, dz = mean.z - campos.z;
  float len = sqrtf(dx * dx + dy * dy + dz * dz);
  float x = dx / len, y = dy / len, z = dz / len;
  float out[3];
  for (int c = 0; c < 3; ++c) {
    auto s = [&](int k) { return sh[3 * k + c]; };
    float r = C0 * s(0);
    if (deg > 0) {
      r = r - C1 * y * s(1) + C1 * z * s(2) - C1 * x * s(3);
      if (deg > 1) {
        float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
        r = r + C2[0] * xy * s(4) + C2[1] * yz * s(5) + C2[2] * (2.f * zz - xx - yy) * s(6) + C2[3] * xz * s(7) +
            C2[4] * (xx - yy) * s(8);
        if (deg > 2)
          r = r + C3[0] * y * (3.f * xx - yy) * s(9) + C3[1] * xy * z * s(10) + C3[2] * y * (4.f * zz - xx - yy) * s(11) +
              C3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy) * s(12) + C3[4] * x * (4.f * zz - xx - yy) * s(13) +
              C3[5] * z * (xx - yy) * s(14) + C3[6] * x * (xx - 3.f * yy) * s(15);
      }
    }
    out[c] = fmaxf(0.f, r + 0.5f);
  }
  return V3{out[0], out[1], out[2]};
}

struct Pixel {  // front-to-back state of one pixel
  float T, r, g, b;
};

// One Gaussian onto one pixel, steps 2-5 of the per-pixel loop.  (dx, dy) = Gaussian centre - pixel.  Returns true when
// the pixel is finished (nothing, this Gaussian included, is added any more).
__host__ __device__ __forceinline__ bool blend(Pixel &p, float dx, float dy, float A, float B, float C, float opacity, V3 colour) {
  float power = -0.5f * (A * dx * dx + C * dy * dy) - B * dx * dy;
  if (power > 0.f) return false;
  float alpha = fminf(ALPHA_MAX, opacity * expf(power));
  if (alpha < ALPHA_MIN) return false;
  float test_T = p.T * (1.f - alpha);
  if (test_T < T_MIN) return true;
  float w = alpha * p.T;
  p.r += colour.x * w; p.g += colour.y * w; p.b += colour.z * w;
  p.T = test_T;
  return false;
}

}  // namespace rast
