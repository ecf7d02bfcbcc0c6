// raster_grad_math.hpp -- the backward pass of the Gaussian rasteriser: the exact derivative of the forward function as
// raster_math.hpp computes it, with every discrete decision held fixed (culling, radius and tile rectangle, depth order,
// power > 0, alpha < 1/255, the T < 1e-4 finish).  The three clamps differentiate as clamps, zero slope where they bind:
// alpha = min(0.99, .), the +-1.3 tanfov clamp of x/z and y/z inside the Jacobian, max(0, sh + 0.5).  Plain C++ for the
// device (raster_backward.hip) and the host (tests/hostraster_grad/) alike; all arithmetic is fp32.
//
// Per pixel, with the contributing entries k = 0 .. K-1 front to back, T_0 = 1, T_{k+1} = T_k (1 - alpha_k):
//   image_c = sum_k colour_kc alpha_k T_k + T_K bg_c,   alpha_out = 1 - T_K
// so with gi = dL/dimage, ga = dL/dalpha_out and behind_kc = sum_{j > k} colour_jc alpha_j T_j
//   dL/dcolour_kc = gi_c alpha_k T_k
//   dL/dalpha_k   = sum_c gi_c (colour_kc T_k - behind_kc / (1 - alpha_k)) - (gi . bg - ga) T_K / (1 - alpha_k)
// The walk goes back to front from the saved T_K and rebuilds T_k = T_{k+1} / (1 - alpha_k).
#pragma once
#include "raster_math.hpp"

namespace rast {

// One row of the per-entry buffer: d px, d py, d a, d b, d c, d opacity, d colour x 3, where [[a, b], [b, c]] is the 2D
// covariance (the inverse of the conic).  The conic's own partials would serve as well in exact arithmetic, but their
// sums over pixels are ill-conditioned for an elongated Gaussian: the map back to the covariance, -Q G Q with the
// near-singular conic Q, multiplies the large component of G by the square of the small eigenvalue, so the fp32 error of
// that component swamps the result (4e-5 relative on a committed scene, against 2e-6 for this form).  With u = Q d,
// d power / d Sigma2 = 1/2 u u^T is taken per pixel instead, where the product with Q is still exact to a rounding.
constexpr int N_PARTIALS = 9;

struct PixelBack {  // back-to-front state of one pixel
  float T;          // transmittance behind the entry visited last (starts as the saved final T)
  float r, g, b;    // colour accumulated behind it
};

// One Gaussian onto one pixel, backwards.  (dx, dy) = Gaussian centre - pixel; gi = dL/dimage of the pixel;
// gt = (gi . bg - dL/dalpha_out) * final T.  Applies the two skips of blend(); returns false (out untouched) when the
// entry contributed nothing.
__host__ __device__ __forceinline__ bool blend_backward(PixelBack &p, float dx, float dy, float A, float B, float C, float opacity,
                                                        V3 colour, V3 gi, float gt, float *out) {
  float power = -0.5f * (A * dx * dx + C * dy * dy) - B * dx * dy;
  if (power > 0.f) return false;
  float G = expf(power);
  float raw = opacity * G;
  float alpha = fminf(ALPHA_MAX, raw);
  if (alpha < ALPHA_MIN) return false;
  float om = 1.f - alpha;
  float Tk = p.T / om;
  float w = alpha * Tk;
  out[6] = gi.x * w; out[7] = gi.y * w; out[8] = gi.z * w;
  float dalpha = gi.x * (colour.x * Tk - p.r / om) + gi.y * (colour.y * Tk - p.g / om) + gi.z * (colour.z * Tk - p.b / om) - gt / om;
  p.r += colour.x * w; p.g += colour.y * w; p.b += colour.z * w;
  p.T = Tk;
  float dop = 0.f, dpow = 0.f;
  if (!(raw > ALPHA_MAX)) { dop = dalpha * G; dpow = dalpha * raw; }  // a bound clamp has zero slope
  float ux = A * dx + B * dy, uy = B * dx + C * dy;  // conic . d: power = -1/2 d . u
  out[0] = -dpow * ux;
  out[1] = -dpow * uy;
  out[2] = dpow * (0.5f * ux * ux);
  out[3] = dpow * (ux * uy);
  out[4] = dpow * (0.5f * uy * uy);
  out[5] = dop;
  return true;
}

// Backward of project() for a Gaussian that was not culled: from d px, d py and the 2D covariance's d a, d b, d c to d mean (two of
// its three paths: the projection and the Jacobian inside the 2D covariance) and d Sigma3 as the six values of
// cov3Ds_precomp, an off-diagonal one being the sum of both positions it fills.
__host__ __device__ __forceinline__ void project_backward(V3 mean, Sym3 S, const float *V, const float *P, int W, int H, float tanfovx,
                                                          float tanfovy, float dpx, float dpy, float da, float db, float dc,
                                                          V3 &dmean, Sym3 &dS) {
  V3 t = xform43(V, mean);
  float fx = (float)W / (2.f * tanfovx), fy = (float)H / (2.f * tanfovy);
  float limx = FRUSTUM_PAD * tanfovx, limy = FRUSTUM_PAD * tanfovy;
  float rx = t.x / t.z, ry = t.y / t.z;
  bool bx = rx < -limx || rx > limx, by = ry < -limy || ry > limy;  // the clamp binds
  float ux = fminf(limx, fmaxf(-limx, rx)), uy = fminf(limy, fmaxf(-limy, ry));
  float iz = 1.f / t.z, iz2 = iz * iz;
  float J00 = fx * iz, J02 = -(fx * ux) * iz, J11 = fy * iz, J12 = -(fy * uy) * iz;
  float T0[3], T1[3];
  for (int i = 0; i < 3; ++i) {
    T0[i] = J00 * V[4 * i + 0] + J02 * V[4 * i + 2];
    T1[i] = J11 * V[4 * i + 1] + J12 * V[4 * i + 2];
  }
  float C3[3][3] = {{S.xx, S.xy, S.xz}, {S.xy, S.yy, S.yz}, {S.xz, S.yz, S.zz}};
  float ST0[3], ST1[3];
  for (int i = 0; i < 3; ++i) {
    ST0[i] = C3[i][0] * T0[0] + C3[i][1] * T0[1] + C3[i][2] * T0[2];
    ST1[i] = C3[i][0] * T1[0] + C3[i][1] * T1[1] + C3[i][2] * T1[2];
  }
  // a = T0 S T0, b = T0 S T1, c = T1 S T1
  auto g = [&](int i, int j) { return da * T0[i] * T0[j] + db * T0[i] * T1[j] + dc * T1[i] * T1[j]; };
  dS = Sym3{g(0, 0), g(0, 1) + g(1, 0), g(0, 2) + g(2, 0), g(1, 1), g(1, 2) + g(2, 1), g(2, 2)};
  float dT0[3], dT1[3];
  for (int i = 0; i < 3; ++i) {
    dT0[i] = 2.f * da * ST0[i] + db * ST1[i];
    dT1[i] = 2.f * dc * ST1[i] + db * ST0[i];
  }
  float dJ00 = dT0[0] * V[0] + dT0[1] * V[4] + dT0[2] * V[8];
  float dJ02 = dT0[0] * V[2] + dT0[1] * V[6] + dT0[2] * V[10];
  float dJ11 = dT1[0] * V[1] + dT1[1] * V[5] + dT1[2] * V[9];
  float dJ12 = dT1[0] * V[2] + dT1[1] * V[6] + dT1[2] * V[10];
  // J02 = -fx x / z^2 where the clamp is free, -fx u / z where it binds (u constant)
  float dtx = bx ? 0.f : -dJ02 * fx * iz2;
  float dty = by ? 0.f : -dJ12 * fy * iz2;
  float dtz = -dJ00 * fx * iz2 - dJ11 * fy * iz2 + dJ02 * (bx ? fx * ux * iz2 : 2.f * fx * t.x * iz2 * iz) +
              dJ12 * (by ? fy * uy * iz2 : 2.f * fy * t.y * iz2 * iz);
  // pixel centre: px = ((h.x / w + 1) W - 1) / 2
  V4 h = xform44(P, mean);
  float w = h.w + 1e-7f, iw = 1.f / w;
  float dhx = dpx * (0.5f * (float)W) * iw, dhy = dpy * (0.5f * (float)H) * iw;
  float dhw = -(dpx * (0.5f * (float)W) * h.x + dpy * (0.5f * (float)H) * h.y) * iw * iw;
  dmean.x = dtx * V[0] + dty * V[1] + dtz * V[2] + dhx * P[0] + dhy * P[1] + dhw * P[3];
  dmean.y = dtx * V[4] + dty * V[5] + dtz * V[6] + dhx * P[4] + dhy * P[5] + dhw * P[7];
  dmean.z = dtx * V[8] + dty * V[9] + dtz * V[10] + dhx * P[8] + dhy * P[9] + dhw * P[11];
}

// Backward of cov3d(): d Sigma3 (six values, off-diagonal = sum of both positions) to d scale and d quaternion, the latter
// through the normalisation cov3d() applies.
__host__ __device__ __forceinline__ void cov3d_backward(V3 scale, float mod, V4 q_wxyz, Sym3 dS, V3 &dscale, V4 &dq) {
  float n = sqrtf(q_wxyz.x * q_wxyz.x + q_wxyz.y * q_wxyz.y + q_wxyz.z * q_wxyz.z + q_wxyz.w * q_wxyz.w);
  float r = q_wxyz.x / n, x = q_wxyz.y / n, y = q_wxyz.z / n, z = q_wxyz.w / n;
  float R[3][3] = {{1.f - 2.f * (y * y + z * z), 2.f * (x * y - r * z), 2.f * (x * z + r * y)},
                   {2.f * (x * y + r * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z - r * x)},
                   {2.f * (x * z - r * y), 2.f * (y * z + r * x), 1.f - 2.f * (x * x + y * y)}};
  float s[3] = {mod * scale.x, mod * scale.y, mod * scale.z};
  // Sigma = M M^T, M = R diag(s): dM = (G + G^T) M with G + G^T = [[2 xx, xy, xz], [xy, 2 yy, yz], [xz, yz, 2 zz]] of dS
  float Gs[3][3] = {{2.f * dS.xx, dS.xy, dS.xz}, {dS.xy, 2.f * dS.yy, dS.yz}, {dS.xz, dS.yz, 2.f * dS.zz}};
  float dR[3][3], ds[3] = {0.f, 0.f, 0.f};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      float dM = (Gs[i][0] * R[0][j] + Gs[i][1] * R[1][j] + Gs[i][2] * R[2][j]) * s[j];
      ds[j] += dM * R[i][j];
      dR[i][j] = dM * s[j];
    }
  dscale = V3{mod * ds[0], mod * ds[1], mod * ds[2]};
  float dr = 2.f * (-z * dR[0][1] + y * dR[0][2] + z * dR[1][0] - x * dR[1][2] - y * dR[2][0] + x * dR[2][1]);
  float dx = 2.f * (y * dR[0][1] + z * dR[0][2] + y * dR[1][0] - 2.f * x * dR[1][1] - r * dR[1][2] + z * dR[2][0] + r * dR[2][1] -
                    2.f * x * dR[2][2]);
  float dy = 2.f * (-2.f * y * dR[0][0] + x * dR[0][1] + r * dR[0][2] + x * dR[1][0] + z * dR[1][2] - r * dR[2][0] + z * dR[2][1] -
                    2.f * y * dR[2][2]);
  float dz = 2.f * (-2.f * z * dR[0][0] - r * dR[0][1] + x * dR[0][2] + r * dR[1][0] - 2.f * z * dR[1][1] + y * dR[1][2] + x * dR[2][0] +
                    y * dR[2][1]);
  float along = r * dr + x * dx + y * dy + z * dz;  // the normalisation removes the radial part
  dq = V4{(dr - r * along) / n, (dx - x * along) / n, (dy - y * along) / n, (dz - z * along) / n};
}

// Backward of sh_colour(): d colour to d sh [n_coeffs][3] (every coefficient is written, zero above the degree and where
// max(0, .) binds) and the third path into d mean, through the normalised view direction (added to dmean).
__host__ __device__ __forceinline__ void sh_backward(int deg, const float *sh, int n_coeffs, V3 mean, V3 campos, V3 dcol, float *dsh,
                                                     V3 &dmean) {
  const float C0 = 0.28209479177387814f, C1 = 0.4886025119029199f;
  const float C2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f, -1.0925484305920792f, 0.5462742152960396f};
  const float C3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f, 0.3731763325901154f,
                       -0.4570457994644658f, 1.445305721320277f, -0.5900435899266435f};
  float ex = mean.x - campos.x, ey = mean.y - campos.y, ez = mean.z - campos.z;
  float len = sqrtf(ex * ex + ey * ey + ez * ez);
  float x = ex / len, y = ey / len, z = ez / len;
  float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
  // basis and its derivatives along x, y, z
  float b[16], bx[16], by[16], bz[16];
  for (int k = 0; k < 16; ++k) b[k] = bx[k] = by[k] = bz[k] = 0.f;
  b[0] = C0;
  b[1] = -C1 * y; by[1] = -C1;
  b[2] = C1 * z; bz[2] = C1;
  b[3] = -C1 * x; bx[3] = -C1;
  b[4] = C2[0] * xy; bx[4] = C2[0] * y; by[4] = C2[0] * x;
  b[5] = C2[1] * yz; by[5] = C2[1] * z; bz[5] = C2[1] * y;
  b[6] = C2[2] * (2.f * zz - xx - yy); bx[6] = -2.f * C2[2] * x; by[6] = -2.f * C2[2] * y; bz[6] = 4.f * C2[2] * z;
  b[7] = C2[3] * xz; bx[7] = C2[3] * z; bz[7] = C2[3] * x;
  b[8] = C2[4] * (xx - yy); bx[8] = 2.f * C2[4] * x; by[8] = -2.f * C2[4] * y;
  b[9] = C3[0] * y * (3.f * xx - yy); bx[9] = C3[0] * 6.f * xy; by[9] = C3[0] * (3.f * xx - 3.f * yy);
  b[10] = C3[1] * xy * z; bx[10] = C3[1] * yz; by[10] = C3[1] * xz; bz[10] = C3[1] * xy;
  b[11] = C3[2] * y * (4.f * zz - xx - yy); bx[11] = -2.f * C3[2] * xy; by[11] = C3[2] * (4.f * zz - xx - 3.f * yy); bz[11] = 8.f * C3[2] * yz;
  b[12] = C3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy); bx[12] = -6.f * C3[3] * xz; by[12] = -6.f * C3[3] * yz;
  bz[12] = C3[3] * (6.f * zz - 3.f * xx - 3.f * yy);
  b[13] = C3[4] * x * (4.f * zz - xx - yy); bx[13] = C3[4] * (4.f * zz - 3.f * xx - yy); by[13] = -2.f * C3[4] * xy; bz[13] = 8.f * C3[4] * xz;
  b[14] = C3[5] * z * (xx - yy); bx[14] = 2.f * C3[5] * xz; by[14] = -2.f * C3[5] * yz; bz[14] = C3[5] * (xx - yy);
  b[15] = C3[6] * x * (xx - 3.f * yy); bx[15] = C3[6] * (3.f * xx - 3.f * yy); by[15] = -6.f * C3[6] * xy;
  const int used = (deg + 1) * (deg + 1);
  const float dc[3] = {dcol.x, dcol.y, dcol.z};
  float gx = 0.f, gy = 0.f, gz = 0.f;
  for (int c = 0; c < 3; ++c) {
    float r = 0.f;
    for (int k = 0; k < used; ++k) r += b[k] * sh[3 * k + c];
    float dr = r + 0.5f > 0.f ? dc[c] : 0.f;
    for (int k = 0; k < n_coeffs; ++k) dsh[3 * k + c] = k < used ? dr * b[k] : 0.f;
    for (int k = 1; k < used; ++k) {
      float v = dr * sh[3 * k + c];
      gx += v * bx[k]; gy += v * by[k]; gz += v * bz[k];
    }
  }
  float along = x * gx + y * gy + z * gz;
  dmean.x += (gx - x * along) / len; dmean.y += (gy - y * along) / len; dmean.z += (gz - z * along) / len;
}

}  // namespace rast
