// image_loss_math.hpp -- the per-pixel statements of the image loss (/root/reference/utils/loss_utils.py:18-64 and
// utils/image_utils.py:17-19) whose numerics the tests pin: the 11-tap window, the SSIM map value from the five windowed
// moments, and the three partial derivatives its gradient is built from.  Plain C++ for the device and the host alike:
// tests/hostimage/ compiles it with g++ over the stand-in for <hip/hip_runtime.h>, the way tests/hostgeo/ compiles
// geo_math.hpp.
//
// THE GRADIENT.  With the zero-padded windowed moments at a map pixel p (w = the 2-D window, the outer product of window())
//   mu1 = sum w x,  mu2 = sum w y,  s1 = sum w x^2 - mu1^2,  s2 = sum w y^2 - mu2^2,  s12 = sum w x y - mu1 mu2,
//   A1 = 2 mu1 mu2 + C1,  A2 = 2 s12 + C2,  B1 = mu1^2 + mu2^2 + C1,  B2 = s1 + s2 + C2,  m = A1 A2 / (B1 B2)
// the map depends on the image x through mu1, s1 and s12 only:
//   dm/ds1  = -A1 A2 / (B1 B2^2)                                   (d_s1)
//   dm/ds12 = 2 A1 / (B1 B2)                                       (d_s12)
//   dm/dmu1 = 2 mu2 A2 / (B1 B2) - 2 mu1 A1 A2 / (B1^2 B2)         at fixed s1, s12; and in total, since s1 and s12 carry
//             -mu1^2 and -mu1 mu2:   d_mu = dm/dmu1 - 2 mu1 d_s1 - mu2 d_s12.
// A pixel q enters the moments of p with weight w(p - q): d mu1(p) / d x(q) = w, d (sum w x^2) / d x(q) = 2 x(q) w,
// d (sum w x y) / d x(q) = y(q) w.  Summed over the map pixels p (the maps are zero outside H x W, the window is symmetric):
//   d (sum_p m) / d x(q) = (w * d_mu)(q) + 2 x(q) (w * d_s1)(q) + y(q) (w * d_s12)(q),
// three more separable convolutions with the same window.  tests/test_image_loss_host.py anchors this against autograd of
// the reference's own function and against torch.autograd.gradcheck of a float64 twin.
//
// NUMERICS.  The reference forms the variances as E[x^2] - mu^2 in fp32, and so does point(): every product and difference
// there is rounded on its own (no FMA contraction), because the cancellation on flat regions is part of what the reference
// returns.  The window sums are written with explicit FMAs in one fixed order, so the host build and
// the kernels accumulate alike.
#pragma once
#include <hip/hip_runtime.h>

namespace imgloss {

constexpr int WIN = 11;              // loss_utils.py:34, the only size any caller uses
constexpr int RAD = WIN / 2;         // F.conv2d(padding = window_size // 2)
constexpr int TILE = 16;             // output pixels per workgroup side (the rasteriser's tile)
constexpr int HALO = TILE + 2 * RAD; // 26: the input rows and columns a tile's outputs read

// loss_utils.py:24-26: exp(-(i - 5)^2 / (2 * 1.5^2)), i = 0..10, over their sum; computed in float64 and rounded once
// (the reference normalises in fp32 and lands within 1 ulp of these).
__host__ __device__ __forceinline__ float window(int i) {
  constexpr float w[WIN] = {0.00102838008f, 0.00759875814f, 0.0360007721f, 0.10936069f, 0.213005538f, 0.266011725f,
                            0.213005538f,   0.10936069f,    0.0360007721f, 0.00759875814f, 0.00102838008f};
  return w[i];
}

// sum_k window(k) v[k * stride]: 11 taps, the first a product, the rest FMAs, in index order
__host__ __device__ __forceinline__ float taps(const float *v, int stride) {
  float acc = window(0) * v[0];
#pragma unroll
  for (int k = 1; k < WIN; ++k) acc = __builtin_fmaf(window(k), v[k * stride], acc);
  return acc;
}

struct Moments {  // the five zero-padded windowed sums at one map pixel
  float x, y, xx, yy, xy;
};

// the horizontal half of the five sums from 11 consecutive pixels of both images: the products are rounded first, as the
// reference's img1 * img1, img2 * img2 and img1 * img2 are before they reach F.conv2d (loss_utils.py:52-54)
__host__ __device__ __forceinline__ Moments row_moments(const float *x, const float *y) {
  Moments r;
  r.x = window(0) * x[0]; r.y = window(0) * y[0];
  r.xx = window(0) * (x[0] * x[0]); r.yy = window(0) * (y[0] * y[0]); r.xy = window(0) * (x[0] * y[0]);
#pragma unroll
  for (int k = 1; k < WIN; ++k) {
    float w = window(k), a = x[k], b = y[k];
    r.x = __builtin_fmaf(w, a, r.x); r.y = __builtin_fmaf(w, b, r.y);
    r.xx = __builtin_fmaf(w, a * a, r.xx); r.yy = __builtin_fmaf(w, b * b, r.yy); r.xy = __builtin_fmaf(w, a * b, r.xy);
  }
  return r;
}

struct Point {
  float m;                  // the SSIM map value, loss_utils.py:59
  float d_mu, d_s1, d_s12;  // the three partials above
};

// loss_utils.py:45-59 at one pixel, operation for operation in fp32
__host__ __device__ __forceinline__ Point point(const Moments &e) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float C1 = (float)(0.01 * 0.01), C2 = (float)(0.03 * 0.03);
  float mu1 = e.x, mu2 = e.y;
  float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
  float s1 = e.xx - mu1_sq, s2 = e.yy - mu2_sq, s12 = e.xy - mu1_mu2;
  float A1 = 2.0f * mu1_mu2 + C1, A2 = 2.0f * s12 + C2, B1 = mu1_sq + mu2_sq + C1, B2 = s1 + s2 + C2;
  float den = B1 * B2;
  Point p;
  p.m = (A1 * A2) / den;
  p.d_s1 = -p.m / B2;
  p.d_s12 = 2.0f * A1 / den;
  float d_mu1 = 2.0f * mu2 * A2 / den - 2.0f * mu1 * p.m / B1;
  p.d_mu = d_mu1 - 2.0f * mu1 * p.d_s1 - mu2 * p.d_s12;
  return p;
}

// d |d| / d d as torch's abs backward gives it: sign(0) = 0
__host__ __device__ __forceinline__ float sign(float d) { return d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f); }

// the pixel gradient of one plane's three means from the three convolved maps: c_* = (w * d_*)(q), inv_n = 1 / (H W)
__host__ __device__ __forceinline__ float pixel_grad(float x, float y, float c_mu, float c_s1, float c_s12, float g_l1, float g_mse,
                                                     float g_ssim, float inv_n) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float d = x - y;
  float ds = c_mu + 2.0f * x * c_s1 + y * c_s12;
  return (g_l1 * sign(d) + g_mse * 2.0f * d + g_ssim * ds) * inv_n;
}

}  // namespace imgloss
