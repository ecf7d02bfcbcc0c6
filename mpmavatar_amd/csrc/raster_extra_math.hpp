// raster_extra_math.hpp -- extra attribute channels blended by the Gaussian rasteriser: what the reference's 4D-DRESS tracking
// script hands over as extra_attrs (preprocess/train_mesh_lbs_4ddress.py:260-277, the [N, 2] garment labelling), reads back as
// the sixth slot of the render call (:299) and compares with the data's garment mask (:306).  Plain C++ for the device
// (raster_extra.hip) and the host (tests/hostraster_extra/) alike; all arithmetic is fp32.
//
// Per pixel, with the contributing entries k = 0 .. K-1 front to back and alpha_k, T_k and the finishing rule of blend()
// exactly as for the colour:
//   extra_e = sum_k a_ke alpha_k T_k        e = 0 .. E-1, no background term
// which is the colour formula of raster_grad_math.hpp with bg = 0.  UNCONFIRMED: the source of diff_gauss is not
// at hand; "no background, the colour's termination" is this project's definition.  With gx = dL/dextra and
// behind_ke = sum_{j > k} a_je alpha_j T_j
//   dL/da_ke = gx_e alpha_k T_k
//   dL/dalpha_k gets sum_e gx_e (a_ke T_k - behind_ke / (1 - alpha_k))
// and the partials to px, py, the 2D covariance and the opacity are linear in dL/dalpha_k, so the extras' share adds to that
// of image and alpha.  The operations stand in the order of blend() / blend_backward(): three channels blended here have the
// bits of three colours over a zero background.
#pragma once
#include "raster_grad_math.hpp"

namespace rast {

constexpr int EXTRA_MAX = 8;      // channels per call: 1 <= E <= EXTRA_MAX
constexpr int N_GEOM = 6;         // the leading partials of a row: d px, d py, d a, d b, d c, d opacity

// One Gaussian onto one pixel, forwards.  T = the transmittance in front of it, acc[E] = the pixel's extras so far, a[E] = the
// Gaussian's attributes.  Applies the two skips of blend().  There is no finishing test: the walk ends at the entry at which the
// colour walk of the same frame ended (pix_stop), which it recorded and this one does not derive again.
template <int E>
__host__ __device__ __forceinline__ void blend_extra(float &T, float *acc, float dx, float dy, float A, float B, float C, float opacity,
                                                     const float *a) {
  float power = -0.5f * (A * dx * dx + C * dy * dy) - B * dx * dy;
  if (power > 0.f) return;
  float alpha = fminf(ALPHA_MAX, opacity * expf(power));
  if (alpha < ALPHA_MIN) return;
  float test_T = T * (1.f - alpha);
  float w = alpha * T;
  for (int e = 0; e < E; ++e) acc[e] += a[e] * w;
  T = test_T;
}

template <int E>
struct PixelBackExtra {  // back-to-front state of one pixel
  float T;               // transmittance behind the entry visited last (starts as the saved final T)
  float behind[E];       // extras accumulated behind it
};

// One Gaussian onto one pixel, backwards.  gx[E] = dL/dextra of the pixel.  geom[N_GEOM] = the extras' share of the six
// geometry / opacity partials of a row (raster_grad_math.hpp), attr[E] = dL/da of this entry from this pixel.  Applies the
// two skips of blend(); returns false (outputs untouched) when the entry contributed nothing.
template <int E>
__host__ __device__ __forceinline__ bool blend_extra_backward(PixelBackExtra<E> &p, float dx, float dy, float A, float B, float C,
                                                              float opacity, const float *a, const float *gx, float *geom, float *attr) {
  float power = -0.5f * (A * dx * dx + C * dy * dy) - B * dx * dy;
  if (power > 0.f) return false;
  float G = expf(power);
  float raw = opacity * G;
  float alpha = fminf(ALPHA_MAX, raw);
  if (alpha < ALPHA_MIN) return false;
  float om = 1.f - alpha;
  float Tk = p.T / om;
  float w = alpha * Tk;
  for (int e = 0; e < E; ++e) attr[e] = gx[e] * w;
  float dalpha = gx[0] * (a[0] * Tk - p.behind[0] / om);
  for (int e = 1; e < E; ++e) dalpha += gx[e] * (a[e] * Tk - p.behind[e] / om);
  for (int e = 0; e < E; ++e) p.behind[e] += a[e] * w;
  p.T = Tk;
  float dop = 0.f, dpow = 0.f;
  if (!(raw > ALPHA_MAX)) { dop = dalpha * G; dpow = dalpha * raw; }  // a bound clamp has zero slope
  float ux = A * dx + B * dy, uy = B * dx + C * dy;  // conic . d: power = -1/2 d . u
  geom[0] = -dpow * ux;
  geom[1] = -dpow * uy;
  geom[2] = dpow * (0.5f * ux * ux);
  geom[3] = dpow * (ux * uy);
  geom[4] = dpow * (0.5f * uy * uy);
  geom[5] = dop;
  return true;
}

}  // namespace rast
