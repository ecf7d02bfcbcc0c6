// A serial statement of the image loss, forward and backward, around mpmavatar_amd/csrc/image_loss_math.hpp compiled for
// the host (tests/test_image_loss_host.py builds it with g++ -ffp-contract=off over tests/hostmath/stub).  Same passes as
// csrc/image_loss.hip -- zero-padded input, horizontal sums, vertical sums, point(), and for the gradient the three maps
// convolved again -- without the tiling, which changes no value.  Test infrastructure only.
#include <cmath>
#include <cstdint>
#include <vector>

#include "image_loss_math.hpp"

using imgloss::RAD;
using imgloss::WIN;

namespace {

// src [H * W] -> [(H + 2 RAD) * (W + 2 RAD)] with a zero border
std::vector<float> padded(const float *src, int H, int W) {
  const int PW = W + 2 * RAD;
  std::vector<float> p((size_t)(H + 2 * RAD) * PW, 0.0f);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) p[(size_t)(y + RAD) * PW + x + RAD] = src[(size_t)y * W + x];
  return p;
}

}  // namespace

extern "C" {

void hi_window(float *w) {
  for (int i = 0; i < WIN; ++i) w[i] = imgloss::window(i);
}

// out_means [planes * 3]; maps [planes * 3 * H * W] and ssim_map [planes * H * W] may be NULL
void hi_forward(const float *img, const float *gt, int planes, int H, int W, float *maps, float *ssim_map, float *out_means) {
  const int PW = W + 2 * RAD, PH = H + 2 * RAD;
  const size_t hw = (size_t)H * W;
  for (int p = 0; p < planes; ++p) {
    const float *x = img + p * hw, *y = gt + p * hw;
    std::vector<float> px = padded(x, H, W), py = padded(y, H, W);
    std::vector<float> hm[5];
    for (auto &v : hm) v.resize((size_t)PH * W);
    for (int r = 0; r < PH; ++r)
      for (int c = 0; c < W; ++c) {
        imgloss::Moments h = imgloss::row_moments(&px[(size_t)r * PW + c], &py[(size_t)r * PW + c]);
        size_t i = (size_t)r * W + c;
        hm[0][i] = h.x; hm[1][i] = h.y; hm[2][i] = h.xx; hm[3][i] = h.yy; hm[4][i] = h.xy;
      }
    double s_abs = 0.0, s_sq = 0.0, s_m = 0.0;
    for (int r = 0; r < H; ++r)
      for (int c = 0; c < W; ++c) {
        size_t i = (size_t)r * W + c;
        imgloss::Moments e{imgloss::taps(&hm[0][i], W), imgloss::taps(&hm[1][i], W), imgloss::taps(&hm[2][i], W),
                           imgloss::taps(&hm[3][i], W), imgloss::taps(&hm[4][i], W)};
        imgloss::Point pt = imgloss::point(e);
        float d = x[i] - y[i];
        s_abs += (double)std::fabs(d); s_sq += (double)(d * d); s_m += (double)pt.m;
        if (maps) { float *o = maps + (size_t)p * 3 * hw + i; o[0] = pt.d_mu; o[hw] = pt.d_s1; o[2 * hw] = pt.d_s12; }
        if (ssim_map) ssim_map[p * hw + i] = pt.m;
      }
    out_means[3 * p] = (float)(s_abs / (double)hw);
    out_means[3 * p + 1] = (float)(s_sq / (double)hw);
    out_means[3 * p + 2] = (float)(s_m / (double)hw);
  }
}

void hi_backward(const float *img, const float *gt, int planes, int H, int W, const float *maps, const float *g_l1, const float *g_mse,
                 const float *g_ssim, float *d_img) {
  const int PW = W + 2 * RAD, PH = H + 2 * RAD;
  const size_t hw = (size_t)H * W;
  const float inv_n = (float)(1.0 / ((double)H * (double)W));
  for (int p = 0; p < planes; ++p) {
    std::vector<float> conv[3];
    for (int k = 0; k < 3; ++k) {
      std::vector<float> pm = padded(maps + ((size_t)p * 3 + k) * hw, H, W), h((size_t)PH * W);
      for (int r = 0; r < PH; ++r)
        for (int c = 0; c < W; ++c) h[(size_t)r * W + c] = imgloss::taps(&pm[(size_t)r * PW + c], 1);
      conv[k].resize(hw);
      for (size_t i = 0; i < hw; ++i) conv[k][i] = imgloss::taps(&h[i], W);
    }
    for (size_t i = 0; i < hw; ++i)
      d_img[p * hw + i] = imgloss::pixel_grad(img[p * hw + i], gt[p * hw + i], conv[0][i], conv[1][i], conv[2][i], g_l1[p], g_mse[p],
                                              g_ssim[p], inv_n);
  }
}

}  // extern "C"
