// The backward math of the rasteriser (mpmavatar_amd/csrc/raster_grad_math.hpp) compiled for the host
// (tests/test_raster_grad_host.py; the stand-in for <hip/hip_runtime.h> is tests/hostmath/stub): a serial statement of the whole
// pipeline -- preprocess, per-tile lists in depth order, per-pixel forward walk, per-pixel backward walk, per-Gaussian sums,
// per-Gaussian backward -- as raster.hip and raster_backward.hip run it, sums in the device's order.
#include "raster_grad_math.hpp"
#include <algorithm>
#include <cstdint>
#include <vector>
using namespace rast;

// cov6 == NULL: scales / rotations (d_scales, d_rots written); else d_cov6.  shs == NULL: colors (d_colors written); else d_shs.
// g_image [3*H*W], g_alpha [H*W].  Every output is written in full.  Returns the number of (tile, Gaussian) entries.
extern "C" int64_t hg_backward(int n, const float *means, const float *opac, const float *scales, const float *rots, float mod,
                               const float *cov6, const float *shs, int n_sh, int sh_degree, const float *colors, const float *view,
                               const float *proj, const float *campos, int W, int H, float tanfovx, float tanfovy, const float *bg,
                               const float *g_image, const float *g_alpha, float *d_means, float *d_means2d, float *d_opac,
                               float *d_scales, float *d_rots, float *d_cov6, float *d_shs, float *d_colors, float *out_image,
                               float *out_alpha) {
  const int gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE;
  std::vector<Splat> sp(n);
  std::vector<Sym3> cov(n);
  std::vector<V3> col(n);
  const V3 cp{campos[0], campos[1], campos[2]};
  for (int i = 0; i < n; ++i) {
    V3 mean{means[3 * i], means[3 * i + 1], means[3 * i + 2]};
    cov[i] = cov6 ? Sym3{cov6[6 * i], cov6[6 * i + 1], cov6[6 * i + 2], cov6[6 * i + 3], cov6[6 * i + 4], cov6[6 * i + 5]}
                  : cov3d(V3{scales[3 * i], scales[3 * i + 1], scales[3 * i + 2]}, mod,
                          V4{rots[4 * i], rots[4 * i + 1], rots[4 * i + 2], rots[4 * i + 3]});
    sp[i] = project(mean, cov[i], view, proj, W, H, tanfovx, tanfovy, gx, gy);
    col[i] = shs ? sh_colour(sh_degree, shs + 3 * (int64_t)n_sh * i, mean, cp) : V3{colors[3 * i], colors[3 * i + 1], colors[3 * i + 2]};
  }
  std::vector<int> order;
  for (int i = 0; i < n; ++i)
    if (sp[i].radius > 0) order.push_back(i);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return sp[a].depth < sp[b].depth; });
  std::vector<std::vector<int>> lists((size_t)gx * gy);
  int64_t entries = 0;
  for (int i : order)
    for (int ty = sp[i].y0; ty < sp[i].y1; ++ty)
      for (int tx = sp[i].x0; tx < sp[i].x1; ++tx) { lists[(size_t)ty * gx + tx].push_back(i); ++entries; }
  // per-Gaussian sums in the order the device takes them: per (tile, entry) the 256 pixels of the tile as four trees of 64
  // (a wave's shuffle reduction), the four added in order; then a Gaussian's tiles in the order of its rectangle, row by row
  std::vector<float> part((size_t)n * N_PARTIALS, 0.f);
  const size_t plane = (size_t)W * H;
  std::vector<float> rows;
  for (int ty = 0; ty < gy; ++ty)
    for (int tx = 0; tx < gx; ++tx) {
      const std::vector<int> &l = lists[(size_t)ty * gx + tx];
      rows.assign(l.size() * (size_t)(TILE * TILE) * N_PARTIALS, 0.f);
      for (int lane = 0; lane < TILE * TILE; ++lane) {
        const int x = tx * TILE + lane % TILE, y = ty * TILE + lane / TILE;
        if (x >= W || y >= H) continue;
        Pixel p{1.f, 0.f, 0.f, 0.f};
        size_t stop = 0;
        for (; stop < l.size(); ++stop) {
          const Splat &s = sp[l[stop]];
          if (blend(p, s.px - (float)x, s.py - (float)y, s.A, s.B, s.C, opac[l[stop]], col[l[stop]])) break;
        }
        const size_t at = (size_t)y * W + x;
        if (out_image) {
          out_image[at] = p.r + p.T * bg[0]; out_image[plane + at] = p.g + p.T * bg[1]; out_image[2 * plane + at] = p.b + p.T * bg[2];
          out_alpha[at] = 1.f - p.T;
        }
        const V3 gi{g_image[at], g_image[plane + at], g_image[2 * plane + at]};
        const float gt = (gi.x * bg[0] + gi.y * bg[1] + gi.z * bg[2] - g_alpha[at]) * p.T;
        PixelBack b{p.T, 0.f, 0.f, 0.f};
        for (size_t k = stop; k-- > 0;) {
          const int g = l[k];
          const Splat &s = sp[g];
          blend_backward(b, s.px - (float)x, s.py - (float)y, s.A, s.B, s.C, opac[g], col[g], gi, gt,
                         &rows[(k * (size_t)(TILE * TILE) + lane) * N_PARTIALS]);
        }
      }
      for (size_t k = 0; k < l.size(); ++k)
        for (int q = 0; q < N_PARTIALS; ++q) {
          float sum = 0.f;
          for (int w = 0; w < 4; ++w) {
            float v[64];
            for (int j = 0; j < 64; ++j) v[j] = rows[(k * (size_t)(TILE * TILE) + 64 * w + j) * N_PARTIALS + q];
            for (int off = 32; off > 0; off >>= 1)
              for (int j = 0; j < off; ++j) v[j] += v[j + off];
            sum = w == 0 ? v[0] : sum + v[0];
          }
          part[(size_t)l[k] * N_PARTIALS + q] += sum;
        }
    }
  for (int i = 0; i < n; ++i) {
    const float *o = &part[(size_t)i * N_PARTIALS];
    V3 mean{means[3 * i], means[3 * i + 1], means[3 * i + 2]};
    V3 dmean{0.f, 0.f, 0.f}, dscale{0.f, 0.f, 0.f};
    V4 dq{0.f, 0.f, 0.f, 0.f};
    Sym3 dS{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const bool vis = sp[i].radius > 0;
    if (vis) {
      project_backward(mean, cov[i], view, proj, W, H, tanfovx, tanfovy, o[0], o[1], o[2], o[3], o[4], dmean, dS);
      if (!cov6)
        cov3d_backward(V3{scales[3 * i], scales[3 * i + 1], scales[3 * i + 2]}, mod,
                       V4{rots[4 * i], rots[4 * i + 1], rots[4 * i + 2], rots[4 * i + 3]}, dS, dscale, dq);
    }
    if (shs) {
      float *d = d_shs + 3 * (int64_t)n_sh * i;
      if (vis) sh_backward(sh_degree, shs + 3 * (int64_t)n_sh * i, n_sh, mean, cp, V3{o[6], o[7], o[8]}, d, dmean);
      else for (int k = 0; k < 3 * n_sh; ++k) d[k] = 0.f;
    } else {
      d_colors[3 * i] = vis ? o[6] : 0.f; d_colors[3 * i + 1] = vis ? o[7] : 0.f; d_colors[3 * i + 2] = vis ? o[8] : 0.f;
    }
    d_means[3 * i] = dmean.x; d_means[3 * i + 1] = dmean.y; d_means[3 * i + 2] = dmean.z;
    d_means2d[3 * i] = vis ? o[0] * (0.5f * (float)W) : 0.f; d_means2d[3 * i + 1] = vis ? o[1] * (0.5f * (float)H) : 0.f; d_means2d[3 * i + 2] = 0.f;
    d_opac[i] = vis ? o[5] : 0.f;
    if (cov6) {
      float *d = d_cov6 + 6 * (int64_t)i;
      d[0] = dS.xx; d[1] = dS.xy; d[2] = dS.xz; d[3] = dS.yy; d[4] = dS.yz; d[5] = dS.zz;
    } else {
      d_scales[3 * i] = dscale.x; d_scales[3 * i + 1] = dscale.y; d_scales[3 * i + 2] = dscale.z;
      d_rots[4 * i] = dq.x; d_rots[4 * i + 1] = dq.y; d_rots[4 * i + 2] = dq.z; d_rots[4 * i + 3] = dq.w;
    }
  }
  return entries;
}
