// The rasteriser math of the product (mpmavatar_amd/csrc/raster_math.hpp) compiled for the host (tests/test_raster_host.py; the
// stand-in for <hip/hip_runtime.h> is tests/hostmath/stub).  hr_preprocess is the serial statement of k_raster_preprocess,
// hr_blend of one pixel's walk through its list in k_raster_render.
#include "raster_math.hpp"
#include <cstdint>
using namespace rast;

// cov6 == NULL: from scales / rotations.  out_f [n*9] = px py A B C depth r g b; out_i [n*5] = radius x0 y0 x1 y1.
// shs == NULL: colours are colors_precomp.
extern "C" void hr_preprocess(int n, const float *means, const float *scales, const float *rots, float mod, const float *cov6,
                              const float *shs, int n_sh, int sh_degree, const float *colors, const float *view, const float *proj,
                              const float *campos, int W, int H, float tanfovx, float tanfovy, float *out_f, int32_t *out_i) {
  const int gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE;
  for (int i = 0; i < n; ++i) {
    V3 mean{means[3 * i], means[3 * i + 1], means[3 * i + 2]};
    Sym3 S = cov6 ? Sym3{cov6[6 * i], cov6[6 * i + 1], cov6[6 * i + 2], cov6[6 * i + 3], cov6[6 * i + 4], cov6[6 * i + 5]}
                  : cov3d(V3{scales[3 * i], scales[3 * i + 1], scales[3 * i + 2]}, mod,
                          V4{rots[4 * i], rots[4 * i + 1], rots[4 * i + 2], rots[4 * i + 3]});
    Splat o = project(mean, S, view, proj, W, H, tanfovx, tanfovy, gx, gy);
    V3 c = shs ? sh_colour(sh_degree, shs + 3 * (int64_t)n_sh * i, mean, V3{campos[0], campos[1], campos[2]})
               : V3{colors[3 * i], colors[3 * i + 1], colors[3 * i + 2]};
    float *f = out_f + 9 * (int64_t)i;
    f[0] = o.px; f[1] = o.py; f[2] = o.A; f[3] = o.B; f[4] = o.C; f[5] = o.depth; f[6] = c.x; f[7] = c.y; f[8] = c.z;
    int32_t *k = out_i + 5 * (int64_t)i;
    k[0] = o.radius; k[1] = o.x0; k[2] = o.y0; k[3] = o.x1; k[4] = o.y1;
  }
}

// seq [m*10] = dx dy A B C opacity r g b pad; out [4] = T r g b.  Returns the number of entries offered before the pixel finished
// (m if it never did).
extern "C" int hr_blend(int m, const float *seq, float *out) {
  Pixel p{1.f, 0.f, 0.f, 0.f};
  int j = 0;
  for (; j < m; ++j) {
    const float *s = seq + 10 * (int64_t)j;
    if (blend(p, s[0], s[1], s[2], s[3], s[4], s[5], V3{s[6], s[7], s[8]})) break;
  }
  out[0] = p.T; out[1] = p.r; out[2] = p.g; out[3] = p.b;
  return j;
}
