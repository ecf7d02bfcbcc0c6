// The extra attribute channels of the rasteriser (mpmavatar_amd/csrc/raster_extra_math.hpp) compiled for the host
// (tests/test_raster_extra_host.py; the stand-in for <hip/hip_runtime.h> is tests/hostmath/stub): tests/hostraster_grad/ with
// the two extra walks of raster_extra.hip added -- the forward walk up to where the colour walk stopped, the backward walk whose
// six geometry / opacity sums are added to the colour's row of the entry, and the per-Gaussian sum of the attribute rows -- sums in
// the device's order.  With -DHOSTRASTER_EXTRA_MAIN a stand-alone program for the sanitizers.
#include "raster_extra_math.hpp"
#include <algorithm>
#include <cstdint>
#include <vector>
using namespace rast;

namespace {

// the 256 values of one (entry, partial) as the device adds them: four trees of 64 (a wave's shuffle reduction), then in order
float tile_sum(const float *v256, size_t stride) {
  float sum = 0.f;
  for (int w = 0; w < 4; ++w) {
    float v[64];
    for (int j = 0; j < 64; ++j) v[j] = v256[(size_t)(64 * w + j) * stride];
    for (int off = 32; off > 0; off >>= 1)
      for (int j = 0; j < off; ++j) v[j] += v[j + off];
    sum = w == 0 ? v[0] : sum + v[0];
  }
  return sum;
}

struct Frame {
  int n, W, H, gx, gy;
  const float *opac, *bg;
  std::vector<Splat> sp;
  std::vector<V3> col;
  std::vector<std::vector<int>> lists;
};

// One tile, both walks of every pixel; part [n][N_PARTIALS] and xpart [n][E] receive the tile's rows.
template <int E>
void tile_walks(const Frame &f, int tx, int ty, const float *extra, const float *g_image, const float *g_alpha, const float *g_extra,
                float *out_image, float *out_alpha, float *out_extra, float *part, float *xpart) {
  constexpr int NQ = N_GEOM + E, LANES = TILE * TILE;
  const std::vector<int> &l = f.lists[(size_t)ty * f.gx + tx];
  const size_t plane = (size_t)f.W * f.H;
  std::vector<float> rows(l.size() * (size_t)LANES * N_PARTIALS, 0.f), xr(l.size() * (size_t)LANES * NQ, 0.f);
  for (int lane = 0; lane < LANES; ++lane) {
    const int x = tx * TILE + lane % TILE, y = ty * TILE + lane / TILE;
    if (x >= f.W || y >= f.H) continue;
    Pixel p{1.f, 0.f, 0.f, 0.f};
    size_t stop = 0;
    for (; stop < l.size(); ++stop) {
      const Splat &s = f.sp[l[stop]];
      if (blend(p, s.px - (float)x, s.py - (float)y, s.A, s.B, s.C, f.opac[l[stop]], f.col[l[stop]])) break;
    }
    // the extra walk ends where the colour walk ended
    float T = 1.f, acc[E];
    for (int e = 0; e < E; ++e) acc[e] = 0.f;
    for (size_t k = 0; k < stop; ++k) {
      const Splat &s = f.sp[l[k]];
      blend_extra<E>(T, acc, s.px - (float)x, s.py - (float)y, s.A, s.B, s.C, f.opac[l[k]], extra + (size_t)l[k] * E);
    }
    const size_t at = (size_t)y * f.W + x;
    out_image[at] = p.r + p.T * f.bg[0]; out_image[plane + at] = p.g + p.T * f.bg[1]; out_image[2 * plane + at] = p.b + p.T * f.bg[2];
    out_alpha[at] = 1.f - p.T;
    for (int e = 0; e < E; ++e) out_extra[e * plane + at] = acc[e];
    const V3 gi{g_image[at], g_image[plane + at], g_image[2 * plane + at]};
    const float gt = (gi.x * f.bg[0] + gi.y * f.bg[1] + gi.z * f.bg[2] - g_alpha[at]) * p.T;
    float gx[E];
    for (int e = 0; e < E; ++e) gx[e] = g_extra[e * plane + at];
    PixelBack b{p.T, 0.f, 0.f, 0.f};
    PixelBackExtra<E> bx;
    bx.T = p.T;
    for (int e = 0; e < E; ++e) bx.behind[e] = 0.f;
    for (size_t k = stop; k-- > 0;) {
      const int g = l[k];
      const Splat &s = f.sp[g];
      blend_backward(b, s.px - (float)x, s.py - (float)y, s.A, s.B, s.C, f.opac[g], f.col[g], gi, gt,
                     &rows[(k * (size_t)LANES + lane) * N_PARTIALS]);
      float *o = &xr[(k * (size_t)LANES + lane) * NQ];
      blend_extra_backward<E>(bx, s.px - (float)x, s.py - (float)y, s.A, s.B, s.C, f.opac[g], extra + (size_t)g * E, gx, o, o + N_GEOM);
    }
  }
  for (size_t k = 0; k < l.size(); ++k) {
    float row[N_PARTIALS];
    for (int q = 0; q < N_PARTIALS; ++q) row[q] = tile_sum(&rows[k * (size_t)LANES * N_PARTIALS + q], N_PARTIALS);
    for (int q = 0; q < N_GEOM; ++q) row[q] += tile_sum(&xr[k * (size_t)LANES * NQ + q], NQ);   // the read-modify-write of the row
    for (int q = 0; q < N_PARTIALS; ++q) part[(size_t)l[k] * N_PARTIALS + q] += row[q];
    for (int e = 0; e < E; ++e) xpart[(size_t)l[k] * E + e] += tile_sum(&xr[k * (size_t)LANES * NQ + N_GEOM + e], NQ);
  }
}

}  // namespace

// hostraster_grad's hg_backward for scales / rotations and precomputed colours, with the extras: extra [n*E], g_extra [E*H*W],
// d_extra [n*E], out_extra [E*H*W].  Every output is written in full.  Returns the number of (tile, Gaussian) entries, -1 for an
// E outside 1 .. EXTRA_MAX.
extern "C" int64_t hx_backward(int n, const float *means, const float *opac, const float *scales, const float *rots, float mod,
                               const float *colors, const float *extra, int E, const float *view, const float *proj, int W, int H,
                               float tanfovx, float tanfovy, const float *bg, const float *g_image, const float *g_alpha,
                               const float *g_extra, float *d_means, float *d_means2d, float *d_opac, float *d_scales, float *d_rots,
                               float *d_colors, float *d_extra, float *out_image, float *out_alpha, float *out_extra) {
  if (E < 1 || E > EXTRA_MAX) return -1;
  Frame f;
  f.n = n; f.W = W; f.H = H; f.gx = (W + TILE - 1) / TILE; f.gy = (H + TILE - 1) / TILE; f.opac = opac; f.bg = bg;
  f.sp.resize(n); f.col.resize(n);
  std::vector<Sym3> cov(n);
  for (int i = 0; i < n; ++i) {
    V3 mean{means[3 * i], means[3 * i + 1], means[3 * i + 2]};
    cov[i] = cov3d(V3{scales[3 * i], scales[3 * i + 1], scales[3 * i + 2]}, mod, V4{rots[4 * i], rots[4 * i + 1], rots[4 * i + 2], rots[4 * i + 3]});
    f.sp[i] = project(mean, cov[i], view, proj, W, H, tanfovx, tanfovy, f.gx, f.gy);
    f.col[i] = V3{colors[3 * i], colors[3 * i + 1], colors[3 * i + 2]};
  }
  std::vector<int> order;
  for (int i = 0; i < n; ++i)
    if (f.sp[i].radius > 0) order.push_back(i);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return f.sp[a].depth < f.sp[b].depth; });
  f.lists.assign((size_t)f.gx * f.gy, {});
  int64_t entries = 0;
  for (int i : order)
    for (int ty = f.sp[i].y0; ty < f.sp[i].y1; ++ty)
      for (int tx = f.sp[i].x0; tx < f.sp[i].x1; ++tx) { f.lists[(size_t)ty * f.gx + tx].push_back(i); ++entries; }
  std::vector<float> part((size_t)n * N_PARTIALS, 0.f), xpart((size_t)n * E, 0.f);
  for (int ty = 0; ty < f.gy; ++ty)
    for (int tx = 0; tx < f.gx; ++tx) {
#define WALK(N) tile_walks<N>(f, tx, ty, extra, g_image, g_alpha, g_extra, out_image, out_alpha, out_extra, part.data(), xpart.data())
      switch (E) {
        case 1: WALK(1); break;
        case 2: WALK(2); break;
        case 3: WALK(3); break;
        case 4: WALK(4); break;
        case 5: WALK(5); break;
        case 6: WALK(6); break;
        case 7: WALK(7); break;
        default: WALK(8); break;
      }
#undef WALK
    }
  for (int i = 0; i < n; ++i) {
    const float *o = &part[(size_t)i * N_PARTIALS];
    V3 mean{means[3 * i], means[3 * i + 1], means[3 * i + 2]};
    V3 dmean{0.f, 0.f, 0.f}, dscale{0.f, 0.f, 0.f};
    V4 dq{0.f, 0.f, 0.f, 0.f};
    Sym3 dS{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const bool vis = f.sp[i].radius > 0;
    if (vis) {
      project_backward(mean, cov[i], view, proj, W, H, tanfovx, tanfovy, o[0], o[1], o[2], o[3], o[4], dmean, dS);
      cov3d_backward(V3{scales[3 * i], scales[3 * i + 1], scales[3 * i + 2]}, mod,
                     V4{rots[4 * i], rots[4 * i + 1], rots[4 * i + 2], rots[4 * i + 3]}, dS, dscale, dq);
    }
    d_colors[3 * i] = vis ? o[6] : 0.f; d_colors[3 * i + 1] = vis ? o[7] : 0.f; d_colors[3 * i + 2] = vis ? o[8] : 0.f;
    d_means[3 * i] = dmean.x; d_means[3 * i + 1] = dmean.y; d_means[3 * i + 2] = dmean.z;
    d_means2d[3 * i] = vis ? o[0] * (0.5f * (float)W) : 0.f; d_means2d[3 * i + 1] = vis ? o[1] * (0.5f * (float)H) : 0.f; d_means2d[3 * i + 2] = 0.f;
    d_opac[i] = vis ? o[5] : 0.f;
    d_scales[3 * i] = dscale.x; d_scales[3 * i + 1] = dscale.y; d_scales[3 * i + 2] = dscale.z;
    d_rots[4 * i] = dq.x; d_rots[4 * i + 1] = dq.y; d_rots[4 * i + 2] = dq.z; d_rots[4 * i + 3] = dq.w;
    for (int e = 0; e < E; ++e) d_extra[(size_t)i * E + e] = vis ? xpart[(size_t)i * E + e] : 0.f;
  }
  return entries;
}

#ifdef HOSTRASTER_EXTRA_MAIN
#include <cmath>
#include <cstdio>

// A camera at the origin looking down +z, 40 x 20 pixels (3 x 2 tiles, the right column and the bottom row partial).  n thin
// Gaussians over the first tile alone make its list longer than 256 and leave the last tile empty; n = 0 leaves every tile
// empty.  Every buffer has exactly its size, so an index past one ends the run with a report.
static int run(int n, int E) {
  const int W = 40, H = 20;
  const float tanx = 0.5f, tany = 0.25f;
  float view[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  float proj[16] = {1.f / tanx, 0, 0, 0, 0, 1.f / tany, 0, 0, 0, 0, 1, 1, 0, 0, -0.01f, 0};
  const float bg[3] = {0.1f, 0.35f, 0.6f};
  std::vector<float> means((size_t)n * 3), opac(n), scales((size_t)n * 3), rots((size_t)n * 4), cols((size_t)n * 3), extra((size_t)n * E);
  uint32_t state = 12345u;
  auto rnd = [&]() { state = state * 1664525u + 1013904223u; return (float)(state >> 8) / 16777216.f; };
  for (int i = 0; i < n; ++i) {
    const float z = 1.f + 4.f * (float)i / (float)(n > 1 ? n - 1 : 1);
    // pixel = ((x / (tan z) + 1) W - 1) / 2: pixels 2 .. 12 of the first tile
    const float px = 2.f + 10.f * rnd(), py = 2.f + 10.f * rnd();
    means[3 * i] = ((2.f * px + 1.f) / W - 1.f) * tanx * z; means[3 * i + 1] = ((2.f * py + 1.f) / H - 1.f) * tany * z; means[3 * i + 2] = z;
    opac[i] = 0.02f + 0.05f * rnd();
    for (int k = 0; k < 3; ++k) { scales[3 * i + k] = 0.004f * z * (1.f + rnd()); cols[3 * i + k] = rnd(); }
    for (int k = 0; k < 4; ++k) rots[4 * i + k] = rnd() - 0.5f + (k == 0 ? 1.f : 0.f);
    for (int e = 0; e < E; ++e) extra[(size_t)i * E + e] = e == 0 ? (rnd() < 0.5f ? 0.f : 1.f) : rnd();
  }
  const size_t plane = (size_t)W * H;
  std::vector<float> gi(3 * plane), ga(plane), gx((size_t)E * plane);
  for (float &v : gi) v = rnd() - 0.5f;
  for (float &v : ga) v = rnd() - 0.5f;
  for (float &v : gx) v = rnd() - 0.5f;
  std::vector<float> dm((size_t)n * 3), dm2((size_t)n * 3), dop(n), dsc((size_t)n * 3), dr((size_t)n * 4), dc((size_t)n * 3), dx((size_t)n * E);
  std::vector<float> image(3 * plane), alpha(plane), out((size_t)E * plane);
  const int64_t entries = hx_backward(n, means.data(), opac.data(), scales.data(), rots.data(), 1.f, cols.data(), extra.data(), E, view, proj,
                                      W, H, tanx, tany, bg, gi.data(), ga.data(), gx.data(), dm.data(), dm2.data(), dop.data(), dsc.data(),
                                      dr.data(), dc.data(), dx.data(), image.data(), alpha.data(), out.data());
  double sum = 0.0;
  for (const auto *v : {&dm, &dm2, &dop, &dsc, &dr, &dc, &dx, &image, &alpha, &out})
    for (float q : *v) {
      if (!std::isfinite(q)) { std::printf("n %d E %d: a value is not finite\n", n, E); return 1; }
      sum += std::fabs((double)q);
    }
  float far_tile = 0.f;     // the last tile (pixels 32 .. 39 x 16 .. 19) is empty: its extras are exactly zero
  for (int e = 0; e < E; ++e)
    for (int y = 16; y < H; ++y)
      for (int x = 32; x < W; ++x) far_tile = std::fmax(far_tile, std::fabs(out[e * plane + (size_t)y * W + x]));
  std::printf("n %d E %d: %lld entries, sum |.| = %.6g, empty tile max %.3g\n", n, E, (long long)entries, sum, (double)far_tile);
  if (far_tile != 0.f) return 1;
  if (n == 0 && entries != 0) return 1;
  if (n >= 300 && entries <= 256) return 1;   // the first tile's list is longer than one batch
  return 0;
}

int main() {
  for (int E : {1, 2, 3, 5, 8})
    for (int n : {0, 1, 300})
      if (run(n, E)) return 1;
  std::printf("ok\n");
  return 0;
}
#endif
