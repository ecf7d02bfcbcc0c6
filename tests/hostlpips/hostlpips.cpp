// LPIPS (mpmavatar_amd/csrc/lpips_math.hpp) compiled for the host (tests/test_lpips_host.py; the stand-in for <hip/hip_runtime.h> is
// tests/hostmath/stub): serial loops that mirror every kernel of lpips.hip -- the flipped weights, the convolution tile by tile with
// the tile staged through the layer's input rule and every output one fmaf chain in the kernel's K order, the head lane by lane with
// the workgroup's tree, the fp64 sum of the slots; backward the head's derivative and the thirteen convolutions over the backward
// layouts -- over the same workspace layout.  The descriptor is include/mpmhip.h's, with host pointers.
// With -DHOSTLPIPS_MAIN the file is a stand-alone program for a sanitizer build: it runs prepare, forward (kept and not kept) and
// backward over exactly sized buffers at the sizes of the cases `tiny` and `odd`.
#include "lpips_math.hpp"

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/mpmhip.h"

using namespace lpips;

namespace {

// k_lpips_conv: every (image, tile, output channel); the chunks of the kernel do not show, an accumulator lives across them
void conv(const Source &src, const Sink &sink, const float *w, int images) {
  const int K = 9 * src.c, KP = k_padded(K);
  std::vector<float> tile((size_t)src.c * PLANE);
  float acc[TILE_H][TILE_W];
  for (int b = 0; b < images; ++b)
    for (int by = 0; by < tiles_y(sink.h); ++by)
      for (int bx = 0; bx < tiles_x(sink.w); ++bx) {
        const int ty0 = by * TILE_H, tx0 = bx * TILE_W;
        const int rows = std::min(TILE_H, sink.h - ty0), cols = std::min(TILE_W, sink.w - tx0);   // the lanes whose result is stored
        for (int c = 0; c < src.c; ++c)
          for (int r = 0; r < PLANE; ++r) tile[(size_t)c * PLANE + r] = tile_value(src, b, c, ty0 + r / HALO_W - 1, tx0 + r % HALO_W - 1);
        for (int m = 0; m < sink.m; ++m) {
          for (int r = 0; r < rows; ++r)
            for (int x = 0; x < cols; ++x) acc[r][x] = 0.f;
          for (int k = 0; k < KP; ++k) {
            const float wv = k < K ? w[(int64_t)m * K + k] : 0.f;
            const float *from = tile.data() + (k < K ? k_offset(k) : 0);
            for (int r = 0; r < rows; ++r)
              for (int x = 0; x < cols; ++x) acc[r][x] = __builtin_fmaf(wv, k < K ? from[r * HALO_W + x] : 0.f, acc[r][x]);
          }
          for (int r = 0; r < rows; ++r)
            for (int x = 0; x < cols; ++x) *sink_at(sink, b, m, ty0 + r, tx0 + x) = sink_value(sink, m, acc[r][x]);
        }
      }
}

double block_sum(double *red) {
  for (int s = TPB / 2; s > 0; s >>= 1)
    for (int t = 0; t < s; ++t) red[t] += red[t + s];
  return red[0];
}

Source forward_source(const mpmhip_lpips_desc *d, const Workspace &ws, float *base, const float *x, const float *y, int L) {
  const int level = layer_level(L), h = level_size(d->h, level), w = level_size(d->w, level);
  Source s = {};
  s.mode = L == 0 ? SRC_IMAGE : pool_in_front(L) ? SRC_POOLED : SRC_PLAIN;
  s.n_first = d->n; s.c = layer_cin(L); s.h = h; s.w = w;
  s.sh = pool_in_front(L) ? level_size(d->h, level - 1) : h;
  s.sw = pool_in_front(L) ? level_size(d->w, level - 1) : w;
  s.p0 = L == 0 ? x : base + ws.x[L - 1];
  s.p1 = L == 0 ? y : base + ws.y[L - 1];
  for (int c = 0; c < 3; ++c) { s.mean[c] = d->mean[c]; s.std[c] = d->std[c]; }
  return s;
}

}  // namespace

extern "C" int64_t hlp_workspace_words(int n, int h, int w, int keep) { return workspace_layout(n, h, w, keep).words; }

extern "C" int64_t hlp_map_offset(int n, int h, int w, int keep, int L) { return workspace_layout(n, h, w, keep).x[L]; }

extern "C" void hlp_prepare(const mpmhip_lpips_desc *d) {
  for (int L = 0; L < LAYERS; ++L)
    for (int64_t e = 0; e < layer_weights(L); ++e) d->weight_bwd[L][e] = d->weight[L][flipped_source(layer_cin(L), layer_cout(L), e)];
}

extern "C" void hlp_forward(const mpmhip_lpips_desc *d, const float *x, const float *y, int keep, float *base, float *out) {
  const int N = d->n, H = d->h, W = d->w;
  const Workspace ws = workspace_layout(N, H, W, keep);
  for (int L = 0; L < LAYERS; ++L) {
    const Source src = forward_source(d, ws, base, x, y, L);
    Sink sink = {};
    sink.mode = SINK_RELU; sink.n_first = N; sink.m = layer_cout(L); sink.h = src.h; sink.w = src.w;
    sink.o0 = base + ws.x[L]; sink.o1 = base + ws.y[L]; sink.bias = d->bias[L];
    conv(src, sink, d->weight[L], 2 * N);
  }
  double total = 0.0, red[TPB];
  for (int t = 0; t < TAPS; ++t) {
    const int L = tap_layer(t), hw = level_size(H, t) * level_size(W, t), groups = head_groups(H, W, t), C = layer_cout(L);
    double *part = (double *)(base + ws.part[t]);
    for (int n = 0; n < N; ++n)
      for (int g = 0; g < groups; ++g) {
        for (int lane = 0; lane < TPB; ++lane) {
          const int p = g * TPB + lane;
          const int64_t at = (int64_t)n * C * hw + p;
          red[lane] = p < hw ? (double)head_pixel(base + ws.x[L] + at, base + ws.y[L] + at, d->tap_weight[t], C, hw) : 0.0;
        }
        part[(int64_t)n * groups + g] = block_sum(red);
      }
    for (int lane = 0; lane < TPB; ++lane) {
      red[lane] = 0.0;
      for (int i = lane; i < N * groups; i += TPB) red[lane] += part[i];
    }
    total += block_sum(red) / (double)hw;
  }
  out[0] = (float)total;
}

extern "C" void hlp_backward(const mpmhip_lpips_desc *d, const float *g_out, float *base, float *dx) {
  const int N = d->n, H = d->h, W = d->w;
  const Workspace ws = workspace_layout(N, H, W, 1);
  for (int t = 0; t < TAPS; ++t) {
    const int L = tap_layer(t), hw = level_size(H, t) * level_size(W, t), C = layer_cout(L);
    for (int n = 0; n < N; ++n)
      for (int p = 0; p < hw; ++p) {
        const int64_t at = (int64_t)n * C * hw + p;
        head_pixel_backward(base + ws.x[L] + at, base + ws.y[L] + at, d->tap_weight[t], C, hw, g_out[0] / (float)hw, base + ws.dtap[t] + at);
      }
  }
  for (int L = LAYERS - 1; L >= 0; --L) {
    const int level = layer_level(L), h = level_size(H, level), w = level_size(W, level);
    const bool pooled = L + 1 < LAYERS && pool_in_front(L + 1);
    Source s = {};
    s.mode = SRC_GRAD; s.n_first = N; s.c = layer_cout(L); s.h = h; s.w = w; s.pooled = pooled;
    s.sh = pooled ? level_size(H, level + 1) : h;
    s.sw = pooled ? level_size(W, level + 1) : w;
    s.p0 = base + ws.x[L];
    s.p1 = tap_of(L) >= 0 ? base + ws.dtap[tap_of(L)] : nullptr;
    s.p2 = L + 1 < LAYERS ? base + ws.dgrad[(L + 1) & 1] : nullptr;
    Sink sink = {};
    sink.mode = L == 0 ? SINK_IMAGE : SINK_PLAIN; sink.n_first = N; sink.m = layer_cin(L); sink.h = h; sink.w = w;
    sink.o0 = L == 0 ? dx : base + ws.dgrad[L & 1];
    for (int c = 0; c < 3; ++c) sink.std[c] = d->std[c];
    conv(s, sink, d->weight_bwd[L], N);
  }
}

#ifdef HOSTLPIPS_MAIN
#include <cmath>
#include <cstdio>

namespace {

float synth(int64_t i) { return std::sin(0.37f * (float)(i % 100003) + 0.1f); }

// every buffer exactly sized: an access past a map, a weight or a workspace section is the sanitizer's to report
int run(int N, int H, int W) {
  mpmhip_lpips_desc d = {};
  d.n = N; d.h = H; d.w = W;
  const float mean[3] = {-.030f, -.088f, -.188f}, dev[3] = {.458f, .448f, .450f};
  for (int c = 0; c < 3; ++c) { d.mean[c] = mean[c]; d.std[c] = dev[c]; }
  std::vector<float> wt[LAYERS], wb[LAYERS], bias[LAYERS], tap[TAPS];
  for (int L = 0; L < LAYERS; ++L) {
    wt[L].resize(layer_weights(L)); wb[L].resize(layer_weights(L)); bias[L].resize(layer_cout(L));
    const float scale = std::sqrt(2.f / (9.f * layer_cin(L)));
    for (size_t i = 0; i < wt[L].size(); ++i) wt[L][i] = 1.4f * scale * synth((int64_t)i * 7 + L);
    for (size_t i = 0; i < bias[L].size(); ++i) bias[L][i] = 0.05f + 0.05f * synth((int64_t)i + 3 * L);
    d.weight[L] = wt[L].data(); d.weight_bwd[L] = wb[L].data(); d.bias[L] = bias[L].data();
  }
  for (int t = 0; t < TAPS; ++t) {
    tap[t].resize(layer_cout(tap_layer(t)));
    for (size_t i = 0; i < tap[t].size(); ++i) tap[t][i] = (1.f + synth((int64_t)i + t)) / tap[t].size();
    d.tap_weight[t] = tap[t].data();
  }
  std::vector<float> x((size_t)N * 3 * H * W), y(x.size()), dx(x.size(), NAN);
  for (size_t i = 0; i < x.size(); ++i) {
    x[i] = 0.5f + 0.5f * synth((int64_t)i * 3 + 1);
    y[i] = std::min(1.f, std::max(0.f, x[i] + 0.15f * synth((int64_t)i * 5 + 2)));
  }
  hlp_prepare(&d);
  std::vector<float> kept(workspace_layout(N, H, W, 1).words), scratch(workspace_layout(N, H, W, 0).words);
  float out = NAN, again = NAN, g = 1.f;
  hlp_forward(&d, x.data(), y.data(), 1, kept.data(), &out);
  hlp_forward(&d, x.data(), y.data(), 0, scratch.data(), &again);
  if (!std::isfinite(out) || !(out > 0.f)) return 2;
  if (out != again) return 3;
  hlp_backward(&d, &g, kept.data(), dx.data());
  float top = 0.f;
  for (float v : dx) {
    if (!std::isfinite(v)) return 4;
    top = std::max(top, std::fabs(v));
  }
  return top > 0.f ? 0 : 5;
}

}  // namespace

int main() {
  const int cases[][3] = {{1, 16, 16}, {2, 35, 22}};
  for (const auto &c : cases) {
    const int rc = run(c[0], c[1], c[2]);
    if (rc) { std::printf("FAILED %d at N %d, %d x %d\n", rc, c[0], c[1], c[2]); return rc; }
  }
  std::printf("ok: %d configurations, prepare, two forward passes and a backward pass each\n", (int)(sizeof(cases) / sizeof(cases[0])));
  return 0;
}
#endif
