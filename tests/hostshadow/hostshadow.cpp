// The shadow network (mpmavatar_amd/csrc/shadow_math.hpp) compiled for the host (tests/test_shadow_host.py; the stand-in for
// <hip/hip_runtime.h> is tests/hostmath/stub): serial loops that mirror every kernel of shadow.hip stage by stage -- the weight norm
// with its tree, the nine layer steps tile by tile and lane by lane, the final resize; backward the head's pre-sigmoid gradient, the
// nine layer steps with their per-tile slots, the wave-shaped reduction and the weight-norm backward -- over the same tables and the
// same workspace layout.  The descriptor is include/mpmhip.h's, with host pointers.
// With -DHOSTSHADOW_MAIN the file is a stand-alone program for a sanitizer build: it runs forward and backward over exactly sized
// buffers at the sizes of the test cases (an odd level, a 1 x 1 level, partial tiles, a batch, both bias kinds, frozen parameters).
#include "shadow_math.hpp"

#include <cstdint>
#include <vector>

#include "../../include/mpmhip.h"

using namespace shadow;

namespace {

void wn_forward(const mpmhip_shadow_desc *d, const Workspace &ws, float *base) {
  const int C = d->n_dims;
  for (int L = 0; L < LAYERS; ++L) {
    const int count = layer_nw(C, L), per_o = layer_cin(C, L) * 9;
    float part[TPB];
    for (int t = 0; t < TPB; ++t) part[t] = wn_partial(d->weight_v[L], count, t);
    for (int s = TPB / 2; s > 0; s >>= 1)
      for (int t = 0; t < s; ++t) part[t] += part[t + s];
    const float norm = sqrtf(part[0]);
    base[ws.norm + L] = norm;
    for (int i = 0; i < count; ++i) base[ws.w[L] + i] = wn_weight(d->weight_v[L][i], d->weight_g[L][i / per_o], norm);
  }
}

template <int CA, int CB, int COUT, bool IS_HEAD>
void layer_forward(const LayerIn &in, int N, const float *w, const float *bias, int tied, float slope, float beta, float *out, float *out2,
                   float *ao_out) {
  constexpr int CIN = CA + CB;
  const int s = in.size;
  std::vector<float> tile(CIN * PLANE);
  for (int n = 0; n < N; ++n)
    for (int by = 0; by < tiles_y(s); ++by)
      for (int bx = 0; bx < tiles_x(s); ++bx) {
        const int ty0 = by * TILE_H, tx0 = bx * TILE_W;
        for (int idx = 0; idx < CIN * PLANE; ++idx) tile[idx] = input_tile_at(in, n, idx, ty0, tx0);
        for (int t = 0; t < TPB; ++t) {
          const int ly = t / TILE_W, lx = t % TILE_W, y = ty0 + ly, x = tx0 + lx;
          if (y >= s || x >= s) continue;
          float acc[COUT];
          conv_at<CIN, COUT>(tile.data(), w, ly, lx, acc);
          if (IS_HEAD) {
            const float z = acc[0] + (tied ? bias[0] : bias[y * s + x]);
            const float v = sigmoid(z + beta);
            const int64_t at = ((int64_t)n * s + y) * s + x;
            out[at] = v;
            if (out2) out2[at] = v;
          } else {
            for (int o = 0; o < COUT; ++o) out[(((int64_t)n * COUT + o) * s + y) * s + x] = lrelu(acc[o] + bias[(o * s + y) * s + x], slope);
            if (ao_out) ao_out[((int64_t)n * s + y) * s + x] = in.ao[((int64_t)n * in.in_h + in.ny[y]) * in.in_w + in.nx[x]];
          }
        }
      }
}

template <int CA, int CB, int COUT>
void layer_backward(const LayerIn &in, const LayerGrad &gr, int N, const float *w, int want_dw, int tied, float *dx_out, float *d_bias,
                    float *part, float *part_bias) {
  constexpr int CIN = CA + CB, NW = COUT * CIN * 9;
  const int s = in.size, tiles = tiles_x(s) * tiles_y(s);
  std::vector<float> xin(CIN * PLANE), dpre(COUT * PLANE), db(TPB * COUT), dw(NW);
  for (int by = 0; by < tiles_y(s); ++by)
    for (int bx = 0; bx < tiles_x(s); ++bx) {
      const int ty0 = by * TILE_H, tx0 = bx * TILE_W, tile = by * tiles_x(s) + bx;
      float tile_bias = 0.f;
      db.assign(db.size(), 0.f);
      dw.assign(dw.size(), 0.f);
      for (int n = 0; n < N; ++n) {
        if (want_dw)
          for (int idx = 0; idx < CIN * PLANE; ++idx) xin[idx] = input_tile_at(in, n, idx, ty0, tx0);
        for (int idx = 0; idx < COUT * PLANE; ++idx) dpre[idx] = dpre_tile_at(gr, s, COUT, n, idx, ty0, tx0);
        for (int t = 0; t < TPB; ++t) {
          const int ly = t / TILE_W, lx = t % TILE_W, y = ty0 + ly, x = tx0 + lx;
          if (y >= s || x >= s) continue;
          for (int o = 0; o < COUT; ++o) db[t * COUT + o] += dpre[o * PLANE + (ly + 1) * HALO_W + lx + 1];
          if (dx_out) {
            float dx[CIN];
            conv_transpose_at<CIN, COUT>(dpre.data(), w, ly, lx, dx);
            for (int c = 0; c < CIN; ++c) dx_out[(((int64_t)n * CIN + c) * s + y) * s + x] = dx[c];
          }
        }
        if (want_dw)
          for (int e = 0; e < NW; ++e) dw[e] += dw_tile_sum<CIN>(xin.data(), dpre.data(), e);
        if (part_bias) tile_bias += tile_sum(dpre.data());
      }
      for (int t = 0; t < TPB; ++t) {
        const int ly = t / TILE_W, lx = t % TILE_W, y = ty0 + ly, x = tx0 + lx;
        if (y >= s || x >= s || !d_bias || tied) continue;
        for (int o = 0; o < COUT; ++o) d_bias[(o * s + y) * s + x] = db[t * COUT + o];
      }
      if (want_dw)
        for (int e = 0; e < NW; ++e) part[(int64_t)e * tiles + tile] = dw[e];
      if (part_bias) part_bias[tile] = tile_bias;
    }
}

// k_shadow_reduce: lane l adds tiles l, l + 64, ..; then the tree of __shfl_down over 64 lanes, of which lane 0 is read
float wave_sum(const float *p, int tiles) {
  float acc[64];
  for (int lane = 0; lane < 64; ++lane) {
    acc[lane] = 0.f;
    for (int i = lane; i < tiles; i += 64) acc[lane] += p[i];
  }
  for (int off = 32; off > 0; off >>= 1)
    for (int lane = 0; lane < off; ++lane) acc[lane] += acc[lane + off];
  return acc[0];
}

template <int C>
void forward_layers(const mpmhip_shadow_desc *d, const Tables &tb, const Workspace &ws, float *base, const float *ao, float *out_ao,
                    float *out_low, float *out_map) {
  const int S = d->shadow_size, N = d->n;
  for (int L = 0; L < LAYERS; ++L) {
    const LayerIn in = layer_input(L, C, S, tb, ws, base, ao, d->ao_mean, d->in_h, d->in_w);
    const float *w = base + ws.w[L], *bias = d->bias[L];
    float *out = L == HEAD ? out_low : base + ws.act[L];
    const int tied = L == HEAD && !d->untied_head_bias;
    if (L == 0) layer_forward<1, 0, C, false>(in, N, w, bias, tied, d->lrelu_slope, d->beta, out, nullptr, out_ao);
    else if (L == HEAD) layer_forward<C, 0, 1, true>(in, N, w, bias, tied, d->lrelu_slope, d->beta, out, d->uv_size == S ? out_map : nullptr, nullptr);
    else if (L >= 5) layer_forward<C, C, C, false>(in, N, w, bias, tied, d->lrelu_slope, d->beta, out, nullptr, nullptr);
    else layer_forward<C, 0, C, false>(in, N, w, bias, tied, d->lrelu_slope, d->beta, out, nullptr, nullptr);
  }
}

template <int C>
void backward_layers(const mpmhip_shadow_desc *d, const Tables &tb, const Workspace &ws, float *base, const float *ao) {
  const int S = d->shadow_size, N = d->n;
  for (int L = LAYERS - 1; L >= 0; --L) {
    const LayerIn in = layer_input(L, C, S, tb, ws, base, ao, d->ao_mean, d->in_h, d->in_w);
    const LayerGrad gr = layer_grad(L, C, tb, ws, base, d->lrelu_slope);
    const int want_dw = d->d_weight_v[L] || d->d_weight_g[L], tied = L == HEAD && !d->untied_head_bias;
    float *dx = L == 0 ? nullptr : base + ws.dx[L], *part = base + ws.part[L];
    float *part_bias = tied && d->d_bias[L] ? base + ws.part_bias : nullptr;
    const float *w = base + ws.w[L];
    if (L == 0) layer_backward<1, 0, C>(in, gr, N, w, want_dw, tied, dx, d->d_bias[L], part, part_bias);
    else if (L == HEAD) layer_backward<C, 0, 1>(in, gr, N, w, want_dw, tied, dx, d->d_bias[L], part, part_bias);
    else if (L >= 5) layer_backward<C, C, C>(in, gr, N, w, want_dw, tied, dx, d->d_bias[L], part, part_bias);
    else layer_backward<C, 0, C>(in, gr, N, w, want_dw, tied, dx, d->d_bias[L], part, part_bias);
    const int tiles = layer_tiles(S, L);
    if (want_dw)
      for (int e = 0; e < layer_nw(C, L); ++e) base[ws.dw[L] + e] = wave_sum(part + (int64_t)e * tiles, tiles);
    if (part_bias) d->d_bias[L][0] = wave_sum(part_bias, tiles);
  }
}

}  // namespace

extern "C" int64_t hsn_table_words(int S, int U) { return table_words(S, U); }
extern "C" int64_t hsn_workspace_words(int N, int S, int C) { return workspace_layout(N, S, C).words; }
extern "C" void hsn_fill_tables(int32_t *words, int in_h, int in_w, int S, int U) { fill_tables(words, in_h, in_w, S, U); }
extern "C" int hsn_nearest(int dst, int in, int out) { return nearest_src(dst, in, out); }
extern "C" void hsn_tap(int dst, int in, int out, int align_corners, int32_t *i0, int32_t *i1, float *l1) {
  Tap t = bilinear_tap(dst, in, out, align_corners != 0);
  *i0 = t.i0; *i1 = t.i1; *l1 = t.l1;
}

extern "C" void hsn_forward(const mpmhip_shadow_desc *d, const float *ao, float *workspace, float *out_ao, float *out_low, float *out_map) {
  const int S = d->shadow_size, U = d->uv_size;
  const Workspace ws = workspace_layout(d->n, S, d->n_dims);
  const Tables tb = tables_at((const int32_t *)d->tables, S, U);
  wn_forward(d, ws, workspace);
  if (d->n_dims == 4) forward_layers<4>(d, tb, ws, workspace, ao, out_ao, out_low, out_map);
  else forward_layers<8>(d, tb, ws, workspace, ao, out_ao, out_low, out_map);
  if (U != S)
    for (int n = 0; n < d->n; ++n)
      for (int y = 0; y < U; ++y)
        for (int x = 0; x < U; ++x) out_map[((int64_t)n * U + y) * U + x] = final_at(tb.fin, out_low, n, y, x);
}

extern "C" void hsn_backward(const mpmhip_shadow_desc *d, const float *ao, const float *low, const float *g_map, const float *g_low,
                             float *workspace) {
  const int S = d->shadow_size, U = d->uv_size, C = d->n_dims;
  const Workspace ws = workspace_layout(d->n, S, C);
  const Tables tb = tables_at((const int32_t *)d->tables, S, U);
  for (int n = 0; n < d->n; ++n)
    for (int y = 0; y < S; ++y)
      for (int x = 0; x < S; ++x)
        workspace[ws.dz + ((int64_t)n * S + y) * S + x] = head_dz_at(tb.fin, U == S, g_map, g_low, low, n, y, x);
  if (C == 4) backward_layers<4>(d, tb, ws, workspace, ao);
  else backward_layers<8>(d, tb, ws, workspace, ao);
  for (int L = 0; L < LAYERS; ++L) {
    if (!d->d_weight_v[L] && !d->d_weight_g[L]) continue;
    const int count = layer_nw(C, L), per_o = layer_cin(C, L) * 9, cout = count / per_o;
    const float *v = d->weight_v[L], *g = d->weight_g[L], *dw = workspace + ws.dw[L];
    const float norm = workspace[ws.norm + L];
    float dot[MAX_C], total = 0.f;
    for (int o = 0; o < cout; ++o) dot[o] = wn_dot(dw, v, o, per_o);
    for (int o = 0; o < cout; ++o) total += g[o] * dot[o];
    if (d->d_weight_g[L])
      for (int o = 0; o < cout; ++o) d->d_weight_g[L][o] = wn_dg(dot[o], norm);
    if (d->d_weight_v[L])
      for (int i = 0; i < count; ++i) d->d_weight_v[L][i] = wn_dv(dw[i], v[i], g[i / per_o], norm, total);
  }
}

#ifdef HOSTSHADOW_MAIN
#include <cmath>
#include <cstdio>

namespace {

float synth(int i) { return 0.5f * std::sin(0.37f * (float)i + 0.1f); }

// every buffer exactly sized: an access past a row, a table or a workspace section is the sanitizer's to report
int run(int N, int in_h, int in_w, int S, int U, int C, int untied, bool freeze) {
  mpmhip_shadow_desc d = {};
  d.n = N; d.in_h = in_h; d.in_w = in_w; d.shadow_size = S; d.uv_size = U; d.n_dims = C; d.untied_head_bias = untied;
  d.lrelu_slope = 0.2f; d.beta = 1.f;
  std::vector<int32_t> tables(table_words(S, U));
  fill_tables(tables.data(), in_h, in_w, S, U);
  d.tables = tables.data();
  std::vector<float> mean((size_t)S * S), ao((size_t)N * in_h * in_w), ws(workspace_layout(N, S, C).words);
  for (size_t i = 0; i < mean.size(); ++i) mean[i] = 0.5f + 0.2f * synth((int)i);
  for (size_t i = 0; i < ao.size(); ++i) ao[i] = 0.5f + synth((int)i + 3);
  d.ao_mean = mean.data();
  std::vector<float> v[LAYERS], g[LAYERS], b[LAYERS], dv[LAYERS], dg[LAYERS], dbias[LAYERS];
  for (int L = 0; L < LAYERS; ++L) {
    const int s = layer_size(S, L), cout = layer_cout(C, L);
    v[L].resize(layer_nw(C, L)); g[L].resize(cout); b[L].resize(L == HEAD && !untied ? 1 : (size_t)cout * s * s);
    for (size_t i = 0; i < v[L].size(); ++i) v[L][i] = synth((int)i + 11 * L);
    for (size_t i = 0; i < g[L].size(); ++i) g[L][i] = 1.5f + synth((int)i + L);
    for (size_t i = 0; i < b[L].size(); ++i) b[L][i] = 0.3f * synth((int)i + 5 * L);
    dv[L].resize(v[L].size()); dg[L].resize(g[L].size()); dbias[L].resize(b[L].size());
    d.weight_v[L] = v[L].data(); d.weight_g[L] = g[L].data(); d.bias[L] = b[L].data();
    const bool keep = !freeze || L % 2 == 0;
    d.d_weight_v[L] = keep ? dv[L].data() : nullptr;
    d.d_weight_g[L] = keep || L == 3 ? dg[L].data() : nullptr;
    d.d_bias[L] = keep || L == HEAD ? dbias[L].data() : nullptr;
  }
  std::vector<float> out_ao((size_t)N * S * S), low((size_t)N * S * S), map((size_t)N * U * U), g_map(map.size()), g_low(low.size());
  for (size_t i = 0; i < g_map.size(); ++i) g_map[i] = synth((int)i + 7);
  for (size_t i = 0; i < g_low.size(); ++i) g_low[i] = synth((int)i + 9);
  hsn_forward(&d, ao.data(), ws.data(), out_ao.data(), low.data(), map.data());
  for (float x : map) if (!std::isfinite(x) || x <= 0.f || x >= 1.f) return 2;
  if (U == S)
    for (size_t i = 0; i < map.size(); ++i) if (map[i] != low[i]) return 3;
  hsn_backward(&d, ao.data(), low.data(), g_map.data(), nullptr, ws.data());
  hsn_backward(&d, ao.data(), low.data(), nullptr, g_low.data(), ws.data());
  hsn_backward(&d, ao.data(), low.data(), g_map.data(), g_low.data(), ws.data());
  for (int L = 0; L < LAYERS; ++L) {
    for (float x : dv[L]) if (!std::isfinite(x)) return 4;
    for (float x : dbias[L]) if (!std::isfinite(x)) return 5;
  }
  hsn_backward(&d, ao.data(), low.data(), nullptr, nullptr, ws.data());  // no upstream: every wanted gradient is written, with zeros
  for (int L = 0; L < LAYERS; ++L) {
    if (d.d_weight_v[L]) for (float x : dv[L]) if (x != 0.f) return 6;
    if (d.d_bias[L]) for (float x : dbias[L]) if (x != 0.f) return 7;
  }
  return 0;
}

}  // namespace

int main() {
  const int cases[][8] = {{1, 33, 33, 20, 24, 4, 0, 0}, {3, 40, 40, 40, 40, 8, 1, 0}, {1, 16, 16, 16, 12, 4, 0, 1}, {1, 9, 9, 9, 9, 4, 0, 0},
                          {2, 7, 13, 8, 1, 8, 0, 1}, {1, 70, 70, 70, 33, 4, 1, 0}};
  for (const auto &c : cases) {
    const int rc = run(c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7] != 0);
    if (rc) { std::printf("FAILED %d at N %d, input %d x %d, S %d, U %d, C %d\n", rc, c[0], c[1], c[2], c[3], c[4], c[5]); return rc; }
  }
  std::printf("ok: %d configurations, forward and four backward passes each\n", (int)(sizeof(cases) / sizeof(cases[0])));
  return 0;
}
#endif
