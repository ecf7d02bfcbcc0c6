// shadow_math.hpp -- the shadow network of the appearance loop (scene/shadow.py:14-181 over scene/network.py: Conv2dUB,
// weight_norm_wrapper, Conv2dWN, Conv2dWNUB), forward and backward, as the statements the device (shadow.hip) and the host
// (tests/hostshadow/) share: the three index and weight rules of the resamplings and their tables, the tap order of the 3 x 3
// convolution, LeakyReLU, sigmoid, the weight norm, and the layouts of the table blob and of the workspace.  All arithmetic is fp32.
//
// The network, for shadow_size S, uv_size U, C = n_dims channels, level sizes s_i = S >> i (i = 0..3):
//   x   = nearest(ao_map -> S x S) - ao_mean                                                      [N, 1, S, S]
//   e_i = lrelu(conv3x3(i == 0 ? x : down(e_{i-1})) + bias_i)            i = 0..3, at s_i         layers 0..3
//   d_0 = lrelu(conv3x3(e_3) + bias),  d_j = lrelu(conv3x3([up(d_{j-1}), e_{3-j}]) + bias)  j = 1..3, at s_{3-j}   layers 4..7
//   low = sigmoid(conv3x3(d_3) + bias + beta)                                                     layer 8, C -> 1
//   map = bilinear(low -> U x U, align_corners = False)
// down / up are bilinear with align_corners = True; conv weights are w[o] = v[o] g[o] / ||v||_F with ONE norm over the whole of v.
//
// Rules kept everywhere:
//   * a resampling is never materialised: a layer reads its input through input_at(), which applies the layer's input transform;
//   * every discrete decision and every fp32 weight of a resampling lives in a 1-D table built once on the host (fill_tables); the
//     forward pass reads (i0, i1, l1) per destination index, the backward pass reads the inverse lists per source index, whose
//     weights are the same floats.  The adjoint of a resampling is therefore a gather, and nothing here uses a floating-point atomic;
//   * tap order of the convolution: input channel outermost, then kernel row, then kernel column, accumulated from zero per output
//     channel; the bias is added after the last tap.  The transposed convolution of the backward pass: output channel outermost, then
//     kernel row, then kernel column;
//   * the rules that decide an index (nearest_src, bilinear_tap) are compiled without FMA contraction, so the host build, the device
//     library's host code and torch agree on every cell; the arithmetic on values may contract on the device.
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

namespace shadow {

constexpr int TILE_W = 32, TILE_H = 8, HALO_W = TILE_W + 2, HALO_H = TILE_H + 2, PLANE = HALO_W * HALO_H, TPB = TILE_W * TILE_H;
constexpr int LAYERS = 9, HEAD = 8, MAX_C = 8;
enum { IN_AO = 0, IN_PLAIN = 1, IN_RESAMPLE = 2 };

// ---- the three index and weight rules ----------------------------------------------------------------------------------------------

// F.interpolate(size=) in its default mode, legacy nearest: src = min(floor(dst * (in / out)), in - 1), the scale in fp32
__host__ __device__ __forceinline__ int32_t nearest_src(int dst, int in, int out) {
#pragma clang fp contract(off)
  float scale = (float)in / (float)out;
  int32_t s = (int32_t)floorf((float)dst * scale);
  return s < in - 1 ? s : in - 1;
}

struct Tap {
  int32_t i0, i1;
  float l1;  // weight of i1; the weight of i0 is 1 - l1
};

// bilinear, one axis.  align_corners = True: src = dst (in - 1) / (out - 1), 0 where out == 1.  align_corners = False:
// src = max((dst + 0.5) in / out - 0.5, 0).  i0 = min(int(src), in - 1), i1 = min(i0 + 1, in - 1), l1 = src - i0 in [0, 1].
__host__ __device__ __forceinline__ Tap bilinear_tap(int dst, int in, int out, bool align_corners) {
#pragma clang fp contract(off)
  float src;
  if (align_corners) {
    float scale = out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f;
    src = scale * (float)dst;
  } else {
    float scale = (float)in / (float)out;
    src = scale * ((float)dst + 0.5f) - 0.5f;
    if (src < 0.f) src = 0.f;
  }
  Tap t;
  t.i0 = (int32_t)src;
  if (t.i0 > in - 1) t.i0 = in - 1;
  t.i1 = t.i0 + (t.i0 < in - 1 ? 1 : 0);
  float l = src - (float)t.i0;
  t.l1 = l < 0.f ? 0.f : l > 1.f ? 1.f : l;
  return t;
}

// torch's order of the four products
__host__ __device__ __forceinline__ float bilerp(float v00, float v01, float v10, float v11, float lx, float ly) {
  float w0 = 1.f - lx, h0 = 1.f - ly;
  return h0 * (w0 * v00 + lx * v01) + ly * (w0 * v10 + lx * v11);
}

__host__ __device__ __forceinline__ float lrelu(float x, float slope) { return x > 0.f ? x : x * slope; }
// from the saved OUTPUT, as torch's in-place LeakyReLU does (slope >= 0): the derivative at exactly 0 is the slope
__host__ __device__ __forceinline__ float lrelu_grad(float y, float slope) { return y > 0.f ? 1.f : slope; }
__host__ __device__ __forceinline__ float sigmoid(float x) { return 1.f / (1.f + expf(-x)); }
__host__ __device__ __forceinline__ float sigmoid_grad(float s) { return s * (1.f - s); }

// ---- shapes --------------------------------------------------------------------------------------------------------------------------

__host__ __device__ __forceinline__ int level_size(int S, int i) { return S >> i; }
// layer L = 0..3 encoder, 4..7 decoder, 8 head
__host__ __device__ __forceinline__ int layer_size(int S, int L) { return L < 4 ? level_size(S, L) : L < 8 ? level_size(S, 7 - L) : S; }
__host__ __device__ __forceinline__ int layer_cin(int C, int L) { return L == 0 ? 1 : (L >= 5 && L <= 7) ? 2 * C : C; }
__host__ __device__ __forceinline__ int layer_cout(int C, int L) { return L == HEAD ? 1 : C; }
__host__ __device__ __forceinline__ int layer_nw(int C, int L) { return layer_cout(C, L) * layer_cin(C, L) * 9; }
__host__ __device__ __forceinline__ int tiles_x(int size) { return (size + TILE_W - 1) / TILE_W; }
__host__ __device__ __forceinline__ int tiles_y(int size) { return (size + TILE_H - 1) / TILE_H; }
__host__ __device__ __forceinline__ int layer_tiles(int S, int L) { return tiles_x(layer_size(S, L)) * tiles_y(layer_size(S, L)); }

// ---- the table blob: int32 words, floats stored by bit pattern -----------------------------------------------------------------------
// [ny: S][nx: S][down 0..2][up 0..2][final], a resampling in -> out being
// [i0: out][i1: out][l1: out][inv_start: in + 1][inv_dst: 2 out][inv_w: 2 out]

struct Resample {
  const int32_t *i0, *i1;
  const float *l1;
  const int32_t *inv_start, *inv_dst;  // per source index: the destinations that read it, ascending (destination, side)
  const float *inv_w;                  // and the weight each of them gives it: 1 - l1 on side 0, l1 on side 1
  int32_t in, out;
};

struct Tables {
  const int32_t *ny, *nx;  // nearest source row / column of the input map per row / column of the S x S map
  Resample down[3];        // s_i -> s_{i+1}
  Resample up[3];          // s_{3-k} -> s_{2-k}: what decoder k + 1 reads decoder k through
  Resample fin;            // S -> U, align_corners = False
};

inline int64_t resample_words(int in, int out) { return 7 * (int64_t)out + in + 1; }

inline int64_t table_words(int S, int U) {
  int64_t n = 2 * (int64_t)S;
  for (int i = 0; i < 3; ++i) n += resample_words(level_size(S, i), level_size(S, i + 1));
  for (int k = 0; k < 3; ++k) n += resample_words(level_size(S, 3 - k), level_size(S, 2 - k));
  return n + resample_words(S, U);
}

inline Resample resample_at(const int32_t *p, int in, int out) {
  Resample r;
  r.i0 = p;
  r.i1 = p + out;
  r.l1 = (const float *)(p + 2 * (int64_t)out);
  r.inv_start = p + 3 * (int64_t)out;
  r.inv_dst = r.inv_start + in + 1;
  r.inv_w = (const float *)(r.inv_dst + 2 * (int64_t)out);
  r.in = in;
  r.out = out;
  return r;
}

// base != nullptr
inline Tables tables_at(const int32_t *base, int S, int U) {
  Tables t;
  t.ny = base;
  t.nx = base + S;
  const int32_t *p = base + 2 * (int64_t)S;
  for (int i = 0; i < 3; ++i) {
    t.down[i] = resample_at(p, level_size(S, i), level_size(S, i + 1));
    p += resample_words(level_size(S, i), level_size(S, i + 1));
  }
  for (int k = 0; k < 3; ++k) {
    t.up[k] = resample_at(p, level_size(S, 3 - k), level_size(S, 2 - k));
    p += resample_words(level_size(S, 3 - k), level_size(S, 2 - k));
  }
  t.fin = resample_at(p, S, U);
  return t;
}

inline void fill_resample(int32_t *p, int in, int out, bool align_corners) {
  int32_t *i0 = p, *i1 = p + out, *start = p + 3 * (int64_t)out, *dst = start + in + 1;
  float *l1 = (float *)(p + 2 * (int64_t)out), *w = (float *)(dst + 2 * (int64_t)out);
  for (int d = 0; d < out; ++d) {
    Tap t = bilinear_tap(d, in, out, align_corners);
    i0[d] = t.i0;
    i1[d] = t.i1;
    l1[d] = t.l1;
  }
  for (int s = 0; s <= in; ++s) start[s] = 0;
  for (int d = 0; d < out; ++d) { ++start[i0[d] + 1]; ++start[i1[d] + 1]; }
  for (int s = 0; s < in; ++s) start[s + 1] += start[s];
  // a stable counting sort over ascending (destination, side); the fill position of a source index is kept in its own start
  // entry and restored afterwards
  for (int d = 0; d < out; ++d)
    for (int side = 0; side < 2; ++side) {
      int s = side ? i1[d] : i0[d];
      int at = start[s]++;
      dst[at] = d;
      w[at] = side ? l1[d] : 1.f - l1[d];
    }
  for (int s = in; s > 0; --s) start[s] = start[s - 1];
  start[0] = 0;
}

// words: table_words(S, U) int32
inline void fill_tables(int32_t *words, int in_h, int in_w, int S, int U) {
  for (int y = 0; y < S; ++y) words[y] = nearest_src(y, in_h, S);
  for (int x = 0; x < S; ++x) words[S + x] = nearest_src(x, in_w, S);
  int32_t *p = words + 2 * (int64_t)S;
  for (int i = 0; i < 3; ++i) {
    fill_resample(p, level_size(S, i), level_size(S, i + 1), true);
    p += resample_words(level_size(S, i), level_size(S, i + 1));
  }
  for (int k = 0; k < 3; ++k) {
    fill_resample(p, level_size(S, 3 - k), level_size(S, 2 - k), true);
    p += resample_words(level_size(S, 3 - k), level_size(S, 2 - k));
  }
  fill_resample(p, S, U, false);
}

// ---- the workspace: fp32 words -----------------------------------------------------------------------------------------------------
// normalised weights and the nine norms | the eight post-activation maps (saved for backward) | backward only: the input gradient of
// layers 1..8, the pre-sigmoid gradient, the per-tile partial sums of dW (entry-major) and of the tied head bias, the reduced dW

struct Workspace {
  int64_t w[LAYERS], norm, act[8], dx[LAYERS], dz, part[LAYERS], part_bias, dw[LAYERS], words;
};

inline int64_t round4(int64_t n) { return (n + 3) & ~(int64_t)3; }

inline Workspace workspace_layout(int N, int S, int C) {
  Workspace ws;
  int64_t at = 0;
  for (int L = 0; L < LAYERS; ++L) { ws.w[L] = at; at += round4(layer_nw(C, L)); }
  ws.norm = at; at += 12;
  for (int L = 0; L < 8; ++L) { ws.act[L] = at; at += round4((int64_t)N * C * layer_size(S, L) * layer_size(S, L)); }
  ws.dx[0] = -1;
  for (int L = 1; L < LAYERS; ++L) { ws.dx[L] = at; at += round4((int64_t)N * layer_cin(C, L) * layer_size(S, L) * layer_size(S, L)); }
  ws.dz = at; at += round4((int64_t)N * S * S);
  for (int L = 0; L < LAYERS; ++L) { ws.part[L] = at; at += round4((int64_t)layer_nw(C, L) * layer_tiles(S, L)); }
  ws.part_bias = at; at += round4(layer_tiles(S, HEAD));
  for (int L = 0; L < LAYERS; ++L) { ws.dw[L] = at; at += round4(layer_nw(C, L)); }
  ws.words = at;
  return ws;
}

// ---- a layer's input, read through its transform ---------------------------------------------------------------------------------------

struct LayerIn {
  int32_t mode, size, ca, cb;  // the input has ca + cb channels of size x size
  const float *a;              // IN_PLAIN: [N, ca, size, size]; IN_RESAMPLE: [N, ca, rs.in, rs.in], read bilinearly
  Resample rs;
  const float *b;              // the skip [N, cb, size, size] behind the ca channels, or nullptr
  const float *ao;             // IN_AO: [N, in_h, in_w] read through ny / nx, minus mean [size, size]
  const int32_t *ny, *nx;
  const float *mean;
  int32_t in_h, in_w;
};

__host__ __device__ __forceinline__ float input_at(const LayerIn &in, int n, int c, int y, int x) {
  const int s = in.size;
  if (c >= in.ca) return in.b[(((int64_t)n * in.cb + (c - in.ca)) * s + y) * s + x];
  if (in.mode == IN_AO) return in.ao[((int64_t)n * in.in_h + in.ny[y]) * in.in_w + in.nx[x]] - in.mean[y * s + x];
  if (in.mode == IN_PLAIN) return in.a[(((int64_t)n * in.ca + c) * s + y) * s + x];
  const int q = in.rs.in;
  const float *p = in.a + ((int64_t)n * in.ca + c) * q * q;
  const int y0 = in.rs.i0[y], y1 = in.rs.i1[y], x0 = in.rs.i0[x], x1 = in.rs.i1[x];
  return bilerp(p[y0 * q + x0], p[y0 * q + x1], p[y1 * q + x0], p[y1 * q + x1], in.rs.l1[x], in.rs.l1[y]);
}

// element `idx` (< channels * PLANE) of the tile at (ty0, tx0) with its halo of one: zero outside the map (the padding)
__host__ __device__ __forceinline__ float input_tile_at(const LayerIn &in, int n, int idx, int ty0, int tx0) {
  const int c = idx / PLANE, r = idx % PLANE, y = ty0 - 1 + r / HALO_W, x = tx0 - 1 + r % HALO_W;
  if (y < 0 || y >= in.size || x < 0 || x >= in.size) return 0.f;
  return input_at(in, n, c, y, x);
}

// ---- the convolution over a tile [channels][HALO_H][HALO_W] ---------------------------------------------------------------------------
// (ly, lx): the thread's pixel inside the tile, 0-based without the halo

template <int CIN, int COUT>
__host__ __device__ __forceinline__ void conv_at(const float *tile, const float *w, int ly, int lx, float acc[COUT]) {
  for (int o = 0; o < COUT; ++o) acc[o] = 0.f;
#pragma unroll
  for (int c = 0; c < CIN; ++c)
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const float v = tile[c * PLANE + (ly + ky) * HALO_W + lx + kx];
#pragma unroll
        for (int o = 0; o < COUT; ++o) acc[o] += w[((o * CIN + c) * 3 + ky) * 3 + kx] * v;
      }
}

// dX[ci] at the pixel from the tile of dPre = dY lrelu'(Y): the same weights flipped and transposed
template <int CIN, int COUT>
__host__ __device__ __forceinline__ void conv_transpose_at(const float *dpre, const float *w, int ly, int lx, float dx[CIN]) {
  for (int c = 0; c < CIN; ++c) dx[c] = 0.f;
#pragma unroll
  for (int o = 0; o < COUT; ++o)
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const float g = dpre[o * PLANE + (ly + 2 - ky) * HALO_W + lx + 2 - kx];
#pragma unroll
        for (int c = 0; c < CIN; ++c) dx[c] += w[((o * CIN + c) * 3 + ky) * 3 + kx] * g;
      }
}

// one tile's share of dW entry e = ((o CIN + c) 3 + ky) 3 + kx: the tile's pixels in row-major order
template <int CIN>
__host__ __device__ __forceinline__ float dw_tile_sum(const float *xin, const float *dpre, int e) {
  const int kx = e % 3, ky = (e / 3) % 3, c = (e / 9) % CIN, o = e / (9 * CIN);
  const float *g = dpre + o * PLANE + HALO_W + 1, *x = xin + c * PLANE + ky * HALO_W + kx;
  float acc = 0.f;
#pragma unroll 1
  for (int py = 0; py < TILE_H; ++py)
    for (int px = 0; px < TILE_W; ++px) acc += g[py * HALO_W + px] * x[py * HALO_W + px];
  return acc;
}

// the tile's sum of the head's pre-sigmoid gradient (the tied bias), the same order
__host__ __device__ __forceinline__ float tile_sum(const float *dpre) {
  float acc = 0.f;
#pragma unroll 1
  for (int py = 0; py < TILE_H; ++py)
    for (int px = 0; px < TILE_W; ++px) acc += dpre[(py + 1) * HALO_W + px + 1];
  return acc;
}

// ---- the gradient a layer's output receives ---------------------------------------------------------------------------------------------

// adjoint of a bilinear resampling at source (y, x): a gather over the inverse lists, rows outermost as in bilerp.
// g: one [rs.out, rs.out] plane of the gradient of the resampled map
__host__ __device__ __forceinline__ float adjoint_at(const Resample &rs, const float *g, int y, int x) {
  float acc = 0.f;
  for (int ey = rs.inv_start[y]; ey < rs.inv_start[y + 1]; ++ey) {
    const float *row = g + (int64_t)rs.inv_dst[ey] * rs.out;
    float r = 0.f;
    for (int ex = rs.inv_start[x]; ex < rs.inv_start[x + 1]; ++ex) r += rs.inv_w[ex] * row[rs.inv_dst[ex]];
    acc += rs.inv_w[ey] * r;
  }
  return acc;
}

struct LayerGrad {         // where dY of a layer comes from: the input gradients of the layers that read its output
  const float *dz;         // the head: its pre-sigmoid gradient [N, size, size]; everything below is then unused
  const float *ga;         // reader A's input gradient [N, ga_ch, .., ..], channels 0 .. cout - 1
  int32_t ga_ch, ga_resampled;
  Resample ga_rs;          // ga_resampled: reader A reads this layer through ga_rs, so ga is [.., ga_rs.out, ga_rs.out]
  const float *gb;         // reader B (the skip) [N, gb_ch, size, size], channels gb_off .. gb_off + cout - 1; or nullptr
  int32_t gb_ch, gb_off;
  const float *y;          // the layer's saved output [N, cout, size, size]
  float slope;
};

// dPre = dY lrelu'(Y) at (n, o, y, x) inside the map; A before B
__host__ __device__ __forceinline__ float dpre_at(const LayerGrad &gr, int size, int cout, int n, int o, int y, int x) {
  if (gr.dz) return gr.dz[((int64_t)n * size + y) * size + x];
  float dy;
  if (gr.ga_resampled)
    dy = adjoint_at(gr.ga_rs, gr.ga + ((int64_t)n * gr.ga_ch + o) * gr.ga_rs.out * gr.ga_rs.out, y, x);
  else
    dy = gr.ga[(((int64_t)n * gr.ga_ch + o) * size + y) * size + x];
  if (gr.gb) dy += gr.gb[(((int64_t)n * gr.gb_ch + gr.gb_off + o) * size + y) * size + x];
  return dy * lrelu_grad(gr.y[(((int64_t)n * cout + o) * size + y) * size + x], gr.slope);
}

__host__ __device__ __forceinline__ float dpre_tile_at(const LayerGrad &gr, int size, int cout, int n, int idx, int ty0, int tx0) {
  const int o = idx / PLANE, r = idx % PLANE, y = ty0 - 1 + r / HALO_W, x = tx0 - 1 + r % HALO_W;
  if (y < 0 || y >= size || x < 0 || x >= size) return 0.f;
  return dpre_at(gr, size, cout, n, o, y, x);
}

// the gradient of the pre-sigmoid map at (n, y, x): (g_lowres + adjoint of the final resize of g_map) sigmoid'(lowres).
// identity: U == S, where the forward pass copied.  NULL upstreams count as zero.
__host__ __device__ __forceinline__ float head_dz_at(const Resample &fin, int identity, const float *g_map, const float *g_low, const float *low,
                                                     int n, int y, int x) {
  const int S = fin.in, U = fin.out;
  float g = g_low ? g_low[((int64_t)n * S + y) * S + x] : 0.f;
  if (g_map) g += identity ? g_map[((int64_t)n * S + y) * S + x] : adjoint_at(fin, g_map + (int64_t)n * U * U, y, x);
  return g * sigmoid_grad(low[((int64_t)n * S + y) * S + x]);
}

// map[n, y, x] of the final resize
__host__ __device__ __forceinline__ float final_at(const Resample &fin, const float *low, int n, int y, int x) {
  const int S = fin.in;
  const float *p = low + (int64_t)n * S * S;
  const int y0 = fin.i0[y], y1 = fin.i1[y], x0 = fin.i0[x], x1 = fin.i1[x];
  return bilerp(p[y0 * S + x0], p[y0 * S + x1], p[y1 * S + x0], p[y1 * S + x1], fin.l1[x], fin.l1[y]);
}

// ---- which buffers a layer reads: said once for the device launches and the host loops -------------------------------------------------
// base: the workspace; ao [N, in_h, in_w] and mean [S, S]: the network's input and ao_mean

inline LayerIn layer_input(int L, int C, int S, const Tables &tb, const Workspace &ws, const float *base, const float *ao, const float *mean,
                           int in_h, int in_w) {
  LayerIn in = {};
  in.size = layer_size(S, L);
  in.ca = L == 0 ? 1 : C;
  if (L == 0) {
    in.mode = IN_AO;
    in.ao = ao; in.ny = tb.ny; in.nx = tb.nx; in.mean = mean; in.in_h = in_h; in.in_w = in_w;
  } else if (L == 4 || L == HEAD) {
    in.mode = IN_PLAIN;
    in.a = base + ws.act[L - 1];
  } else {
    in.mode = IN_RESAMPLE;
    in.a = base + ws.act[L - 1];
    in.rs = L < 4 ? tb.down[L - 1] : tb.up[L - 5];
    if (L > 4) { in.b = base + ws.act[7 - L]; in.cb = C; }   // decoder j = L - 4 beside encoder 3 - j
  }
  return in;
}

// encoder i < 3 is read by encoder i + 1 (through down[i]) and by decoder 3 - i (the skip: channels C .. 2C - 1); encoder 3 by decoder 0;
// decoder j < 3 by decoder j + 1 (through up[j]); decoder 3 by the head
inline LayerGrad layer_grad(int L, int C, const Tables &tb, const Workspace &ws, const float *base, float slope) {
  LayerGrad gr = {};
  gr.slope = slope;
  if (L == HEAD) {
    gr.dz = base + ws.dz;
    return gr;
  }
  gr.y = base + ws.act[L];
  gr.ga = base + ws.dx[L + 1];
  gr.ga_ch = layer_cin(C, L + 1);
  if (L < 3) {
    gr.ga_resampled = 1; gr.ga_rs = tb.down[L];
    gr.gb = base + ws.dx[7 - L]; gr.gb_ch = 2 * C; gr.gb_off = C;
  } else if (L >= 4 && L < 7) {
    gr.ga_resampled = 1; gr.ga_rs = tb.up[L - 4];
  }
  return gr;
}

// ---- the weight norm: w[o] = v[o] g[o] / n with n = ||v||_F over the whole tensor --------------------------------------------------------
// The sum of squares: lane t of TPB adds elements t, t + TPB, .. in ascending order (wn_partial), then a binary tree over the TPB
// partials, stride TPB / 2 down to 1 (part[t] += part[t + stride] for t < stride).  The backward pass sums <dW[o], v[o]> per
// output channel in ascending element order, then over o in ascending order.

__host__ __device__ __forceinline__ float wn_partial(const float *v, int count, int t) {
  float acc = 0.f;
  for (int i = t; i < count; i += TPB) acc += v[i] * v[i];
  return acc;
}

__host__ __device__ __forceinline__ float wn_weight(float v, float g, float norm) { return v * g / norm; }

__host__ __device__ __forceinline__ float wn_dot(const float *dw, const float *v, int o, int per_o) {
  float acc = 0.f;
  for (int i = 0; i < per_o; ++i) acc += dw[o * per_o + i] * v[o * per_o + i];
  return acc;
}

// dg[o] = dot[o] / n;  dv = dW (g[o] / n) - v total / n^3  with total = sum_o g[o] dot[o]
__host__ __device__ __forceinline__ float wn_dg(float dot, float norm) { return dot / norm; }
__host__ __device__ __forceinline__ float wn_dv(float dw, float v, float g, float norm, float total) {
  return dw * (g / norm) - v * (total / (norm * norm * norm));
}

}  // namespace shadow
