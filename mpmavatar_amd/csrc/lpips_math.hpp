// lpips_math.hpp -- LPIPS (net_type 'vgg', version 0.1; lpipsPyTorch/modules/{lpips,networks,utils}.py) written out: the layer table,
// the tile and its K walk, what a tile load reads forward (z-score, 2 x 2 maximum) and backward (ReLU mask, pooling route, tap
// gradient), the epilogues, the distance head with its derivative, the flipped weights and the workspace.  Host and device compile
// the same text (tests/hostlpips/hostlpips.cpp restates the kernels of lpips.hip over it as serial loops).
//
//   z = (v - mean_c) / std_c                                  zero padding pads z
//   13 x [conv3x3(pad 1) + bias + ReLU], MaxPool2d(2, 2) in front of layers 2, 4, 7, 10; taps after layers 1, 3, 6, 9, 12
//   per tap: u = f / (sqrt(sum_c f_c^2) + 1e-10);  s = sum_c w_c (ux_c - uy_c)^2;  mean over the pixels
//   out [1, 1, 1, 1] = the sum over the five taps AND over the N images (the reference concatenates along the batch and sums it)
//
// The bits.  A convolution output is ONE fmaf chain from 0 over k = 0 .. K - 1, k = c * 9 + ky * 3 + kx (channel, row, column),
// which is what v_mfma_f32_32x32x2_f32 computes when its two k slots are fed in that order; then + bias, then ReLU.  Where K is odd
// (27 of the image layer) one product 0 * 0 closes the chain.  The head sums channels in ascending order with fmaf, a workgroup's
// pixels in a fixed tree, and the workgroups' slots in fp64 in a fixed order.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#define LPIPS_HD __host__ __device__ inline

namespace lpips {

constexpr int LAYERS = 13, TAPS = 5, LEVELS = 5;
constexpr int TPB = 256;                              // four waves
constexpr int TILE_H = 4, TILE_W = 32;                // 128 output pixels; a wave takes two rows, one 32 x 32 MFMA block each
constexpr int HALO_H = TILE_H + 2, HALO_W = TILE_W + 2, PLANE = HALO_H * HALO_W;
constexpr int TILE_M = 64;                            // output channels of a workgroup: two row blocks of 32
constexpr int CHUNK_C = 8;                            // input channels staged per K chunk (the image layer: its 3)
constexpr int W_STRIDE = TILE_M + 1;                  // LDS row of a weight slice [k][m]: writes walk k, reads walk m, both conflict-free
constexpr float EPS = 1e-10f;
constexpr int MIN_SIZE = 16, MAX_SIZE = 8192, MAX_BATCH = 1024;

LPIPS_HD int layer_cout(int L) { return L < 2 ? 64 : L < 4 ? 128 : L < 7 ? 256 : 512; }
LPIPS_HD int layer_cin(int L) { return L == 0 ? 3 : L == 2 ? 64 : L == 4 ? 128 : L == 7 ? 256 : layer_cout(L); }
LPIPS_HD int layer_level(int L) { return L < 2 ? 0 : L < 4 ? 1 : L < 7 ? 2 : L < 10 ? 3 : 4; }
LPIPS_HD bool pool_in_front(int L) { return L == 2 || L == 4 || L == 7 || L == 10; }
LPIPS_HD int tap_layer(int t) { return t == 0 ? 1 : t == 1 ? 3 : t == 2 ? 6 : t == 3 ? 9 : 12; }
LPIPS_HD int tap_of(int L) { return L == 1 ? 0 : L == 3 ? 1 : L == 6 ? 2 : L == 9 ? 3 : L == 12 ? 4 : -1; }
LPIPS_HD int level_size(int s, int level) { return s >> level; }   // four floor halvings
LPIPS_HD int64_t layer_weights(int L) { return (int64_t)layer_cout(L) * layer_cin(L) * 9; }
LPIPS_HD int tiles_x(int w) { return (w + TILE_W - 1) / TILE_W; }
LPIPS_HD int tiles_y(int h) { return (h + TILE_H - 1) / TILE_H; }

// ---- the K walk ----------------------------------------------------------------------------------------------------------------------

// k within a chunk -> the offset of its tap in the staged tile, for the output pixel at (row 0, column 0) of the tile
LPIPS_HD constexpr int k_offset(int k) { return (k / 9) * PLANE + ((k % 9) / 3) * HALO_W + k % 3; }
LPIPS_HD constexpr int k_padded(int k_count) { return (k_count + 1) & ~1; }   // the MFMA takes two k at a time

// ---- what a tile load reads ------------------------------------------------------------------------------------------------------------

enum { SRC_IMAGE = 0, SRC_PLAIN = 1, SRC_POOLED = 2, SRC_GRAD = 3 };

// images 0 .. n_first - 1 of a launch live in p0, the others in p1 (x and y go through the same launches)
// SRC_IMAGE   p0 / p1: the images [n, 3, h, w]; the value is the z-score
// SRC_PLAIN   p0 / p1: the maps [n, c, h, w]
// SRC_POOLED  p0 / p1: the maps [n, c, sh, sw] in front of the pooling; the value is the maximum of the window
// SRC_GRAD    p0: the saved output [n, c, h, w] of the layer, p1: the tap's gradient or NULL, p2: the gradient of the next layer's
//             input or NULL, [n, c, sh, sw] (behind a pooling where pooled).  The value is dOut (out > 0): torch's in-place ReLU rule.
struct Source {
  int32_t mode, n_first, c, h, w, sh, sw, pooled;
  const float *p0, *p1, *p2;
  float mean[3], std[3];
};

LPIPS_HD float zscore(float v, float mean, float std) { return (v - mean) / std; }
LPIPS_HD float relu(float v) { return v > 0.f ? v : 0.f; }

// the first maximum of a 2 x 2 window in row-major order (a later element wins only if it is greater): 0 .. 3
LPIPS_HD int first_max(float a, float b, float c, float d) {
  int at = 0;
  float m = a;
  if (b > m) { m = b; at = 1; }
  if (c > m) { m = c; at = 2; }
  if (d > m) { m = d; at = 3; }
  return at;
}

LPIPS_HD float max4(float a, float b, float c, float d) {
  float m = a;
  if (b > m) m = b;
  if (c > m) m = c;
  if (d > m) m = d;
  return m;
}

// the gradient that arrives at output (c, y, x) of a layer, before the ReLU mask
LPIPS_HD float grad_arriving(const Source &s, const float *out, int64_t img, int c, int y, int x) {
  float g = 0.f;
  if (s.p1) g = s.p1[((img * s.c + c) * s.h + y) * s.w + x];
  if (s.p2) {
    if (!s.pooled) {
      g += s.p2[((img * s.c + c) * s.h + y) * s.w + x];
    } else {
      const int yp = y >> 1, xp = x >> 1;
      if (yp < s.sh && xp < s.sw) {   // an odd size drops its last row or column
        const float *o = out + (int64_t)(2 * yp) * s.w + 2 * xp;
        const int at = first_max(o[0], o[1], o[s.w], o[s.w + 1]);
        if (at == (y & 1) * 2 + (x & 1)) g += s.p2[((img * s.c + c) * s.sh + yp) * s.sw + xp];
      }
    }
  }
  return g;
}

// the value at (c, y, x) of image b of the convolution's input grid; 0 outside it (the padding)
LPIPS_HD float tile_value(const Source &s, int b, int c, int y, int x) {
  if (y < 0 || y >= s.h || x < 0 || x >= s.w) return 0.f;
  if (s.mode == SRC_GRAD) {
    const float *plane = s.p0 + ((int64_t)b * s.c + c) * s.h * s.w;
    if (!(plane[(int64_t)y * s.w + x] > 0.f)) return 0.f;
    return grad_arriving(s, plane, b, c, y, x);
  }
  const bool first = b < s.n_first;
  const float *p = first ? s.p0 : s.p1;
  const int64_t img = first ? b : b - s.n_first;
  if (s.mode == SRC_IMAGE) return zscore(p[((img * s.c + c) * s.h + y) * s.w + x], s.mean[c], s.std[c]);
  if (s.mode == SRC_PLAIN) return p[((img * s.c + c) * s.h + y) * s.w + x];
  const float *o = p + ((img * s.c + c) * s.sh + 2 * y) * s.sw + 2 * x;   // 2 y + 1 < sh: h = sh / 2
  return max4(o[0], o[1], o[s.sw], o[s.sw + 1]);
}

// ---- the epilogues -------------------------------------------------------------------------------------------------------------------

enum { SINK_RELU = 0, SINK_PLAIN = 1, SINK_IMAGE = 2 };

// SINK_RELU   relu(acc + bias[m])      forward
// SINK_PLAIN  acc                      the gradient of a layer's input
// SINK_IMAGE  acc / std[m]             the gradient of the image (the z-score's derivative)
struct Sink {
  int32_t mode, n_first, m, h, w;
  float *o0, *o1;
  const float *bias;
  float std[3];
};

LPIPS_HD float sink_value(const Sink &k, int m, float acc) {
  if (k.mode == SINK_RELU) return relu(acc + k.bias[m]);
  if (k.mode == SINK_IMAGE) return acc / k.std[m];
  return acc;
}

LPIPS_HD float *sink_at(const Sink &k, int b, int m, int y, int x) {
  const bool first = b < k.n_first;
  const int64_t img = first ? b : b - k.n_first;
  return (first ? k.o0 : k.o1) + ((img * k.m + m) * k.h + y) * k.w + x;
}

// ---- the backward weights ------------------------------------------------------------------------------------------------------------

// element e of the backward layout [cin][cout][3][3] of a layer: flipped and transposed, so that the gradient of the input is the
// same convolution over it -> the index into the forward layout [cout][cin][3][3]
LPIPS_HD int64_t flipped_source(int cin, int cout, int64_t e) {
  const int t = (int)(e % 9);
  const int64_t co = (e / 9) % cout, ci = e / (9 * (int64_t)cout);
  return (co * cin + ci) * 9 + (8 - t);
}

// ---- the distance head -----------------------------------------------------------------------------------------------------------------

LPIPS_HD float sum_squares(const float *f, int c_count, int64_t stride) {
  float s = 0.f;
  for (int c = 0; c < c_count; ++c) s = fmaf(f[c * stride], f[c * stride], s);
  return s;
}

// one pixel of one tap: fx, fy point at channel 0 of the pixel, channels `stride` apart
LPIPS_HD float head_pixel(const float *fx, const float *fy, const float *w, int c_count, int64_t stride) {
  const float nx = sqrtf(sum_squares(fx, c_count, stride)) + EPS, ny = sqrtf(sum_squares(fy, c_count, stride)) + EPS;
  float s = 0.f;
  for (int c = 0; c < c_count; ++c) {
    const float d = fx[c * stride] / nx - fy[c * stride] / ny;
    s = fmaf(w[c] * d, d, s);
  }
  return s;
}

// d (scale * s) / d fx of one pixel, written to dfx (same strides).  A pixel whose fx is all zero contributes nothing (the
// reference's gradient there is NaN: 0 / 0 through sqrt).
LPIPS_HD void head_pixel_backward(const float *fx, const float *fy, const float *w, int c_count, int64_t stride, float scale, float *dfx) {
  const float r = sqrtf(sum_squares(fx, c_count, stride));
  if (r == 0.f) {
    for (int c = 0; c < c_count; ++c) dfx[c * stride] = 0.f;
    return;
  }
  const float nx = r + EPS, ny = sqrtf(sum_squares(fy, c_count, stride)) + EPS;
  float dot = 0.f;
  for (int c = 0; c < c_count; ++c) {
    const float a = 2.f * scale * w[c] * (fx[c * stride] / nx - fy[c * stride] / ny);
    dot = fmaf(a, fx[c * stride], dot);
  }
  const float pull = dot / (r * nx * nx);
  for (int c = 0; c < c_count; ++c) {
    const float a = 2.f * scale * w[c] * (fx[c * stride] / nx - fy[c * stride] / ny);
    dfx[c * stride] = fmaf(-fx[c * stride], pull, a / nx);
  }
}

LPIPS_HD int head_groups(int h, int w, int tap) {   // workgroups (slots) per image at a tap
  return (level_size(h, tap) * level_size(w, tap) + TPB - 1) / TPB;
}

// ---- the workspace (offsets in floats) ---------------------------------------------------------------------------------------------------

// keep = 1: the thirteen maps of x stay (backward reads their ReLU masks and pooling windows), with the five tap maps of y, the five
// tap gradients and two buffers the input gradients alternate between.  keep = 0: only the taps of either image stay until the head
// has run; every other map alternates between two buffers.
struct Workspace {
  int64_t x[LAYERS], y[LAYERS], dtap[TAPS], dgrad[2], part[TAPS], words;
};

LPIPS_HD int64_t map_words(int n, int h, int w, int L) {
  return (int64_t)n * layer_cout(L) * level_size(h, layer_level(L)) * level_size(w, layer_level(L));
}

LPIPS_HD Workspace workspace_layout(int n, int h, int w, int keep) {
  Workspace ws;
  int64_t at = 0;
  const int64_t big = (int64_t)n * 64 * h * w;   // no map and no input gradient is larger than layer 0's output
  auto take = [&at](int64_t count) { const int64_t here = at; at += (count + 63) & ~(int64_t)63; return here; };
  const int64_t ytmp[2] = {take(big), take(big)};
  int64_t xtmp[2] = {0, 0};
  if (!keep) { xtmp[0] = take(big); xtmp[1] = take(big); }
  int transient = 0;
  for (int L = 0; L < LAYERS; ++L) {
    if (tap_of(L) >= 0) {
      ws.x[L] = take(map_words(n, h, w, L));
      ws.y[L] = take(map_words(n, h, w, L));
    } else {
      ws.x[L] = keep ? take(map_words(n, h, w, L)) : xtmp[transient & 1];
      ws.y[L] = ytmp[transient & 1];
      ++transient;   // two transient layers in a row never share a buffer
    }
  }
  for (int t = 0; t < TAPS; ++t) {
    ws.dtap[t] = keep ? take(map_words(n, h, w, tap_layer(t))) : 0;
    ws.part[t] = take(2 * (int64_t)n * head_groups(h, w, t));   // one double per workgroup
  }
#ifdef LPIPS_POOL_KERNEL   // the A/B build of lpips.hip parks its pooled maps in these two buffers during the forward pass
  const bool scratch = true;
#else
  const bool scratch = keep != 0;
#endif
  ws.dgrad[0] = scratch ? take(big) : 0;
  ws.dgrad[1] = scratch ? take(big) : 0;
  ws.words = at;
  return ws;
}

}  // namespace lpips
