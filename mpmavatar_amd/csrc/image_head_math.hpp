// image_head_math.hpp -- the per-pixel statements of the image head: the expression between the render call and the loss of
// the appearance loop (train_appearance.py:126-127, again at :206-207 and in train_material_params.py:865-870),
//   image = ((render * exp(cam_m[idx]) + cam_c[idx]) * mask).clip(0, 1),
// its gradient, the 8-bit frames of train_material_params.py:865-876 and the metric inputs of eval.py:68-87.  Plain C++ for
// the device and the host alike: tests/hostimagehead/ compiles it with g++ over the stand-in for <hip/hip_runtime.h>.
//
// THE GRADIENT.  With a_c = exp(cam_m[idx][c]), v = (render[c] a_c + cam_c[idx][c]) mask and the upstream gradient g of the
// clipped image, g_v = g where 0 <= v <= 1 and 0 elsewhere -- TORCH's slope of clip(0., 1.), both ends included (at v = 0.0,
// -0.0 and 1.0 its gradient is 1), not the "zero where a clamp binds" rule of this project's own kernels: every pixel with
// mask == 0 has v == 0 exactly and still hands a gradient to mask.
//   d_render[c]      = g_v mask a_c
//   d_mask           = sum_c g_v[c] (render[c] a_c + cam_c[idx][c])
//   d_cam_c[idx][c]  = sum_pixels g_v[c] mask
//   d_cam_m[idx][c]  = a_c sum_pixels g_v[c] mask render[c]
// The backward pass recomputes v with value(), the forward's own function, and no contraction is allowed in it: the pass
// decision is then the forward's, bit for bit, and no flag map is stored.
//
// THE SUMS.  The six pixel sums have fp32 terms and fp64 additions.  Pixels are dealt out in quads of QUAD consecutive pixels;
// workgroup b of n = workgroups(H W) takes the quads b TPB + t, (b + n) TPB + t, ... for its lane t, so the partition depends on
// H W alone.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace imghead {

constexpr int TPB = 256;                   // lanes per workgroup
constexpr int QUAD = 4;                    // consecutive pixels per lane and pass: one 16-byte access per plane
constexpr int WG_PIXELS = TPB * QUAD;      // 1024
constexpr int MAX_WORKGROUPS = 1024;       // beyond 1024 x 1024 pixels the workgroups stride over the image
constexpr int SUMS = 6;                    // per workgroup: sum g_v mask [3], then sum g_v mask render [3]
constexpr int WHITE_SUM = 689;             // eval.py:73: mean of three bytes / 255 > 0.90  <=>  their sum >= 689

// MPMHIP_IMAGE_HEAD_WORKGROUPS of include/mpmhip.h
__host__ __device__ __forceinline__ int32_t workgroups(int64_t n_pixels) {
  const int64_t w = (n_pixels + WG_PIXELS - 1) / WG_PIXELS;
  return (int32_t)(w < MAX_WORKGROUPS ? w : MAX_WORKGROUPS);
}

// render * a + c, each operation rounded on its own as torch's two launches round them
__host__ __device__ __forceinline__ float affine(float r, float a, float c) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float p = r * a;
  return p + c;
}

// the unclipped value: forward and backward pass both call this
__host__ __device__ __forceinline__ float value(float r, float a, float c, float m) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return affine(r, a, c) * m;
}

// torch's clamp(0, 1): NaN fails both comparisons and leaves as NaN
__host__ __device__ __forceinline__ float clip01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }

// torch's clamp backward: the gradient passes on the closed interval
__host__ __device__ __forceinline__ bool passes(float v) { return v >= 0.f && v <= 1.f; }

struct PixelGrad {
  float d_render;  // g_v mask a
  float d_mask;    // g_v (render a + c): one channel's share
  float s_c;       // g_v mask: the term of d_cam_c
  float s_m;       // g_v mask render: the term of d_cam_m before the factor a
};

__host__ __device__ __forceinline__ PixelGrad pixel_grad(float r, float a, float c, float m, float g) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float gv = passes(value(r, a, c, m)) ? g : 0.f;
  const float gm = gv * m;
  return PixelGrad{gm * a, gv * affine(r, a, c), gm, gm * r};
}

// the three channel shares of d_mask in channel order
__host__ __device__ __forceinline__ float mask_grad(float t0, float t1, float t2) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return (t0 + t1) + t2;
}

// train_material_params.py:865-870 at one channel of one pixel: the byte of (clamp(r, 0, 1) * 255.).astype(np.uint8), the
// product in fp32, truncated toward zero.  NaN gives 0.
__host__ __device__ __forceinline__ uint8_t frame_byte(float r, float a, float c, float m, bool white) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float v = value(r, a, c, m);
  if (white) v = v + (1.0f - m);
  v = v > 0.f ? (v > 1.f ? 1.f : v) : 0.f;
  return (uint8_t)(int32_t)(v * 255.0f);
}

// train_appearance.py:108-110: rgb * msk (+ (1 - msk)), not clipped
__host__ __device__ __forceinline__ float compose(float rgb, float m, bool white) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float v = rgb * m;
  return white ? v + (1.0f - m) : v;
}

// eval.py:68-87 at one pixel of one image: bytes -> floats by a true division (a product with 1 / 255 differs at 126 of the
// 256 values), the white rule in integers, the mask
__host__ __device__ __forceinline__ void eval_pixel(const uint8_t rgb[3], float m, bool remove_white, float out[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const bool white = remove_white && (int32_t)rgb[0] + (int32_t)rgb[1] + (int32_t)rgb[2] >= WHITE_SUM;
#pragma unroll
  for (int c = 0; c < 3; ++c) out[c] = (white ? 0.0f : (float)rgb[c] / 255.0f) * m;
}

}  // namespace imghead
