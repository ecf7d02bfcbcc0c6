// image_head.hip -- the image head of the appearance loop: what stands between the render call and the loss
// (train_appearance.py:126-127: the per-camera affine exp(cam_m) * render + cam_c, the product with the rasteriser's alpha
// and the clip to [0, 1]) with its gradient to all four tensors, and the forward-only maps of the evaluation side: the 8-bit
// frames of train_material_params.py:865-876, the ground-truth composition of train_appearance.py:108-110 and the metric
// inputs of eval.py:68-87.  Stand-alone maps on [dev] arrays like image_loss.hip: no context, no allocation, no
// synchronisation; every buffer, scratch included, is the caller's.  The per-pixel arithmetic is image_head_math.hpp.
//
// Every kernel has the same shape.  A lane takes a quad of four consecutive pixels of all three channels: mask as one
// 16-byte load, render as three, the image as three 16-byte stores (1 KiB per wave and instruction); the three exp(cam_m)
// and cam_c sit at a wave-uniform address.  Workgroup b of n = workgroups(H W) <= 1024 takes the quads b 256 + t,
// (b + n) 256 + t, ...  The 16-byte path needs H W % 4 == 0 and 16-byte aligned planes (then every plane of a [3, H, W]
// tensor is aligned too); otherwise the same quads are read and written pixel by pixel, bounds checked.  Nothing but HBM
// traffic: 28 bytes per pixel forward, 44 backward.  No LDS except for the fold of the six sums, no floating-point atomics:
// per-workgroup partials leave with plain stores and one workgroup folds them in index order.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "entry.hpp"
#include "image_head_math.hpp"

namespace {

using namespace entry;
using imghead::QUAD;
using imghead::SUMS;
using imghead::TPB;

constexpr int WAVES = TPB / 64;
static_assert(TPB == 256 && QUAD == 4 && SUMS == 6, "the quad layout above");

struct Quad {
  float v[QUAD];
};

// pixels p .. p + 3 of one plane; zero past the end of the plane (scalar path only: the 16-byte path has no partial quad)
template <bool VEC>
__device__ __forceinline__ Quad load_quad(const float *__restrict__ plane, int64_t p, int64_t hw) {
  Quad q;
  if (VEC) {
    const float4 f = *reinterpret_cast<const float4 *>(plane + p);
    q.v[0] = f.x; q.v[1] = f.y; q.v[2] = f.z; q.v[3] = f.w;
  } else {
#pragma unroll
    for (int k = 0; k < QUAD; ++k) q.v[k] = p + k < hw ? plane[p + k] : 0.0f;
  }
  return q;
}

template <bool VEC>
__device__ __forceinline__ void store_quad(float *__restrict__ plane, int64_t p, int64_t hw, const Quad &q) {
  if (VEC) {
    *reinterpret_cast<float4 *>(plane + p) = make_float4(q.v[0], q.v[1], q.v[2], q.v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < QUAD; ++k)
      if (p + k < hw) plane[p + k] = q.v[k];
  }
}

// twelve bytes, pixels p .. p + 3 of an [H, W, 3] byte image: b[3 k + c]
template <bool VEC>
__device__ __forceinline__ void load_bytes(const uint8_t *__restrict__ img, int64_t p, int64_t hw, uint8_t b[3 * QUAD]) {
  if (VEC) {
    const uint32_t *w = reinterpret_cast<const uint32_t *>(img + 3 * p);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const uint32_t x = w[i];
      b[4 * i] = (uint8_t)x; b[4 * i + 1] = (uint8_t)(x >> 8); b[4 * i + 2] = (uint8_t)(x >> 16); b[4 * i + 3] = (uint8_t)(x >> 24);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 3 * QUAD; ++i) b[i] = p + i / 3 < hw ? img[3 * p + i] : (uint8_t)0;
  }
}

// cam_m3, cam_c3: the three values of the camera's row, or NULL = the identity
__device__ __forceinline__ void camera_row(const float *__restrict__ cam_m3, const float *__restrict__ cam_c3, float a[3], float c[3]) {
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    a[ch] = cam_m3 ? expf(cam_m3[ch]) : 1.0f;
    c[ch] = cam_m3 ? cam_c3[ch] : 0.0f;
  }
}

// Sum of one double per lane over the workgroup in a fixed order, as block_sum3 of image_loss.hip.  Valid in thread 0 only.
__device__ __forceinline__ void block_sum3(double &a, double &b, double &c, double (*red)[WAVES]) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_down(a, off);
    b += __shfl_down(b, off);
    c += __shfl_down(c, off);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[0][wave] = a; red[1][wave] = b; red[2][wave] = c; }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = red[0][0]; b = red[1][0]; c = red[2][0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) { a += red[0][w]; b += red[1][w]; c += red[2][w]; }
  }
}

// render [3 * hw], mask [hw], image [3 * hw]
template <bool VEC>
__global__ __launch_bounds__(TPB) void k_image_head_forward(const float *__restrict__ render, const float *__restrict__ mask,
                                                            const float *__restrict__ cam_m3, const float *__restrict__ cam_c3, int64_t hw,
                                                            float *__restrict__ image) {
  float a[3], c[3];
  camera_row(cam_m3, cam_c3, a, c);
  const int64_t n_quads = (hw + QUAD - 1) / QUAD;
  for (int64_t q = (int64_t)blockIdx.x * TPB + threadIdx.x; q < n_quads; q += (int64_t)gridDim.x * TPB) {
    const int64_t p = q * QUAD;
    const Quad m = load_quad<VEC>(mask, p, hw);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const Quad r = load_quad<VEC>(render + ch * hw, p, hw);
      Quad o;
#pragma unroll
      for (int k = 0; k < QUAD; ++k) o.v[k] = imghead::clip01(imghead::value(r.v[k], a[ch], c[ch], m.v[k]));
      store_quad<VEC>(image + ch * hw, p, hw, o);
    }
  }
}

// The map of the backward pass and the per-workgroup partials of the six sums.  g_image, d_render, d_mask and partials may
// each be NULL (zeros upstream / not wanted); partials [gridDim.x * SUMS].
template <bool VEC>
__global__ __launch_bounds__(TPB) void k_image_head_backward(const float *__restrict__ render, const float *__restrict__ mask,
                                                             const float *__restrict__ cam_m3, const float *__restrict__ cam_c3, int64_t hw,
                                                             const float *__restrict__ g_image, float *__restrict__ d_render,
                                                             float *__restrict__ d_mask, double *__restrict__ partials) {
  __shared__ double red[3][WAVES];
  float a[3], c[3];
  camera_row(cam_m3, cam_c3, a, c);
  double s_c[3] = {0.0, 0.0, 0.0}, s_m[3] = {0.0, 0.0, 0.0};
  const int64_t n_quads = (hw + QUAD - 1) / QUAD;
  for (int64_t q = (int64_t)blockIdx.x * TPB + threadIdx.x; q < n_quads; q += (int64_t)gridDim.x * TPB) {
    const int64_t p = q * QUAD;
    const Quad m = load_quad<VEC>(mask, p, hw);
    float t[3][QUAD];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const Quad r = load_quad<VEC>(render + ch * hw, p, hw);
      Quad g;
      if (g_image) {
        g = load_quad<VEC>(g_image + ch * hw, p, hw);
      } else {
#pragma unroll
        for (int k = 0; k < QUAD; ++k) g.v[k] = 0.0f;
      }
      Quad dr;
#pragma unroll
      for (int k = 0; k < QUAD; ++k) {
        const imghead::PixelGrad pg = imghead::pixel_grad(r.v[k], a[ch], c[ch], m.v[k], g.v[k]);
        dr.v[k] = pg.d_render;
        t[ch][k] = pg.d_mask;
        s_c[ch] += (double)pg.s_c;
        s_m[ch] += (double)pg.s_m;
      }
      if (d_render) store_quad<VEC>(d_render + ch * hw, p, hw, dr);
    }
    if (d_mask) {
      Quad dm;
#pragma unroll
      for (int k = 0; k < QUAD; ++k) dm.v[k] = imghead::mask_grad(t[0][k], t[1][k], t[2][k]);
      store_quad<VEC>(d_mask, p, hw, dm);
    }
  }
  if (!partials) return;  // uniform over the grid
  block_sum3(s_c[0], s_c[1], s_c[2], red);
  __syncthreads();        // red is used again
  block_sum3(s_m[0], s_m[1], s_m[2], red);
  if (threadIdx.x == 0) {
    double *o = partials + (size_t)blockIdx.x * SUMS;
    o[0] = s_c[0]; o[1] = s_c[1]; o[2] = s_c[2]; o[3] = s_m[0]; o[4] = s_m[1]; o[5] = s_m[2];
  }
}

// One workgroup: lane t adds the partials of workgroups t, t + 256, ... in that order, the lanes are folded as in
// block_sum3, and both [n_cam, 3] outputs (either may be NULL) are written in full, zeros off the camera's row.
__global__ __launch_bounds__(TPB) void k_image_head_fold(const double *__restrict__ partials, int32_t n_wg, const float *__restrict__ cam_m,
                                                         int32_t n_cam, int32_t cam, float *__restrict__ d_cam_m,
                                                         float *__restrict__ d_cam_c) {
  __shared__ double red[3][WAVES];
  __shared__ float row[SUMS];  // d_cam_c[cam][0..2], d_cam_m[cam][0..2]
  double s[SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int32_t w = threadIdx.x; w < n_wg; w += TPB) {
#pragma unroll
    for (int k = 0; k < SUMS; ++k) s[k] += partials[(size_t)w * SUMS + k];
  }
  block_sum3(s[0], s[1], s[2], red);
  __syncthreads();
  block_sum3(s[3], s[4], s[5], red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      row[ch] = (float)s[ch];
      row[3 + ch] = (float)((double)expf(cam_m[3 * (size_t)cam + ch]) * s[3 + ch]);
    }
  }
  __syncthreads();
  for (int32_t i = threadIdx.x; i < 3 * n_cam; i += TPB) {
    const int32_t r = i / 3, ch = i - 3 * r;
    if (d_cam_c) d_cam_c[i] = r == cam ? row[ch] : 0.0f;
    if (d_cam_m) d_cam_m[i] = r == cam ? row[3 + ch] : 0.0f;
  }
}

// out_u8 [hw * 3], HWC
template <bool VEC>
__global__ __launch_bounds__(TPB) void k_image_head_bytes(const float *__restrict__ render, const float *__restrict__ mask,
                                                          const float *__restrict__ cam_m3, const float *__restrict__ cam_c3, bool white,
                                                          int64_t hw, uint8_t *__restrict__ out_u8) {
  float a[3], c[3];
  camera_row(cam_m3, cam_c3, a, c);
  const int64_t n_quads = (hw + QUAD - 1) / QUAD;
  for (int64_t q = (int64_t)blockIdx.x * TPB + threadIdx.x; q < n_quads; q += (int64_t)gridDim.x * TPB) {
    const int64_t p = q * QUAD;
    const Quad m = load_quad<VEC>(mask, p, hw);
    uint8_t b[3 * QUAD];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const Quad r = load_quad<VEC>(render + ch * hw, p, hw);
#pragma unroll
      for (int k = 0; k < QUAD; ++k) b[3 * k + ch] = imghead::frame_byte(r.v[k], a[ch], c[ch], m.v[k], white);
    }
    if (VEC) {
      uint32_t *w = reinterpret_cast<uint32_t *>(out_u8 + 3 * p);
#pragma unroll
      for (int i = 0; i < 3; ++i)
        w[i] = (uint32_t)b[4 * i] | (uint32_t)b[4 * i + 1] << 8 | (uint32_t)b[4 * i + 2] << 16 | (uint32_t)b[4 * i + 3] << 24;
    } else {
#pragma unroll
      for (int i = 0; i < 3 * QUAD; ++i)
        if (p + i / 3 < hw) out_u8[3 * p + i] = b[i];
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(TPB) void k_image_compose(const float *__restrict__ rgb, const float *__restrict__ msk, bool white, int64_t hw,
                                                       float *__restrict__ out) {
  const int64_t n_quads = (hw + QUAD - 1) / QUAD;
  for (int64_t q = (int64_t)blockIdx.x * TPB + threadIdx.x; q < n_quads; q += (int64_t)gridDim.x * TPB) {
    const int64_t p = q * QUAD;
    const Quad m = load_quad<VEC>(msk, p, hw);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const Quad r = load_quad<VEC>(rgb + ch * hw, p, hw);
      Quad o;
#pragma unroll
      for (int k = 0; k < QUAD; ++k) o.v[k] = imghead::compose(r.v[k], m.v[k], white);
      store_quad<VEC>(out + ch * hw, p, hw, o);
    }
  }
}

// pred_u8, gt_u8 [hw * 3] HWC; mask [hw]; out_pred, out_gt [3 * hw] CHW
template <bool VEC>
__global__ __launch_bounds__(TPB) void k_eval_pair(const uint8_t *__restrict__ pred_u8, const uint8_t *__restrict__ gt_u8,
                                                   const float *__restrict__ mask, bool remove_white, int64_t hw, float *__restrict__ out_pred,
                                                   float *__restrict__ out_gt) {
  const int64_t n_quads = (hw + QUAD - 1) / QUAD;
  for (int64_t q = (int64_t)blockIdx.x * TPB + threadIdx.x; q < n_quads; q += (int64_t)gridDim.x * TPB) {
    const int64_t p = q * QUAD;
    const Quad m = load_quad<VEC>(mask, p, hw);
#pragma unroll
    for (int img = 0; img < 2; ++img) {
      uint8_t b[3 * QUAD];
      load_bytes<VEC>(img ? gt_u8 : pred_u8, p, hw, b);
      Quad o[3];
#pragma unroll
      for (int k = 0; k < QUAD; ++k) {
        float f[3];
        imghead::eval_pixel(b + 3 * k, m.v[k], remove_white, f);
        o[0].v[k] = f[0]; o[1].v[k] = f[1]; o[2].v[k] = f[2];
      }
      float *out = img ? out_gt : out_pred;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) store_quad<VEC>(out + ch * hw, p, hw, o[ch]);
    }
  }
}

bool sizes_ok(int32_t H, int32_t W) { return H > 0 && W > 0 && (int64_t)H * W <= INT32_MAX; }

bool camera_ok(const float *cam_m, const float *cam_c, int32_t n_cam, int32_t cam) {
  return cam_m && cam_c && n_cam > 0 && cam >= 0 && cam < n_cam;
}

// the 16-byte path: whole quads, and every plane (p + k * hw floats, hw * 3 bytes) as aligned as its base
template <typename... P>
bool vec_ok(int64_t hw, P... ptrs) {
  return hw % QUAD == 0 && ((... | (uintptr_t)ptrs) & 15) == 0;
}

}  // namespace

extern "C" {

int mpmhip_image_head_forward(int32_t device, void *stream, const float *render, const float *mask, const float *cam_m, const float *cam_c,
                              int32_t n_cam, int32_t cam, int32_t H, int32_t W, float *out_image) {
  if (!sizes_ok(H, W) || !render || !mask || !camera_ok(cam_m, cam_c, n_cam, cam) || !out_image) return MPMHIP_ERR_INVALID;
  if (int rc = select_device(device)) return rc;
  const int64_t hw = (int64_t)H * W;
  const unsigned grid = (unsigned)imghead::workgroups(hw);
  const float *m3 = cam_m + 3 * (size_t)cam, *c3 = cam_c + 3 * (size_t)cam;
  hipStream_t s = (hipStream_t)stream;
  if (vec_ok(hw, render, mask, out_image))
    hipLaunchKernelGGL(k_image_head_forward<true>, grid, TPB, 0, s, render, mask, m3, c3, hw, out_image);
  else
    hipLaunchKernelGGL(k_image_head_forward<false>, grid, TPB, 0, s, render, mask, m3, c3, hw, out_image);
  return check(hipGetLastError());
}

int mpmhip_image_head_backward(int32_t device, void *stream, const float *render, const float *mask, const float *cam_m, const float *cam_c,
                               int32_t n_cam, int32_t cam, int32_t H, int32_t W, const float *g_image, double *scratch, float *d_render,
                               float *d_mask, float *d_cam_m, float *d_cam_c) {
  const bool sums = d_cam_m || d_cam_c;
  if (!sizes_ok(H, W) || !render || !mask || !camera_ok(cam_m, cam_c, n_cam, cam) || (sums && !scratch)) return MPMHIP_ERR_INVALID;
  if (int rc = select_device(device)) return rc;
  if (!sums && !d_render && !d_mask) return MPMHIP_OK;
  const int64_t hw = (int64_t)H * W;
  const int32_t n_wg = imghead::workgroups(hw);
  const float *m3 = cam_m + 3 * (size_t)cam, *c3 = cam_c + 3 * (size_t)cam;
  double *partials = sums ? scratch : nullptr;
  hipStream_t s = (hipStream_t)stream;
  if (vec_ok(hw, render, mask, g_image, d_render, d_mask))
    hipLaunchKernelGGL(k_image_head_backward<true>, (unsigned)n_wg, TPB, 0, s, render, mask, m3, c3, hw, g_image, d_render, d_mask, partials);
  else
    hipLaunchKernelGGL(k_image_head_backward<false>, (unsigned)n_wg, TPB, 0, s, render, mask, m3, c3, hw, g_image, d_render, d_mask, partials);
  if (sums) hipLaunchKernelGGL(k_image_head_fold, 1, TPB, 0, s, (const double *)scratch, n_wg, cam_m, n_cam, cam, d_cam_m, d_cam_c);
  return check(hipGetLastError());
}

int mpmhip_image_head_bytes(int32_t device, void *stream, const float *render, const float *mask, const float *cam_m, const float *cam_c,
                            int32_t n_cam, int32_t cam, int32_t white, int32_t H, int32_t W, uint8_t *out_u8) {
  const bool identity = !cam_m && !cam_c;
  if (!sizes_ok(H, W) || !render || !mask || !(identity || camera_ok(cam_m, cam_c, n_cam, cam)) || !out_u8) return MPMHIP_ERR_INVALID;
  if (int rc = select_device(device)) return rc;
  const int64_t hw = (int64_t)H * W;
  const unsigned grid = (unsigned)imghead::workgroups(hw);
  const float *m3 = identity ? nullptr : cam_m + 3 * (size_t)cam, *c3 = identity ? nullptr : cam_c + 3 * (size_t)cam;
  hipStream_t s = (hipStream_t)stream;
  if (vec_ok(hw, render, mask, out_u8))
    hipLaunchKernelGGL(k_image_head_bytes<true>, grid, TPB, 0, s, render, mask, m3, c3, white != 0, hw, out_u8);
  else
    hipLaunchKernelGGL(k_image_head_bytes<false>, grid, TPB, 0, s, render, mask, m3, c3, white != 0, hw, out_u8);
  return check(hipGetLastError());
}

int mpmhip_image_compose(int32_t device, void *stream, const float *rgb, const float *msk, int32_t white, int32_t H, int32_t W, float *out) {
  if (!sizes_ok(H, W) || !rgb || !msk || !out) return MPMHIP_ERR_INVALID;
  if (int rc = select_device(device)) return rc;
  const int64_t hw = (int64_t)H * W;
  const unsigned grid = (unsigned)imghead::workgroups(hw);
  hipStream_t s = (hipStream_t)stream;
  if (vec_ok(hw, rgb, msk, out))
    hipLaunchKernelGGL(k_image_compose<true>, grid, TPB, 0, s, rgb, msk, white != 0, hw, out);
  else
    hipLaunchKernelGGL(k_image_compose<false>, grid, TPB, 0, s, rgb, msk, white != 0, hw, out);
  return check(hipGetLastError());
}

int mpmhip_eval_pair(int32_t device, void *stream, const uint8_t *pred_u8, const uint8_t *gt_u8, const float *mask, int32_t remove_white,
                     int32_t H, int32_t W, float *out_pred, float *out_gt) {
  if (!sizes_ok(H, W) || !pred_u8 || !gt_u8 || !mask || !out_pred || !out_gt) return MPMHIP_ERR_INVALID;
  if (int rc = select_device(device)) return rc;
  const int64_t hw = (int64_t)H * W;
  const unsigned grid = (unsigned)imghead::workgroups(hw);
  hipStream_t s = (hipStream_t)stream;
  if (vec_ok(hw, pred_u8, gt_u8, mask, out_pred, out_gt))
    hipLaunchKernelGGL(k_eval_pair<true>, grid, TPB, 0, s, pred_u8, gt_u8, mask, remove_white != 0, hw, out_pred, out_gt);
  else
    hipLaunchKernelGGL(k_eval_pair<false>, grid, TPB, 0, s, pred_u8, gt_u8, mask, remove_white != 0, hw, out_pred, out_gt);
  return check(hipGetLastError());
}

}  // extern "C"
