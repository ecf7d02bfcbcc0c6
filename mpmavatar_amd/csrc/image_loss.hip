// image_loss.hip -- the loss between the render call and loss.backward() of the appearance loop
// (/root/reference/train_appearance.py:132-134: (1 - lambda) l1_loss + lambda (1 - ssim), utils/loss_utils.py:18-64) and the
// image metrics every run ends with (eval.py:89-91: psnr of utils/image_utils.py:17-19, ssim), as three kernels: one fused
// forward (L1, squared error and the SSIM map with its three partial maps from one read of both images), one reduction
// to per-plane means, one backward (three separable convolutions of the partial maps and the closed forms of L1 / MSE).
// Stand-alone maps on [dev] arrays like geo.hip: no context, no allocation, no synchronisation; every buffer, scratch
// included, is the caller's.  A "plane" is one (batch, channel) image; all work is per plane.
//
// One 256-thread workgroup per 16 x 16 output tile.  The 26 x 26 halo of the inputs sits in LDS with a row stride of
// HS = 48 dwords: ds_read_b32 banks are (address / 4) mod 32 per 32-lane half, a half covers two tile rows of 16 columns,
// and 48 = 16 mod 32 puts those two rows on disjoint banks at every tap (26 would make them overlap: two-way conflicts).
// The horizontal pass leaves 26 rows x 16 columns per quantity at stride 16, which has the same property for the vertical
// pass.  No floating-point atomics: the tile sums are folded in a fixed order and written with plain stores, the same input
// gives the same bits.  Measured numbers: DESIGN.md section 14.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "entry.hpp"
#include "image_loss_math.hpp"

namespace {

using namespace entry;
using imgloss::HALO;
using imgloss::RAD;
using imgloss::TILE;

constexpr int TPB = TILE * TILE;  // 256: four waves
constexpr int WAVES = TPB / 64;
constexpr int HS = 48;            // halo row stride in dwords: >= HALO and = 16 mod 32
static_assert(HS >= HALO && HS % 32 == 16 && TILE == 16 && TPB == 256, "the bank layout above");

struct TilePos {
  int plane, y0, x0;  // first output pixel of the tile
};

__device__ __forceinline__ TilePos tile_pos(int tiles_x, int tiles_per_plane) {
  const int plane = (int)(blockIdx.x / (unsigned)tiles_per_plane);
  const int t = (int)(blockIdx.x - (unsigned)plane * (unsigned)tiles_per_plane);
  return TilePos{plane, (t / tiles_x) * TILE, (t % tiles_x) * TILE};
}

// dst[r * HS + c] = src(y0 - RAD + r, x0 - RAD + c) for the 26 x 26 halo, zero outside the H x W plane
__device__ __forceinline__ void load_halo(float *dst, const float *__restrict__ src, int y0, int x0, int H, int W) {
  for (int i = threadIdx.x; i < HALO * HALO; i += TPB) {
    const int r = i / HALO, c = i - r * HALO;
    const int gy = y0 - RAD + r, gx = x0 - RAD + c;
    const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
    dst[r * HS + c] = in ? src[(size_t)gy * W + gx] : 0.0f;
  }
}

// Sum of one double per lane over the workgroup in a fixed order: shuffles within each wave (lane l += lane l + off,
// off = 32 .. 1), then lane 0 of wave 0 adds the four wave sums in wave order.  Valid in thread 0 only.
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

// img, gt [planes * H * W]; maps [planes * 3 * H * W] (d_mu, d_s1, d_s12 of each plane, one H x W plane each) or NULL;
// tile_sums [gridDim.x * 3] doubles: sum |d|, sum d^2, sum m over the tile's pixels inside the image.
__global__ __launch_bounds__(TPB) void k_image_loss_forward(const float *__restrict__ img, const float *__restrict__ gt, int H, int W,
                                                            int tiles_x, int tiles_per_plane, float *__restrict__ maps,
                                                            double *__restrict__ tile_sums) {
  __shared__ float sx[HALO * HS], sy[HALO * HS];
  __shared__ float hm[5][HALO * TILE];
  __shared__ double red[3][WAVES];
  const TilePos tp = tile_pos(tiles_x, tiles_per_plane);
  const size_t plane_off = (size_t)tp.plane * H * W;
  load_halo(sx, img + plane_off, tp.y0, tp.x0, H, W);
  load_halo(sy, gt + plane_off, tp.y0, tp.x0, H, W);
  __syncthreads();
  for (int i = threadIdx.x; i < HALO * TILE; i += TPB) {  // horizontal pass: 26 rows x 16 columns
    const int r = i / TILE, c = i % TILE;
    const imgloss::Moments h = imgloss::row_moments(&sx[r * HS + c], &sy[r * HS + c]);
    hm[0][i] = h.x; hm[1][i] = h.y; hm[2][i] = h.xx; hm[3][i] = h.yy; hm[4][i] = h.xy;
  }
  __syncthreads();
  const int ty = threadIdx.x / TILE, tx = threadIdx.x % TILE;
  const int at = ty * TILE + tx;  // vertical pass: rows ty .. ty + 10 of the horizontal sums
  const imgloss::Moments e{imgloss::taps(&hm[0][at], TILE), imgloss::taps(&hm[1][at], TILE), imgloss::taps(&hm[2][at], TILE),
                           imgloss::taps(&hm[3][at], TILE), imgloss::taps(&hm[4][at], TILE)};
  const imgloss::Point p = imgloss::point(e);
  const int gy = tp.y0 + ty, gx = tp.x0 + tx;
  const bool in = gy < H && gx < W;
  const float d = sx[(ty + RAD) * HS + tx + RAD] - sy[(ty + RAD) * HS + tx + RAD];
  double s_abs = in ? (double)__builtin_fabsf(d) : 0.0, s_sq = in ? (double)(d * d) : 0.0, s_m = in ? (double)p.m : 0.0;
  if (maps && in) {
    const size_t hw = (size_t)H * W, o = (size_t)tp.plane * 3 * hw + (size_t)gy * W + gx;
    maps[o] = p.d_mu; maps[o + hw] = p.d_s1; maps[o + 2 * hw] = p.d_s12;
  }
  block_sum3(s_abs, s_sq, s_m, red);
  if (threadIdx.x == 0) {
    double *o = tile_sums + (size_t)blockIdx.x * 3;
    o[0] = s_abs; o[1] = s_sq; o[2] = s_m;
  }
}

// One workgroup per plane: lane t adds the plane's tile triples t, t + 256, ... in that order, the lanes are folded as in
// block_sum3, and the three means over H x W leave as fp32: out[plane * 3 + {0, 1, 2}] = mean |d|, mean d^2, mean m.
__global__ __launch_bounds__(TPB) void k_image_loss_reduce(const double *__restrict__ tile_sums, int tiles_per_plane, double n_pixels,
                                                           float *__restrict__ out) {
  __shared__ double red[3][WAVES];
  const double *s = tile_sums + (size_t)blockIdx.x * tiles_per_plane * 3;
  double a = 0.0, b = 0.0, c = 0.0;
  for (int t = threadIdx.x; t < tiles_per_plane; t += TPB) { a += s[3 * (size_t)t]; b += s[3 * (size_t)t + 1]; c += s[3 * (size_t)t + 2]; }
  block_sum3(a, b, c, red);
  if (threadIdx.x == 0) {
    float *o = out + (size_t)blockIdx.x * 3;
    o[0] = (float)(a / n_pixels); o[1] = (float)(b / n_pixels); o[2] = (float)(c / n_pixels);
  }
}

// d_img(q) = (g_l1[p] sign(x - y) + g_mse[p] 2 (x - y) + g_ssim[p] ((w * d_mu) + 2 x (w * d_s1) + y (w * d_s12))(q)) / (H W)
__global__ __launch_bounds__(TPB) void k_image_loss_backward(const float *__restrict__ img, const float *__restrict__ gt, int H, int W,
                                                             int tiles_x, int tiles_per_plane, const float *__restrict__ maps,
                                                             const float *__restrict__ g_l1, const float *__restrict__ g_mse,
                                                             const float *__restrict__ g_ssim, float inv_n, float *__restrict__ d_img) {
  __shared__ float sm[3][HALO * HS];
  __shared__ float hc[3][HALO * TILE];
  const TilePos tp = tile_pos(tiles_x, tiles_per_plane);
  const size_t hw = (size_t)H * W;
#pragma unroll
  for (int k = 0; k < 3; ++k) load_halo(sm[k], maps + ((size_t)tp.plane * 3 + k) * hw, tp.y0, tp.x0, H, W);
  __syncthreads();
  for (int i = threadIdx.x; i < HALO * TILE; i += TPB) {
    const int r = i / TILE, c = i % TILE;
#pragma unroll
    for (int k = 0; k < 3; ++k) hc[k][i] = imgloss::taps(&sm[k][r * HS + c], 1);
  }
  __syncthreads();
  const int ty = threadIdx.x / TILE, tx = threadIdx.x % TILE;
  const int gy = tp.y0 + ty, gx = tp.x0 + tx;
  if (gy >= H || gx >= W) return;
  const int at = ty * TILE + tx;
  const float c_mu = imgloss::taps(&hc[0][at], TILE), c_s1 = imgloss::taps(&hc[1][at], TILE), c_s12 = imgloss::taps(&hc[2][at], TILE);
  const size_t o = (size_t)tp.plane * hw + (size_t)gy * W + gx;
  d_img[o] = imgloss::pixel_grad(img[o], gt[o], c_mu, c_s1, c_s12, g_l1[tp.plane], g_mse[tp.plane], g_ssim[tp.plane], inv_n);
}

bool sizes_ok(int32_t planes, int32_t H, int32_t W) {
  return planes > 0 && H > 0 && W > 0 && (int64_t)planes * H * W <= INT32_MAX;  // H * W alone cannot overflow 64 bits
}

}  // namespace

extern "C" {

int mpmhip_image_loss_forward(int32_t device, void *stream, const float *img, const float *gt, int32_t planes, int32_t H, int32_t W,
                              float *maps, double *scratch, float *out_means) {
  if (!sizes_ok(planes, H, W) || !img || !gt || !scratch || !out_means) return MPMHIP_ERR_INVALID;
  if (int rc = select_device(device)) return rc;
  const int tiles_x = (W + TILE - 1) / TILE, tiles_per_plane = tiles_x * ((H + TILE - 1) / TILE);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_image_loss_forward, (unsigned)((int64_t)planes * tiles_per_plane), TPB, 0, s, img, gt, H, W, tiles_x, tiles_per_plane,
                     maps, scratch);
  hipLaunchKernelGGL(k_image_loss_reduce, (unsigned)planes, TPB, 0, s, (const double *)scratch, tiles_per_plane, (double)H * (double)W,
                     out_means);
  return check(hipGetLastError());
}

int mpmhip_image_loss_backward(int32_t device, void *stream, const float *img, const float *gt, int32_t planes, int32_t H, int32_t W,
                               const float *maps, const float *g_l1, const float *g_mse, const float *g_ssim, float *d_img) {
  if (!sizes_ok(planes, H, W) || !img || !gt || !maps || !g_l1 || !g_mse || !g_ssim || !d_img) return MPMHIP_ERR_INVALID;
  if (int rc = select_device(device)) return rc;
  const int tiles_x = (W + TILE - 1) / TILE, tiles_per_plane = tiles_x * ((H + TILE - 1) / TILE);
  hipLaunchKernelGGL(k_image_loss_backward, (unsigned)((int64_t)planes * tiles_per_plane), TPB, 0, (hipStream_t)stream, img, gt, H, W,
                     tiles_x, tiles_per_plane, maps, g_l1, g_mse, g_ssim, (float)(1.0 / ((double)H * (double)W)), d_img);
  return check(hipGetLastError());
}

}  // extern "C"
