// raster_extra.hip -- extra attribute channels through the Gaussian rasteriser, forward and backward: the extra_attrs argument
// and the sixth slot of the render call of the reference's 4D-DRESS tracking script (preprocess/train_mesh_lbs_4ddress.py:260-277,
// :299, :306: the [N, 2] garment labelling rendered to a garment mask and compared with the data's).  The math is
// raster_extra_math.hpp; this file is one more walk over tile lists that the colour pass has already sorted, in both directions:
//
//   k_raster_extra_forward         one workgroup of 256 lanes per 16 x 16 tile walks [range.x, pix_stop) of the list the colour
//                                  pass of the same frame just sorted and writes extra [E, H, W]
//   k_raster_extra_backward_tiles  the back-to-front walk of k_raster_backward_tiles for the extras: per entry the six geometry /
//                                  opacity partials are ADDED into the row the colour tile kernel has written, the E attribute
//                                  partials go to a row buffer of their own
//   k_raster_extra_gather          one lane per (Gaussian, channel) sums the attribute rows through the inverse map
//
// between the stages of mpmhip_raster_backward (raster_state.hpp), which run unchanged.  No floating-point atomics: an entry
// belongs to one tile, so its row is read and written by one lane of one workgroup, after the colour tile kernel on the same
// stream; a Gaussian's rows are added in the order of its rectangle.  The same input gives the same bits.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "raster_extra_math.hpp"
#include "raster_state.hpp"

namespace {

using namespace raster_host;
constexpr int NP = rast::N_PARTIALS;
constexpr int NG = rast::N_GEOM;
constexpr int WAVES = TPB / 64;

// Lane t = pixel (t % 16, t / 16) of the tile, batches of TPB records staged in LDS, as in k_raster_render.  A lane walks the
// entries below its own stop: the position at which the colour walk finished the pixel (or the end of the tile's range), read
// from pix_stop and clamped into the range.  Lanes outside the image stop at once but stage and meet every barrier.  Every
// element of `out` is written.  `total` and `n` only bound what the kernel can touch.
template <int E>
__global__ __launch_bounds__(TPB) void k_raster_extra_forward(int W, int H, int gx, uint32_t total, uint32_t n,
                                                              const uint2 *__restrict__ ranges, const uint32_t *__restrict__ vals,
                                                              const float4 *__restrict__ rec0, const float4 *__restrict__ rec1,
                                                              const float *__restrict__ extra, const uint32_t *__restrict__ pix_stop,
                                                              float *out) {
  __shared__ float4 s0[TPB], s1[TPB];
  __shared__ float sx[TPB][E];
  const int t = threadIdx.x;
  const int x = blockIdx.x * TILE + (t % TILE), y = blockIdx.y * TILE + (t / TILE);
  const bool inside = x < W && y < H;
  uint2 range = ranges[blockIdx.y * gx + blockIdx.x];
  range.y = min(range.y, total);
  range.x = min(range.x, range.y);
  const float fx = (float)x, fy = (float)y;
  const size_t at = (size_t)y * W + x, plane = (size_t)W * H;
  uint32_t stop = range.x;
  if (inside) stop = min(max(pix_stop[at], range.x), range.y);
  float T = 1.f, acc[E];
#pragma unroll
  for (int q = 0; q < E; ++q) acc[q] = 0.f;
  for (uint32_t base = range.x; base < range.y; base += TPB) {
    // the barrier that also keeps a fast lane from overwriting LDS a slow lane still reads
    if (!__syncthreads_or(stop > base)) break;
    const uint32_t e = base + t;
    if (e < range.y) {
      size_t g = vals[e];
      if (g >= n) g = 0;
      s0[t] = rec0[g]; s1[t] = rec1[g];
#pragma unroll
      for (int q = 0; q < E; ++q) sx[t][q] = extra[g * E + q];
    }
    __syncthreads();
    const int nb = (int)min((uint32_t)TPB, range.y - base);
    const int mine = stop > base ? (int)min((uint32_t)nb, stop - base) : 0;
    for (int j = 0; j < mine; ++j) {
      const float4 a = s0[j], c = s1[j];
      rast::blend_extra<E>(T, acc, a.x - fx, a.y - fy, c.x, c.y, c.z, a.z, sx[j]);
    }
  }
  if (inside) {
#pragma unroll
    for (int q = 0; q < E; ++q) out[q * plane + at] = acc[q];
  }
}

// k_raster_backward_tiles for the extras: the same batches from the last to the first, the same sums over the 256 pixels in
// the same fixed order (shuffles within a wave, then the four waves out of LDS by the lane that owns the entry).  That lane
// then ADDS the six geometry / opacity sums to rows[e][0 .. 5] with a plain read-modify-write -- the colour tile kernel, an
// earlier launch on this stream, wrote every row of the range, and no other lane of this launch touches row e -- and stores
// the E attribute sums in xrows[e].  A batch no pixel reached leaves its rows alone and zero-fills its xrows: every element
// of xrows below `total` that a tile's range covers is written.
template <int E>
__global__ __launch_bounds__(TPB) void k_raster_extra_backward_tiles(int W, int H, int gx, uint32_t total, uint32_t n,
                                                                     const uint2 *__restrict__ ranges, const uint32_t *__restrict__ vals,
                                                                     const float4 *__restrict__ rec0, const float4 *__restrict__ rec1,
                                                                     const float *__restrict__ extra, const float *__restrict__ pix_T,
                                                                     const uint32_t *__restrict__ pix_stop,
                                                                     const float *__restrict__ g_extra, float *rows, float *xrows) {
  constexpr int NQ = NG + E;
  __shared__ float4 s0[TPB], s1[TPB];
  __shared__ float sx[TPB][E];
  __shared__ float part[TPB][WAVES][NQ];
  const int t = threadIdx.x, wave = t / 64, lane = t % 64;
  const int x = blockIdx.x * TILE + (t % TILE), y = blockIdx.y * TILE + (t / TILE);
  const bool inside = x < W && y < H;
  uint2 range = ranges[blockIdx.y * gx + blockIdx.x];
  range.y = min(range.y, total);
  range.x = min(range.x, range.y);
  const float fx = (float)x, fy = (float)y;
  uint32_t stop = range.x;
  float gxv[E];
  rast::PixelBackExtra<E> p;
  p.T = 0.f;
#pragma unroll
  for (int q = 0; q < E; ++q) { gxv[q] = 0.f; p.behind[q] = 0.f; }
  if (inside) {
    const size_t at = (size_t)y * W + x, plane = (size_t)W * H;
    stop = min(max(pix_stop[at], range.x), range.y);
    p.T = pix_T[at];
#pragma unroll
    for (int q = 0; q < E; ++q) gxv[q] = g_extra[q * plane + at];
  }
  const uint32_t count = range.y - range.x;
  for (uint32_t b = (count + TPB - 1) / TPB; b-- > 0;) {
    const uint32_t base = range.x + b * TPB;
    const uint32_t e = base + t;
    // the barrier that also keeps a fast lane from overwriting LDS a slow lane still reads
    if (!__syncthreads_or(stop > base)) {
      if (e < range.y) {
#pragma unroll
        for (int q = 0; q < E; ++q) xrows[(size_t)e * E + q] = 0.f;
      }
      continue;
    }
    if (e < range.y) {
      size_t g = vals[e];
      if (g >= n) g = 0;
      s0[t] = rec0[g]; s1[t] = rec1[g];
#pragma unroll
      for (int q = 0; q < E; ++q) sx[t][q] = extra[g * E + q];
    }
    __syncthreads();
    const int nb = (int)min((uint32_t)TPB, range.y - base);
    for (int j = nb - 1; j >= 0; --j) {
      float o[NQ];
      bool hit = false;
      if (base + (uint32_t)j < stop) {
        const float4 a = s0[j], c = s1[j];
        hit = rast::blend_extra_backward<E>(p, a.x - fx, a.y - fy, c.x, c.y, c.z, a.z, sx[j], gxv, o, o + NG);
      }
      if (__ballot(hit) == 0ull) {  // wave-uniform
        if (lane < NQ) part[j][wave][lane] = 0.f;
        continue;
      }
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        float v = hit ? o[q] : 0.f;
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
        if (lane == 0) part[j][wave][q] = v;
      }
    }
    __syncthreads();
    if (t < nb) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        float v = part[t][0][q];
        for (int w = 1; w < WAVES; ++w) v += part[t][w][q];
        if (q < NG) rows[(size_t)e * NP + q] += v;
        else xrows[(size_t)e * E + (q - NG)] = v;
      }
    }
  }
}

// One lane per (Gaussian, channel): the channel's sums of the Gaussian's entries, found through the inverse map, added in the
// order of its rectangle.  Every element of d_extra is written: zeros for a culled Gaussian.
__global__ __launch_bounds__(TPB) void k_raster_extra_gather(int64_t items, int E, const int4 *__restrict__ rect,
                                                             const uint64_t *__restrict__ offsets, const uint32_t *__restrict__ inv,
                                                             uint32_t total, const float *__restrict__ xrows, float *d_extra) {
  const int64_t at = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (at >= items) return;
  const int64_t i = at / E;
  const int q = (int)(at - i * E);
  const int4 r = rect[i];
  float sum = 0.f;
  if (r.z > r.x && r.w > r.y) {
    const uint64_t k0 = offsets[i], k1 = offsets[i + 1];
    if (k1 <= (uint64_t)total && k0 <= k1)
      for (uint64_t k = k0; k < k1; ++k) {
        const uint32_t e = inv[k];
        if (e < total) sum += xrows[(size_t)e * E + q];
      }
  }
  d_extra[at] = sum;
}

int reserve_xrows(mpmhip_raster *r, size_t count) {
  if (count <= r->cap_xrows) return MPMHIP_OK;
  ENTRY_CHECK(hipStreamSynchronize(r->stream));
  const size_t cap = grown(r->cap_xrows, count);
  r->cap_xrows = 0;
  if (int rc = regrow(r->xrows, cap)) return rc;
  r->cap_xrows = cap;
  return MPMHIP_OK;
}

bool channels_ok(int32_t E) { return E >= 1 && E <= rast::EXTRA_MAX; }

// the kernels are instantiated for every channel count, so that the accumulators stay in registers
#define EXTRA_DISPATCH(E, LAUNCH) \
  switch (E) {                    \
    case 1: LAUNCH(1); break;     \
    case 2: LAUNCH(2); break;     \
    case 3: LAUNCH(3); break;     \
    case 4: LAUNCH(4); break;     \
    case 5: LAUNCH(5); break;     \
    case 6: LAUNCH(6); break;     \
    case 7: LAUNCH(7); break;     \
    default: LAUNCH(8); break;    \
  }

}  // namespace

extern "C" int mpmhip_raster_extra_forward(mpmhip_raster *r, const mpmhip_raster_settings *s, int32_t n, const float *extra, int32_t E,
                                           float *out_extra) {
  if (!r || !s || n < 0 || !channels_ok(E) || !out_extra || (n > 0 && !extra)) return MPMHIP_ERR_INVALID;
  if (s->image_height <= 0 || s->image_width <= 0) return MPMHIP_ERR_INVALID;
  // the frame whose lists and stopping positions this walk reads must be the handle's newest, of this n and image size
  if (!r->grad_frame || r->grad_n != n || r->grad_w != s->image_width || r->grad_h != s->image_height) return MPMHIP_ERR_STATE;
  ENTRY_CHECK(hipSetDevice(r->device));
  const int W = r->grad_w, H = r->grad_h, gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE;
#define LAUNCH(N)                                                                                                                   \
  hipLaunchKernelGGL(k_raster_extra_forward<N>, dim3((unsigned)gx, (unsigned)gy), TPB, 0, r->stream, W, H, gx,                      \
                     (uint32_t)r->grad_entries, (uint32_t)n, (const uint2 *)r->ranges, (const uint32_t *)r->vals[1],                \
                     (const float4 *)r->rec0, (const float4 *)r->rec1, extra, (const uint32_t *)r->pix_stop, out_extra)
  EXTRA_DISPATCH(E, LAUNCH)
#undef LAUNCH
  return check(hipGetLastError());
}

extern "C" int mpmhip_raster_backward_extra(mpmhip_raster *r, const mpmhip_raster_settings *s, int32_t n, const float *means3D,
                                            const float *shs, int32_t n_sh_coeffs, const float *colors_precomp,
                                            const float *opacities, const float *scales, const float *rotations,
                                            const float *cov3D_precomp, const void *saved, int64_t saved_bytes, int64_t n_entries,
                                            const float *dL_dimage, const float *dL_dalpha, float *d_means3D, float *d_means2D,
                                            float *d_shs, float *d_colors_precomp, float *d_opacities, float *d_scales,
                                            float *d_rotations, float *d_cov3D_precomp, const float *extra, int32_t E,
                                            const float *g_extra, float *d_extra) {
  if (!channels_ok(E) || (n > 0 && (!extra || !d_extra))) return MPMHIP_ERR_INVALID;
  const Inputs in{means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, n_sh_coeffs};
  const Grads out{d_means3D, d_means2D, d_shs, d_colors_precomp, d_opacities, d_scales, d_rotations, d_cov3D_precomp};
  BackwardFrame f;
  if (int rc = backward_check(r, s, n, in, saved, saved_bytes, n_entries, out, &f)) return rc;
  if (n == 0) return MPMHIP_OK;  // nothing to write
  ENTRY_CHECK(hipSetDevice(r->device));
  if (int rc = backward_tiles(r, s, n, f, saved, n_entries, dL_dimage, dL_dalpha)) return rc;
  const char *sv = (const char *)saved;
  const SavedLayout &l = f.l;
  if (g_extra && n_entries > 0) {
    if (int rc = reserve_xrows(r, (size_t)n_entries * E)) return rc;
#define LAUNCH(N)                                                                                                                   \
  hipLaunchKernelGGL(k_raster_extra_backward_tiles<N>, dim3((unsigned)f.gx, (unsigned)f.gy), TPB, 0, r->stream, f.W, f.H, f.gx,     \
                     (uint32_t)n_entries, (uint32_t)n, (const uint2 *)(sv + l.ranges), (const uint32_t *)(sv + l.vals),             \
                     (const float4 *)(sv + l.rec0), (const float4 *)(sv + l.rec1), extra, (const float *)(sv + l.pix_T),            \
                     (const uint32_t *)(sv + l.pix_stop), g_extra, r->rows, r->xrows)
    EXTRA_DISPATCH(E, LAUNCH)
#undef LAUNCH
    ENTRY_CHECK(hipGetLastError());
  }
  if (int rc = backward_gaussians(r, s, n, in, f, saved, n_entries, out)) return rc;
  if (g_extra && n_entries > 0) {
    const int64_t items = (int64_t)n * E;
    hipLaunchKernelGGL(k_raster_extra_gather, blocks(items, TPB), TPB, 0, r->stream, items, (int)E, (const int4 *)(sv + l.rect),
                       (const uint64_t *)(sv + l.offsets), (const uint32_t *)(sv + l.inv), (uint32_t)n_entries,
                       (const float *)r->xrows, d_extra);
    ENTRY_CHECK(hipGetLastError());
  } else {  // no upstream gradient or nothing visible: zeros
    ENTRY_CHECK(hipMemsetAsync(d_extra, 0, (size_t)n * E * sizeof(float), r->stream));
  }
  return MPMHIP_OK;
}
