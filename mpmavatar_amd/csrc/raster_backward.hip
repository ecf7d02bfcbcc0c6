// raster_backward.hip -- the backward pass of the Gaussian rasteriser: what loss.backward() of the reference's
// train_appearance.py:123-155 needs of diff_gauss.GaussianRasterizer.  The math is raster_grad_math.hpp (the exact derivative
// of the forward function, decisions held fixed); this file is the pipeline, over a frame saved by mpmhip_raster_save:
//
//   k_raster_backward_tiles      one workgroup of 256 lanes per 16 x 16 tile walks the tile's entries back to front and
//                                leaves, per entry, the nine partials summed over the tile's pixels in a row of `rows`
//   k_raster_backward_gaussians  one lane per Gaussian sums its rows (found through the inverse map, in the order of its
//                                rectangle) and runs the per-Gaussian backward: conic, covariance, projection, SH
//
// No floating-point atomics: a (tile, Gaussian) entry belongs to one tile, so its row is written with plain stores by one
// lane, and a Gaussian's rows are added in a fixed order -- the same input gives the same bits.  The price is the row
// buffer, 36 B per entry written once and read once (DESIGN.md section 13 sets it against the frame's other bytes).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "raster_state.hpp"

namespace {

using namespace raster_host;
constexpr int NP = rast::N_PARTIALS;
constexpr int WAVES = TPB / 64;

// Lane t = pixel (t % 16, t / 16) of the tile, as in k_raster_render.  The tile's entries [range.x, range.y) are taken in
// batches of TPB from the last (partial) one to the first; a batch no pixel of the tile reached (every stop <= its first
// entry) is only zero-filled.  Otherwise lane t stages the record of entry base + t in LDS, every lane walks the batch
// from its end, and for each entry the nine partials are summed over the 256 pixels in a fixed order: within a wave by
// shuffles (a wave whose ballot shows no contributing lane writes zeros without them), then lane t adds the four waves'
// sums of entry base + t out of LDS and stores the row.  Lanes outside the image contribute nothing but stage and meet
// every barrier.  Every row of the tile's range is written, so `rows` needs no clearing.
// `total` and `n` only bound what a damaged saved frame could make the kernel touch.
__global__ __launch_bounds__(TPB) void k_raster_backward_tiles(int W, int H, int gx, uint32_t total, uint32_t n,
                                                               const uint2 *__restrict__ ranges, const uint32_t *__restrict__ vals,
                                                               const float4 *__restrict__ rec0, const float4 *__restrict__ rec1,
                                                               const float *__restrict__ colour, const float *__restrict__ pix_T,
                                                               const uint32_t *__restrict__ pix_stop, float bg_r, float bg_g,
                                                               float bg_b, const float *__restrict__ g_image,
                                                               const float *__restrict__ g_alpha, float *rows) {
  __shared__ float4 s0[TPB], s1[TPB];
  __shared__ float sr[TPB], sg[TPB], sb[TPB];
  __shared__ float part[TPB][WAVES][NP];
  const int t = threadIdx.x, wave = t / 64, lane = t % 64;
  const int x = blockIdx.x * TILE + (t % TILE), y = blockIdx.y * TILE + (t / TILE);
  const bool inside = x < W && y < H;
  uint2 range = ranges[blockIdx.y * gx + blockIdx.x];
  range.y = min(range.y, total);
  range.x = min(range.x, range.y);
  const float fx = (float)x, fy = (float)y;
  uint32_t stop = range.x;
  rast::V3 gi{0.f, 0.f, 0.f};
  float gt = 0.f;
  rast::PixelBack p{0.f, 0.f, 0.f, 0.f};
  if (inside) {
    const size_t at = (size_t)y * W + x, plane = (size_t)W * H;
    stop = min(max(pix_stop[at], range.x), range.y);
    p.T = pix_T[at];
    if (g_image) gi = rast::V3{g_image[at], g_image[plane + at], g_image[2 * plane + at]};
    const float ga = g_alpha ? g_alpha[at] : 0.f;
    gt = (gi.x * bg_r + gi.y * bg_g + gi.z * bg_b - ga) * p.T;
  }
  const uint32_t count = range.y - range.x;
  for (uint32_t b = (count + TPB - 1) / TPB; b-- > 0;) {
    const uint32_t base = range.x + b * TPB;
    const uint32_t e = base + t;
    // the barrier that also keeps a fast lane from overwriting LDS a slow lane still reads
    if (!__syncthreads_or(stop > base)) {
      if (e < range.y)
        for (int q = 0; q < NP; ++q) rows[(size_t)e * NP + q] = 0.f;
      continue;
    }
    if (e < range.y) {
      size_t g = vals[e];
      if (g >= n) g = 0;
      s0[t] = rec0[g]; s1[t] = rec1[g];
      sr[t] = colour[3 * g]; sg[t] = colour[3 * g + 1]; sb[t] = colour[3 * g + 2];
    }
    __syncthreads();
    const int nb = (int)min((uint32_t)TPB, range.y - base);
    for (int j = nb - 1; j >= 0; --j) {
      float o[NP];
      bool hit = false;
      if (base + (uint32_t)j < stop) {
        const float4 a = s0[j], c = s1[j];
        hit = rast::blend_backward(p, a.x - fx, a.y - fy, c.x, c.y, c.z, a.z, rast::V3{sr[j], sg[j], sb[j]}, gi, gt, o);
      }
      if (__ballot(hit) == 0ull) {  // wave-uniform
        if (lane < NP) part[j][wave][lane] = 0.f;
        continue;
      }
      for (int q = 0; q < NP; ++q) {
        float v = hit ? o[q] : 0.f;
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
        if (lane == 0) part[j][wave][q] = v;
      }
    }
    __syncthreads();
    if (t < nb)
      for (int q = 0; q < NP; ++q) {
        float v = part[t][0][q];
        for (int w = 1; w < WAVES; ++w) v += part[t][w][q];
        rows[(size_t)e * NP + q] = v;
      }
  }
}

// One lane per Gaussian.  Every output element of the Gaussian is written: zeros when it was culled.
__global__ __launch_bounds__(TPB) void k_raster_backward_gaussians(int n, Camera cam, Inputs in, const int4 *__restrict__ rect,
                                                                   const uint64_t *__restrict__ offsets,
                                                                   const uint32_t *__restrict__ inv, uint32_t total,
                                                                   const float *__restrict__ rows, Grads out) {
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const size_t s = (size_t)i;
  const int4 r = rect[i];
  const bool vis = r.z > r.x && r.w > r.y;
  float o[NP];
  for (int q = 0; q < NP; ++q) o[q] = 0.f;
  if (vis) {
    const uint64_t k0 = offsets[i], k1 = offsets[i + 1];
    if (k1 <= (uint64_t)total && k0 <= k1)
      for (uint64_t k = k0; k < k1; ++k) {
        const uint32_t e = inv[k];
        if (e < total)
          for (int q = 0; q < NP; ++q) o[q] += rows[(size_t)e * NP + q];
      }
  }
  rast::V3 mean{in.means[3 * s], in.means[3 * s + 1], in.means[3 * s + 2]};
  rast::V3 dmean{0.f, 0.f, 0.f}, dscale{0.f, 0.f, 0.f};
  rast::V4 dq{0.f, 0.f, 0.f, 0.f};
  rast::Sym3 dS{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (vis) {
    float V[16], P[16];
    for (int k = 0; k < 16; ++k) { V[k] = cam.view[k]; P[k] = cam.proj[k]; }
    rast::Sym3 S;
    if (in.cov) {
      const float *c = in.cov + 6 * s;
      S = rast::Sym3{c[0], c[1], c[2], c[3], c[4], c[5]};
    } else {
      S = rast::cov3d(rast::V3{in.scales[3 * s], in.scales[3 * s + 1], in.scales[3 * s + 2]}, cam.scale_modifier,
                      rast::V4{in.rots[4 * s], in.rots[4 * s + 1], in.rots[4 * s + 2], in.rots[4 * s + 3]});
    }
    rast::project_backward(mean, S, V, P, cam.W, cam.H, cam.tanfovx, cam.tanfovy, o[0], o[1], o[2], o[3], o[4], dmean, dS);
    if (!in.cov)
      rast::cov3d_backward(rast::V3{in.scales[3 * s], in.scales[3 * s + 1], in.scales[3 * s + 2]}, cam.scale_modifier,
                           rast::V4{in.rots[4 * s], in.rots[4 * s + 1], in.rots[4 * s + 2], in.rots[4 * s + 3]}, dS, dscale, dq);
  }
  if (in.shs) {
    float *d = out.shs + 3 * (size_t)in.n_sh * s;
    if (vis)
      rast::sh_backward(cam.sh_degree, in.shs + 3 * (size_t)in.n_sh * s, in.n_sh, mean,
                        rast::V3{cam.campos[0], cam.campos[1], cam.campos[2]}, rast::V3{o[6], o[7], o[8]}, d, dmean);
    else
      for (int k = 0; k < 3 * in.n_sh; ++k) d[k] = 0.f;
  } else {
    out.colors[3 * s] = o[6]; out.colors[3 * s + 1] = o[7]; out.colors[3 * s + 2] = o[8];
  }
  out.means[3 * s] = dmean.x; out.means[3 * s + 1] = dmean.y; out.means[3 * s + 2] = dmean.z;
  // the published convention: the gradient with respect to an additive NDC offset of the pixel centre
  out.means2d[3 * s] = o[0] * (0.5f * (float)cam.W); out.means2d[3 * s + 1] = o[1] * (0.5f * (float)cam.H); out.means2d[3 * s + 2] = 0.f;
  out.opac[i] = o[5];
  if (in.cov) {
    float *d = out.cov + 6 * s;
    d[0] = dS.xx; d[1] = dS.xy; d[2] = dS.xz; d[3] = dS.yy; d[4] = dS.yz; d[5] = dS.zz;
  } else {
    out.scales[3 * s] = dscale.x; out.scales[3 * s + 1] = dscale.y; out.scales[3 * s + 2] = dscale.z;
    out.rots[4 * s] = dq.x; out.rots[4 * s + 1] = dq.y; out.rots[4 * s + 2] = dq.z; out.rots[4 * s + 3] = dq.w;
  }
}

int reserve_rows(mpmhip_raster *r, size_t count) {
  if (count <= r->cap_rows) return MPMHIP_OK;
  ENTRY_CHECK(hipStreamSynchronize(r->stream));
  const size_t cap = grown(r->cap_rows, count);
  r->cap_rows = 0;
  if (int rc = regrow(r->rows, cap)) return rc;
  r->cap_rows = cap;
  return MPMHIP_OK;
}

}  // namespace

namespace raster_host {

int backward_check(const mpmhip_raster *r, const mpmhip_raster_settings *s, int32_t n, const Inputs &in, const void *saved,
                   int64_t saved_bytes, int64_t n_entries, const Grads &out, BackwardFrame *frame) {
  if (!saved || n_entries < 0 || n_entries > (int64_t)INT32_MAX) return MPMHIP_ERR_INVALID;
  if (n > 0) {
    if (!out.means || !out.means2d || !out.opac) return MPMHIP_ERR_INVALID;
    if (in.shs ? !out.shs : !out.colors) return MPMHIP_ERR_INVALID;
    if (in.scales && in.rots ? (!out.scales || !out.rots) : !out.cov) return MPMHIP_ERR_INVALID;
  } else if (n_entries != 0) {
    return MPMHIP_ERR_INVALID;
  }
  int gx = 0, gy = 0;
  if (int rc = validate_frame(r, s, n, in, &gx, &gy)) return rc;
  const int W = s->image_width, H = s->image_height;
  *frame = BackwardFrame{W, H, gx, gy, saved_layout((size_t)n, (size_t)gx * gy, (size_t)W * H, (size_t)n_entries)};
  if (saved_bytes != (int64_t)frame->l.bytes) return MPMHIP_ERR_INVALID;  // another n, image size or entry count than the frame's
  return MPMHIP_OK;
}

int backward_tiles(mpmhip_raster *r, const mpmhip_raster_settings *s, int32_t n, const BackwardFrame &f, const void *saved,
                   int64_t n_entries, const float *dL_dimage, const float *dL_dalpha) {
  if (n_entries <= 0) return MPMHIP_OK;
  const SavedLayout &l = f.l;
  const char *sv = (const char *)saved;
  if (int rc = reserve_rows(r, (size_t)n_entries * NP)) return rc;
  hipLaunchKernelGGL(k_raster_backward_tiles, dim3((unsigned)f.gx, (unsigned)f.gy), TPB, 0, r->stream, f.W, f.H, f.gx,
                     (uint32_t)n_entries, (uint32_t)n, (const uint2 *)(sv + l.ranges), (const uint32_t *)(sv + l.vals),
                     (const float4 *)(sv + l.rec0), (const float4 *)(sv + l.rec1), (const float *)(sv + l.colour),
                     (const float *)(sv + l.pix_T), (const uint32_t *)(sv + l.pix_stop), s->bg[0], s->bg[1], s->bg[2], dL_dimage,
                     dL_dalpha, r->rows);
  return check(hipGetLastError());
}

int backward_gaussians(mpmhip_raster *r, const mpmhip_raster_settings *s, int32_t n, const Inputs &in, const BackwardFrame &f,
                       const void *saved, int64_t n_entries, const Grads &out) {
  const SavedLayout &l = f.l;
  const char *sv = (const char *)saved;
  Camera cam{f.W, f.H, f.gx, f.gy, s->tanfovx, s->tanfovy, s->scale_modifier, s->sh_degree, s->viewmatrix, s->projmatrix, s->campos};
  hipLaunchKernelGGL(k_raster_backward_gaussians, blocks(n, TPB), TPB, 0, r->stream, n, cam, in, (const int4 *)(sv + l.rect),
                     (const uint64_t *)(sv + l.offsets), (const uint32_t *)(sv + l.inv), (uint32_t)n_entries,
                     (const float *)r->rows, out);
  return check(hipGetLastError());
}

}  // namespace raster_host

extern "C" int mpmhip_raster_backward(mpmhip_raster *r, const mpmhip_raster_settings *s, int32_t n, const float *means3D,
                                      const float *shs, int32_t n_sh_coeffs, const float *colors_precomp, const float *opacities,
                                      const float *scales, const float *rotations, const float *cov3D_precomp, const void *saved,
                                      int64_t saved_bytes, int64_t n_entries, const float *dL_dimage, const float *dL_dalpha,
                                      float *d_means3D, float *d_means2D, float *d_shs, float *d_colors_precomp, float *d_opacities,
                                      float *d_scales, float *d_rotations, float *d_cov3D_precomp) {
  const Inputs in{means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, n_sh_coeffs};
  const Grads out{d_means3D, d_means2D, d_shs, d_colors_precomp, d_opacities, d_scales, d_rotations, d_cov3D_precomp};
  BackwardFrame f;
  if (int rc = backward_check(r, s, n, in, saved, saved_bytes, n_entries, out, &f)) return rc;
  if (n == 0) return MPMHIP_OK;  // nothing to write
  ENTRY_CHECK(hipSetDevice(r->device));
  if (int rc = backward_tiles(r, s, n, f, saved, n_entries, dL_dimage, dL_dalpha)) return rc;
  return backward_gaussians(r, s, n, in, f, saved, n_entries, out);
}
