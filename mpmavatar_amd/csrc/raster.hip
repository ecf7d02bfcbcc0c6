// raster.hip -- forward Gaussian rasteriser: what the reference calls as diff_gauss.GaussianRasterizer
// (/root/reference/gaussian_renderer/__init__.py:14,36-103), as the eval loop (train_material_params.py:857-872) and the
// demo (run_demo.py:540-604) use it, and its training flavour (mpmhip_raster_forward_grad), which also records what the
// backward pass (raster_backward.hip) needs.  The math is raster_math.hpp; this file is the pipeline:
//
//   k_raster_preprocess  one lane per Gaussian: projection, conic, radius, tile rectangle, colour -> packed records
//   rocprim::exclusive_scan of tiles_touched (n + 1 values: the last offset is the entry count)
//   >> the entry count is read back with one 8-byte device-to-host copy: ONE STREAM SYNCHRONISATION PER RENDERED FRAME,
//      as the CUDA original has (it sizes the sort).  Nothing in the solver path calls into this file.
//   k_raster_duplicate   key (tile << 32 | depth bits) and Gaussian index for every (tile, Gaussian) entry
//   rocprim::radix_sort_pairs over bits [0, 32 + ceil(log2 tiles)): stable, so equal depths keep the index order
//   k_raster_ranges      start / end of every tile's run in the sorted keys
//   k_raster_render      one workgroup of 256 lanes per 16 x 16 tile, front-to-back blend (the hot path)
//
// No floating-point atomics anywhere: the same input gives the same bits.  The scratch (records, keys, sort temporaries,
// tile ranges) belongs to the handle, grows geometrically when a frame needs more and is reused otherwise: no allocation
// in steady state.  Measured numbers: DESIGN.md section 13, profiles/raster_bench.json.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <new>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "entry.hpp"
#include "raster_state.hpp"

namespace {

using namespace raster_host;

__global__ __launch_bounds__(TPB) void k_raster_preprocess(int n, Camera cam, const float *__restrict__ means,
                                                           const float *__restrict__ shs, int n_sh,
                                                           const float *__restrict__ colors, const float *__restrict__ opac,
                                                           const float *__restrict__ scales, const float *__restrict__ rots,
                                                           const float *__restrict__ cov, float4 *rec0, float4 *rec1,
                                                           float *colour, int4 *rect, uint32_t *touched, int32_t *radii) {
  int i = blockIdx.x * TPB + threadIdx.x;
  if (i > n) return;
  if (i == n) { touched[n] = 0; return; }  // the scan runs over n + 1 values
  float V[16], P[16];
  for (int k = 0; k < 16; ++k) { V[k] = cam.view[k]; P[k] = cam.proj[k]; }
  const size_t s = (size_t)i;
  rast::V3 mean{means[3 * s], means[3 * s + 1], means[3 * s + 2]};
  rast::Sym3 S;
  if (cov) {
    const float *c = cov + 6 * s;
    S = rast::Sym3{c[0], c[1], c[2], c[3], c[4], c[5]};
  } else {
    S = rast::cov3d(rast::V3{scales[3 * s], scales[3 * s + 1], scales[3 * s + 2]}, cam.scale_modifier,
                    rast::V4{rots[4 * s], rots[4 * s + 1], rots[4 * s + 2], rots[4 * s + 3]});
  }
  rast::Splat o = rast::project(mean, S, V, P, cam.W, cam.H, cam.tanfovx, cam.tanfovy, cam.gx, cam.gy);
  radii[i] = o.radius;
  if (o.radius == 0) {
    touched[i] = 0;
    rect[i] = make_int4(0, 0, 0, 0);
    return;
  }
  rast::V3 col;
  if (shs) col = rast::sh_colour(cam.sh_degree, shs + 3 * (size_t)n_sh * s, mean, rast::V3{cam.campos[0], cam.campos[1], cam.campos[2]});
  else col = rast::V3{colors[3 * s], colors[3 * s + 1], colors[3 * s + 2]};
  rec0[i] = make_float4(o.px, o.py, opac[i], o.depth);
  rec1[i] = make_float4(o.A, o.B, o.C, 0.f);
  colour[3 * s] = col.x; colour[3 * s + 1] = col.y; colour[3 * s + 2] = col.z;
  rect[i] = make_int4(o.x0, o.y0, o.x1, o.y1);
  touched[i] = (uint32_t)(o.x1 - o.x0) * (uint32_t)(o.y1 - o.y0);
}

// Entries offsets[i] .. offsets[i + 1) belong to Gaussian i: the scan was taken over the very counts this loop runs, so
// nothing is written at or beyond offsets[n] (= the entry count the buffers were sized for).
__global__ __launch_bounds__(TPB) void k_raster_duplicate(int n, int gx, const int4 *__restrict__ rect,
                                                          const float4 *__restrict__ rec0,
                                                          const uint64_t *__restrict__ offsets, uint64_t *keys, uint32_t *vals) {
  int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  int4 r = rect[i];
  if (r.z <= r.x || r.w <= r.y) return;
  uint64_t at = offsets[i];
  const uint64_t depth = __float_as_uint(rec0[i].w);  // positive: the bits order like the value
  for (int y = r.y; y < r.w; ++y)
    for (int x = r.x; x < r.z; ++x) {
      keys[at] = ((uint64_t)(uint32_t)(y * gx + x) << 32) | depth;
      vals[at] = (uint32_t)i;
      ++at;
    }
}

// ranges[] is zeroed before: a tile without entries keeps (0, 0)
__global__ __launch_bounds__(TPB) void k_raster_ranges(int64_t total, const uint64_t *__restrict__ keys, uint2 *ranges) {
  int64_t e = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (e >= total) return;
  uint32_t tile = (uint32_t)(keys[e] >> 32);
  if (e == 0) {
    ranges[tile].x = 0;
  } else {
    uint32_t prev = (uint32_t)(keys[e - 1] >> 32);
    if (prev != tile) { ranges[prev].y = (uint32_t)e; ranges[tile].x = (uint32_t)e; }
  }
  if (e == total - 1) ranges[tile].y = (uint32_t)total;
}

// One workgroup per tile, lane t = pixel (t % 16, t / 16) of it: wave w owns pixel rows 4 w .. 4 w + 3.  The tile's list is
// consumed in batches of TPB entries: lane t fetches the record of entry base + t into LDS (two float4 and the colour,
// 11 KB per workgroup), then every lane walks the batch out of LDS -- the address is the same for all lanes, so the reads
// are broadcasts without bank conflicts.  The count barrier at the top of a batch is also what keeps a fast lane from
// overwriting records a slow lane still reads.  Lanes outside the image take part in staging and barriers, count as
// done from the start and write nothing.
// SAVE = the training flavour (mpmhip_raster_forward_grad): every pixel also stores its final T and the position in the
// sorted entries at which it stopped -- the entry that finished it, or the end of its tile's range -- for the backward pass.
template <bool SAVE>
__global__ __launch_bounds__(TPB) void k_raster_render(int W, int H, int gx, const uint2 *__restrict__ ranges,
                                                       const uint32_t *__restrict__ vals, const float4 *__restrict__ rec0,
                                                       const float4 *__restrict__ rec1, const float *__restrict__ colour,
                                                       float bg_r, float bg_g, float bg_b, float *out_color, float *out_alpha,
                                                       float *pix_T, uint32_t *pix_stop) {
  __shared__ float4 s0[TPB], s1[TPB];
  __shared__ float sr[TPB], sg[TPB], sb[TPB];
  const int t = threadIdx.x;
  const int x = blockIdx.x * TILE + (t % TILE), y = blockIdx.y * TILE + (t / TILE);
  const bool inside = x < W && y < H;
  const uint2 range = ranges[blockIdx.y * gx + blockIdx.x];
  const float fx = (float)x, fy = (float)y;
  rast::Pixel p{1.f, 0.f, 0.f, 0.f};
  bool done = !inside;
  uint32_t stop = range.y;
  for (uint32_t base = range.x; base < range.y; base += TPB) {
    if (__syncthreads_count(done) == TPB) break;
    const uint32_t e = base + t;
    if (e < range.y) {
      const size_t g = vals[e];
      s0[t] = rec0[g]; s1[t] = rec1[g];
      sr[t] = colour[3 * g]; sg[t] = colour[3 * g + 1]; sb[t] = colour[3 * g + 2];
    }
    __syncthreads();
    const int nb = (int)min((uint32_t)TPB, range.y - base);
    for (int j = 0; !done && j < nb; ++j) {
      const float4 a = s0[j], c = s1[j];
      done = rast::blend(p, a.x - fx, a.y - fy, c.x, c.y, c.z, a.z, rast::V3{sr[j], sg[j], sb[j]});
      if constexpr (SAVE) {
        if (done) stop = base + (uint32_t)j;
      }
    }
  }
  if (inside) {
    const size_t at = (size_t)y * W + x, plane = (size_t)W * H;
    out_color[at] = p.r + p.T * bg_r;
    out_color[plane + at] = p.g + p.T * bg_g;
    out_color[2 * plane + at] = p.b + p.T * bg_b;
    out_alpha[at] = 1.f - p.T;
    if constexpr (SAVE) { pix_T[at] = p.T; pix_stop[at] = stop; }
  }
}

// After the sort: where each entry went.  Before the sort Gaussian g's entries lie at offsets[g] + (ty - y0) (x1 - x0) +
// (tx - x0) (k_raster_duplicate); inv[that] = the sorted position, so the backward pass finds a Gaussian's rows without a
// search.  Every slot below `total` is written exactly once: the sort permutes the entries.
__global__ __launch_bounds__(TPB) void k_raster_inverse(int64_t total, int gx, const uint64_t *__restrict__ keys,
                                                        const uint32_t *__restrict__ vals, const int4 *__restrict__ rect,
                                                        const uint64_t *__restrict__ offsets, uint32_t *inv) {
  int64_t e = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (e >= total) return;
  const uint32_t g = vals[e], tile = (uint32_t)(keys[e] >> 32);
  const int tx = (int)(tile % (uint32_t)gx), ty = (int)(tile / (uint32_t)gx);
  const int4 r = rect[g];
  inv[offsets[g] + (uint64_t)((ty - r.y) * (r.z - r.x) + (tx - r.x))] = (uint32_t)e;
}

// touched[i] > 0 exactly when radii[i] > 0 (k_raster_preprocess), and unlike radii it is the handle's own memory
__global__ __launch_bounds__(TPB) void k_raster_counts(int tiles, const uint2 *ranges, int n, const uint32_t *touched, int32_t *counts) {
  int i = blockIdx.x * TPB + threadIdx.x;
  if (i < tiles) atomicMax(&counts[0], (int32_t)(ranges[i].y - ranges[i].x));
  if (i < n && touched[i] > 0) atomicAdd(&counts[1], 1);
}

// stage k of the frame ends here (profiling only)
int mark(mpmhip_raster *r, int k) { return r->profile ? check(hipEventRecord(r->ev[k], r->stream)) : MPMHIP_OK; }

unsigned bits_for(int tiles) {  // ceil(log2(tiles))
  unsigned b = 0;
  while (((int64_t)1 << b) < tiles) ++b;
  return b;
}

int reserve_grad(mpmhip_raster *r, size_t pixels, size_t total) {
  if (pixels > r->cap_pix) {
    ENTRY_CHECK(hipStreamSynchronize(r->stream));
    const size_t cap = grown(r->cap_pix, pixels);
    r->cap_pix = 0;
    if (int rc = regrow(r->pix_T, cap)) return rc;
    if (int rc = regrow(r->pix_stop, cap)) return rc;
    r->cap_pix = cap;
  }
  if (total > r->cap_inv) {
    ENTRY_CHECK(hipStreamSynchronize(r->stream));
    const size_t cap = grown(r->cap_inv, total);
    r->cap_inv = 0;
    if (int rc = regrow(r->inv, cap)) return rc;
    r->cap_inv = cap;
  }
  return MPMHIP_OK;
}

// grad = false is mpmhip_raster_forward: the render kernel's plain instantiation, no per-pixel state, nothing more allocated
int forward_impl(mpmhip_raster *r, const mpmhip_raster_settings *s, int32_t n, const float *means3D, const float *shs,
                 int32_t n_sh_coeffs, const float *colors_precomp, const float *opacities, const float *scales,
                 const float *rotations, const float *cov3D_precomp, float *out_color, float *out_alpha, int32_t *radii, bool grad);

}  // namespace

extern "C" {

int mpmhip_raster_create(int32_t device, void *stream, mpmhip_raster **out) {
  if (!out) return MPMHIP_ERR_INVALID;
  *out = nullptr;
  if (int rc = select_device(device)) return rc;
  mpmhip_raster *r = new (std::nothrow) mpmhip_raster();
  if (!r) return MPMHIP_ERR_HIP;
  r->device = device;
  r->stream = (hipStream_t)stream;
  if (hipHostMalloc((void **)&r->h_total, sizeof(uint64_t), hipHostMallocDefault) != hipSuccess ||
      hipMalloc((void **)&r->d_counts, 2 * sizeof(int32_t)) != hipSuccess) {
    mpmhip_raster_destroy(r);
    return MPMHIP_ERR_HIP;
  }
  *out = r;
  return MPMHIP_OK;
}

void mpmhip_raster_destroy(mpmhip_raster *r) {
  if (!r) return;
  (void)hipSetDevice(r->device);
  (void)hipStreamSynchronize(r->stream);
  void *dev[] = {r->rec0, r->rec1, r->colour, r->rect, r->touched, r->offsets, r->scan_tmp, r->keys[0], r->keys[1],
                 r->vals[0], r->vals[1], r->sort_tmp, r->ranges, r->d_counts, r->pix_T, r->pix_stop, r->inv, r->rows, r->xrows};
  for (void *p : dev)
    if (p) (void)hipFree(p);
  if (r->h_total) (void)hipHostFree(r->h_total);
  for (hipEvent_t e : r->ev)
    if (e) (void)hipEventDestroy(e);
  delete r;
}

int mpmhip_raster_forward(mpmhip_raster *r, const mpmhip_raster_settings *s, int32_t n, const float *means3D, const float *shs,
                          int32_t n_sh_coeffs, const float *colors_precomp, const float *opacities, const float *scales,
                          const float *rotations, const float *cov3D_precomp, float *out_color, float *out_alpha,
                          int32_t *radii) {
  return forward_impl(r, s, n, means3D, shs, n_sh_coeffs, colors_precomp, opacities, scales, rotations, cov3D_precomp, out_color,
                      out_alpha, radii, false);
}

int mpmhip_raster_forward_grad(mpmhip_raster *r, const mpmhip_raster_settings *s, int32_t n, const float *means3D, const float *shs,
                               int32_t n_sh_coeffs, const float *colors_precomp, const float *opacities, const float *scales,
                               const float *rotations, const float *cov3D_precomp, float *out_color, float *out_alpha,
                               int32_t *radii) {
  return forward_impl(r, s, n, means3D, shs, n_sh_coeffs, colors_precomp, opacities, scales, rotations, cov3D_precomp, out_color,
                      out_alpha, radii, true);
}

int mpmhip_raster_saved_bytes(const mpmhip_raster *r, int64_t *bytes, int64_t *n_entries) {
  if (!r || !bytes || !n_entries) return MPMHIP_ERR_INVALID;
  if (!r->grad_frame) return MPMHIP_ERR_STATE;
  *bytes = (int64_t)saved_layout((size_t)r->grad_n, (size_t)r->grad_tiles, r->grad_pixels, (size_t)r->grad_entries).bytes;
  *n_entries = r->grad_entries;
  return MPMHIP_OK;
}

int mpmhip_raster_save(mpmhip_raster *r, void *dst, int64_t bytes) {
  if (!r || !dst) return MPMHIP_ERR_INVALID;
  if (!r->grad_frame) return MPMHIP_ERR_STATE;
  const size_t n = (size_t)r->grad_n, e = (size_t)r->grad_entries;
  const SavedLayout l = saved_layout(n, (size_t)r->grad_tiles, r->grad_pixels, e);
  if (bytes != (int64_t)l.bytes) return MPMHIP_ERR_INVALID;
  ENTRY_CHECK(hipSetDevice(r->device));
  char *d = (char *)dst;
  auto copy = [&](size_t at, const void *src, size_t size) {
    return size == 0 ? MPMHIP_OK : check(hipMemcpyAsync(d + at, src, size, hipMemcpyDeviceToDevice, r->stream));
  };
  if (int rc = copy(l.rec0, r->rec0, n * sizeof(float4))) return rc;
  if (int rc = copy(l.rec1, r->rec1, n * sizeof(float4))) return rc;
  if (int rc = copy(l.rect, r->rect, n * sizeof(int4))) return rc;
  if (int rc = copy(l.offsets, r->offsets, n ? (n + 1) * sizeof(uint64_t) : 0)) return rc;
  if (int rc = copy(l.ranges, r->ranges, (size_t)r->grad_tiles * sizeof(uint2))) return rc;
  if (int rc = copy(l.colour, r->colour, n * 3 * sizeof(float))) return rc;
  if (int rc = copy(l.pix_T, r->pix_T, r->grad_pixels * sizeof(float))) return rc;
  if (int rc = copy(l.pix_stop, r->pix_stop, r->grad_pixels * sizeof(uint32_t))) return rc;
  if (int rc = copy(l.vals, r->vals[1], e * sizeof(uint32_t))) return rc;
  if (int rc = copy(l.inv, r->inv, e * sizeof(uint32_t))) return rc;
  return MPMHIP_OK;
}

}  // extern "C"

namespace {

int forward_impl(mpmhip_raster *r, const mpmhip_raster_settings *s, int32_t n, const float *means3D, const float *shs,
                 int32_t n_sh_coeffs, const float *colors_precomp, const float *opacities, const float *scales,
                 const float *rotations, const float *cov3D_precomp, float *out_color, float *out_alpha, int32_t *radii,
                 const bool grad) {
  if (!out_color || !out_alpha || (n > 0 && !radii)) return MPMHIP_ERR_INVALID;
  const Inputs in{means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, n_sh_coeffs};
  int gx = 0, gy = 0;
  if (int rc = validate_frame(r, s, n, in, &gx, &gy)) return rc;
  const int W = s->image_width, H = s->image_height, tiles = gx * gy;
  ENTRY_CHECK(hipSetDevice(r->device));
  hipStream_t st = r->stream;
  if (int rc = reserve_tiles(r, tiles)) return rc;
  if (int rc = reserve_gaussians(r, n > 0 ? n : 1)) return rc;
  ENTRY_CHECK(hipMemsetAsync(r->ranges, 0, (size_t)tiles * sizeof(uint2), st));
  r->last_n = n; r->last_tiles = tiles; r->last_entries = 0;
  r->grad_frame = false;

  uint64_t total = 0;
  if (int rc = mark(r, 0)) return rc;
  if (n > 0) {
    Camera cam{W, H, gx, gy, s->tanfovx, s->tanfovy, s->scale_modifier, s->sh_degree, s->viewmatrix, s->projmatrix, s->campos};
    hipLaunchKernelGGL(k_raster_preprocess, blocks((int64_t)n + 1, TPB), TPB, 0, st, n, cam, means3D, shs, n_sh_coeffs, colors_precomp,
                       opacities, scales, rotations, cov3D_precomp, r->rec0, r->rec1, r->colour, r->rect, r->touched, radii);
    ENTRY_CHECK(hipGetLastError());
    if (int rc = mark(r, 1)) return rc;
    size_t tmp = 0;
    ENTRY_CHECK(rocprim::exclusive_scan(nullptr, tmp, r->touched, r->offsets, (uint64_t)0, (size_t)n + 1, rocprim::plus<uint64_t>(), st));
    if (int rc = reserve_tmp(r, r->scan_tmp, r->scan_tmp_bytes, tmp)) return rc;
    ENTRY_CHECK(rocprim::exclusive_scan(r->scan_tmp, tmp, r->touched, r->offsets, (uint64_t)0, (size_t)n + 1, rocprim::plus<uint64_t>(), st));
    ENTRY_CHECK(hipMemcpyAsync(r->h_total, r->offsets + n, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    ENTRY_CHECK(hipStreamSynchronize(st));  // the one synchronisation of a frame
    total = *r->h_total;
    if (total > (uint64_t)INT32_MAX) return MPMHIP_ERR_LIMIT;
  } else if (int rc = mark(r, 1)) {
    return rc;
  }
  if (int rc = mark(r, 2)) return rc;
  if (total > 0) {
    if (int rc = reserve_entries(r, (size_t)total)) return rc;
    hipLaunchKernelGGL(k_raster_duplicate, blocks(n, TPB), TPB, 0, st, n, gx, (const int4 *)r->rect, (const float4 *)r->rec0,
                       (const uint64_t *)r->offsets, r->keys[0], r->vals[0]);
    ENTRY_CHECK(hipGetLastError());
    if (int rc = mark(r, 3)) return rc;
    const unsigned end_bit = 32u + bits_for(tiles);
    size_t tmp = 0;
    ENTRY_CHECK(rocprim::radix_sort_pairs(nullptr, tmp, r->keys[0], r->keys[1], r->vals[0], r->vals[1], (size_t)total, 0u, end_bit, st));
    if (int rc = reserve_tmp(r, r->sort_tmp, r->sort_tmp_bytes, tmp)) return rc;
    ENTRY_CHECK(rocprim::radix_sort_pairs(r->sort_tmp, tmp, r->keys[0], r->keys[1], r->vals[0], r->vals[1], (size_t)total, 0u,
                                       end_bit, st));
    if (int rc = mark(r, 4)) return rc;
    hipLaunchKernelGGL(k_raster_ranges, blocks((int64_t)total, TPB), TPB, 0, st, (int64_t)total, (const uint64_t *)r->keys[1], r->ranges);
    ENTRY_CHECK(hipGetLastError());
    if (grad) {
      if (int rc = reserve_grad(r, (size_t)W * H, (size_t)total)) return rc;
      hipLaunchKernelGGL(k_raster_inverse, blocks((int64_t)total, TPB), TPB, 0, st, (int64_t)total, gx, (const uint64_t *)r->keys[1],
                         (const uint32_t *)r->vals[1], (const int4 *)r->rect, (const uint64_t *)r->offsets, r->inv);
      ENTRY_CHECK(hipGetLastError());
    }
  } else {
    if (int rc = mark(r, 3)) return rc;
    if (int rc = mark(r, 4)) return rc;
  }
  if (int rc = mark(r, 5)) return rc;
  r->last_entries = (int64_t)total;
  if (grad) {
    if (int rc = reserve_grad(r, (size_t)W * H, 0)) return rc;
    hipLaunchKernelGGL(k_raster_render<true>, dim3((unsigned)gx, (unsigned)gy), TPB, 0, st, W, H, gx, (const uint2 *)r->ranges,
                       (const uint32_t *)r->vals[1], (const float4 *)r->rec0, (const float4 *)r->rec1, (const float *)r->colour,
                       s->bg[0], s->bg[1], s->bg[2], out_color, out_alpha, r->pix_T, r->pix_stop);
    r->grad_frame = true;
    r->grad_n = n; r->grad_tiles = tiles; r->grad_pixels = (size_t)W * H; r->grad_entries = (int64_t)total;
    r->grad_w = W; r->grad_h = H;
  } else {
    hipLaunchKernelGGL(k_raster_render<false>, dim3((unsigned)gx, (unsigned)gy), TPB, 0, st, W, H, gx, (const uint2 *)r->ranges,
                       (const uint32_t *)r->vals[1], (const float4 *)r->rec0, (const float4 *)r->rec1, (const float *)r->colour,
                       s->bg[0], s->bg[1], s->bg[2], out_color, out_alpha, (float *)nullptr, (uint32_t *)nullptr);
  }
  ENTRY_CHECK(hipGetLastError());
  if (r->profile) {
    if (int rc = mark(r, 6)) return rc;
    ENTRY_CHECK(hipEventSynchronize(r->ev[6]));
    for (int k = 0; k < MPMHIP_RASTER_STAGES; ++k) {
      float ms = 0.f;
      ENTRY_CHECK(hipEventElapsedTime(&ms, r->ev[k], r->ev[k + 1]));
      r->stage_ms[k] += ms;
    }
    ++r->profiled_frames;
  }
  return MPMHIP_OK;
}

}  // namespace

extern "C" {

int mpmhip_raster_profile(mpmhip_raster *r, int32_t on, double *stage_ms, int64_t *frames) {
  if (!r) return MPMHIP_ERR_INVALID;
  ENTRY_CHECK(hipSetDevice(r->device));
  if (stage_ms) for (int k = 0; k < MPMHIP_RASTER_STAGES; ++k) stage_ms[k] = r->stage_ms[k];
  if (frames) *frames = r->profiled_frames;
  if (on && !r->profile) {
    for (auto &e : r->ev)
      if (!e) ENTRY_CHECK(hipEventCreate(&e));
    for (double &v : r->stage_ms) v = 0.0;
    r->profiled_frames = 0;
  }
  r->profile = on != 0;
  return MPMHIP_OK;
}

int mpmhip_raster_stats(const mpmhip_raster *r, mpmhip_raster_stats_t *out) {
  if (!r || !out) return MPMHIP_ERR_INVALID;
  ENTRY_CHECK(hipSetDevice(r->device));
  int32_t counts[2] = {0, 0};
  if (r->last_tiles > 0) {
    ENTRY_CHECK(hipMemsetAsync(r->d_counts, 0, sizeof(counts), r->stream));
    const int m = r->last_tiles > r->last_n ? r->last_tiles : r->last_n;
    hipLaunchKernelGGL(k_raster_counts, blocks(m, TPB), TPB, 0, r->stream, r->last_tiles, (const uint2 *)r->ranges, r->last_n,
                       (const uint32_t *)r->touched, r->d_counts);
    ENTRY_CHECK(hipGetLastError());
    ENTRY_CHECK(hipMemcpyAsync(counts, r->d_counts, sizeof(counts), hipMemcpyDeviceToHost, r->stream));
    ENTRY_CHECK(hipStreamSynchronize(r->stream));
  }
  out->n_entries = r->last_entries;
  out->max_tile_entries = counts[0];
  out->n_visible = counts[1];
  out->scratch_bytes = (int64_t)((size_t)r->cap_n * (2 * sizeof(float4) + 3 * sizeof(float) + sizeof(int4)) +
                                 ((size_t)r->cap_n + 1) * (sizeof(uint32_t) + sizeof(uint64_t)) + r->scan_tmp_bytes +
                                 r->cap_e * 2 * (sizeof(uint64_t) + sizeof(uint32_t)) + r->sort_tmp_bytes +
                                 (size_t)r->cap_tiles * sizeof(uint2) + r->cap_pix * (sizeof(float) + sizeof(uint32_t)) +
                                 r->cap_inv * sizeof(uint32_t) + (r->cap_rows + r->cap_xrows) * sizeof(float));
  return MPMHIP_OK;
}

}  // extern "C"
