// ao.hip -- the ambient-occlusion bake on the device (blender/bake.py, called from train_material_params.py:819-822): the six
// mpmhip_ao_* entry points.  The math is ao_math.hpp; what is added here is how the work is spread.
//   coverage (once per mesh)   k_ao_cov_clear, k_ao_cov_claim (one lane per face, integer atomicMin over the texels of its UV
//                              box: the lowest face wins whatever the order), k_ao_cov_finish (one lane per texel: barycentrics)
//   grid (per frame)           k_ao_prepare      one lane per face: the 48-byte record; per workgroup a partial box and a partial
//                                                sum of edge lengths, reduced in LDS in a fixed tree
//                              k_ao_grid_setup   one lane: the partials in index order -> ao::Grid
//                              k_ao_count        one lane per face: +1 on every cell of ao::for_face_cells
//                              rocprim::exclusive_scan over the cap_cells + 1 counters (saturating, so that an overflow shows)
//                              k_ao_fill         the same walk; an integer cursor per cell places the face
//                              The order of the faces inside a cell depends on the order the atomics retire in and is not
//                              deterministic.  The result is: occlusion is an any-hit boolean, so the order in which a cell's
//                              faces are tried cannot change it.
//   trace (per frame)          k_ao_trace        one wave64 per covered texel, lanes striding the S rays; every ray is a 3-D DDA
//                                                walk with an early exit at its first hit; the texel's count is the popcount of
//                                                the wave's ballot, accumulated over the strides; one fp32 store per texel
//   margin                     k_ao_margin       one lane per texel
// All 64 rays of a stride leave from one point, so in the first cells every lane reads the same cell range and the same face
// records: those loads are one address per wave and are served as broadcasts from the vector cache.  The records are NOT staged in
// LDS: the staged set would be the first cell only, lanes leave it at different steps, and a copy plus a barrier-free wave-level
// handshake buys nothing over a broadcast load that already hits the cache.  Nobody has measured the alternative.
// No floating-point atomics anywhere; integer atomics in k_ao_cov_claim (min), k_ao_count and k_ao_fill (add) only.
#include <hip/hip_runtime.h>

#include <cstdint>

#include <rocprim/device/device_scan.hpp>

#include "ao_math.hpp"
#include "entry.hpp"

namespace {

using namespace entry;
constexpr int TPB = 256;
constexpr int WAVE = 64;
constexpr int PREP_BLOCKS = 64;     // partials of the box and of the edge sum: a fixed number, so the sum has one order
constexpr int PARTIAL = 8;          // floats per partial: min xyz, max xyz, edge sum, unused

struct SatAdd {  // counts that would pass 2^32 - 1 stay there: "more than cap_entries" survives the scan
  __host__ __device__ uint32_t operator()(uint32_t a, uint32_t b) const {
    const uint64_t s = (uint64_t)a + b;
    return s > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)s;
  }
};

// the caller's scratch, cut up; every section 256-byte aligned
struct Layout {
  size_t tri, partial, grid, count, start, items, scan_tmp, bytes;
};
Layout layout(int32_t n_faces, int32_t cap_cells, int32_t cap_entries, size_t scan_tmp_bytes) {
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  Layout l;
  size_t at = 0;
  l.tri = at; at = up(at + (size_t)n_faces * sizeof(ao::Tri));
  l.partial = at; at = up(at + (size_t)PREP_BLOCKS * PARTIAL * sizeof(float));
  l.grid = at; at = up(at + sizeof(ao::Grid));
  l.count = at; at = up(at + ((size_t)cap_cells + 1) * sizeof(uint32_t));
  l.start = at; at = up(at + ((size_t)cap_cells + 1) * sizeof(uint32_t));
  l.items = at; at = up(at + (size_t)cap_entries * sizeof(int32_t));
  l.scan_tmp = at; at = up(at + scan_tmp_bytes);
  l.bytes = at;
  return l;
}

int scan_tmp_bytes(int32_t cap_cells, hipStream_t st, size_t *bytes) {
  *bytes = 0;
  return check(rocprim::exclusive_scan(nullptr, *bytes, (uint32_t *)nullptr, (uint32_t *)nullptr, 0u, (size_t)cap_cells + 1, SatAdd(), st));
}

// ---- coverage

__global__ void k_ao_cov_clear(int n_t, int32_t *cov_face) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n_t) cov_face[t] = INT32_MAX;
}

__global__ void k_ao_cov_claim(int n_f, const int32_t *faces, const int32_t *ft, const float *vt, int H, int W, int32_t *cov_face) {
  int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_f) return;
  ao::face_texels(f, faces, ft, vt, H, W, [&](int texel) { atomicMin(&cov_face[texel], f); });
}

__global__ void k_ao_cov_finish(int n_t, const int32_t *ft, const float *vt, int H, int W, int32_t *cov_face, float *cov_bary) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_t) return;
  const int32_t f = cov_face[t];
  if (f == INT32_MAX) {
    cov_face[t] = -1;
    cov_bary[2 * t] = 0.f;
    cov_bary[2 * t + 1] = 0.f;
  } else {
    ao::texel_bary(t, f, ft, vt, H, W, cov_bary + 2 * (int64_t)t);
  }
}

// ---- frames

__device__ __forceinline__ ao::Frame frame_of(int texel, int32_t f, const float *verts, const int32_t *faces, const float *cov_bary, const float *rot) {
  return ao::texel_frame(ao::load3(verts, faces[3 * (int64_t)f]), ao::load3(verts, faces[3 * (int64_t)f + 1]),
                         ao::load3(verts, faces[3 * (int64_t)f + 2]), cov_bary[2 * (int64_t)texel], cov_bary[2 * (int64_t)texel + 1],
                         rot[2 * (int64_t)texel], rot[2 * (int64_t)texel + 1]);
}

__global__ void k_ao_texel_frames(int n_t, const float *verts, const int32_t *faces, const int32_t *cov_face, const float *cov_bary,
                                  const float *rot, float *origin, float *normal, float *tangent) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_t) return;
  const int32_t f = cov_face[t];
  ao::Frame fr{};
  if (f >= 0) fr = frame_of(t, f, verts, faces, cov_bary, rot);
  ao::store3(origin, t, fr.p);
  ao::store3(normal, t, fr.n);
  ao::store3(tangent, t, fr.t);
}

// ---- grid

__global__ void __launch_bounds__(TPB) k_ao_prepare(int n_f, const float *verts, const int32_t *faces, ao::Tri *tri, float *partial) {
  __shared__ float red[PARTIAL - 1][TPB];
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY}, edges = 0.f;
  for (int f = blockIdx.x * TPB + threadIdx.x; f < n_f; f += PREP_BLOCKS * TPB) {
    const ao::V3 v[3] = {ao::load3(verts, faces[3 * (int64_t)f]), ao::load3(verts, faces[3 * (int64_t)f + 1]), ao::load3(verts, faces[3 * (int64_t)f + 2])};
    tri[f] = ao::make_tri(v[0], v[1], v[2]);
    for (int k = 0; k < 3; ++k) {
      mn[0] = fminf(mn[0], v[k].x); mn[1] = fminf(mn[1], v[k].y); mn[2] = fminf(mn[2], v[k].z);
      mx[0] = fmaxf(mx[0], v[k].x); mx[1] = fmaxf(mx[1], v[k].y); mx[2] = fmaxf(mx[2], v[k].z);
      const ao::V3 e = ao::sub(v[(k + 1) % 3], v[k]);
      edges += sqrtf(ao::dot(e, e));
    }
  }
  for (int k = 0; k < 3; ++k) { red[k][threadIdx.x] = mn[k]; red[3 + k][threadIdx.x] = mx[k]; }
  red[6][threadIdx.x] = edges;
  __syncthreads();
  for (int s = TPB / 2; s > 0; s >>= 1) {  // a fixed tree: the same sum on every run
    if ((int)threadIdx.x < s) {
      for (int k = 0; k < 3; ++k) {
        red[k][threadIdx.x] = fminf(red[k][threadIdx.x], red[k][threadIdx.x + s]);
        red[3 + k][threadIdx.x] = fmaxf(red[3 + k][threadIdx.x], red[3 + k][threadIdx.x + s]);
      }
      red[6][threadIdx.x] += red[6][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x < PARTIAL) partial[blockIdx.x * PARTIAL + threadIdx.x] = threadIdx.x < PARTIAL - 1 ? red[threadIdx.x][0] : 0.f;
}

__global__ void k_ao_grid_setup(int n_f, const float *partial, int32_t cap_cells, ao::Grid *grid) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY}, edges = 0.f;
  for (int b = 0; b < PREP_BLOCKS; ++b) {
    for (int k = 0; k < 3; ++k) {
      mn[k] = fminf(mn[k], partial[b * PARTIAL + k]);
      mx[k] = fmaxf(mx[k], partial[b * PARTIAL + 3 + k]);
    }
    edges += partial[b * PARTIAL + 6];
  }
  *grid = ao::grid_setup(mn, mx, n_f > 0 ? edges / (3.f * (float)n_f) : 0.f, cap_cells);
}

__global__ void k_ao_count(int n_f, const float *verts, const int32_t *faces, const ao::Grid *grid, uint32_t *count) {
  int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_f) return;
  const ao::Grid g = *grid;
  ao::for_face_cells(g, verts, faces, f, [&](int32_t cell) { atomicAdd(&count[cell], 1u); });
}

__global__ void k_ao_fill(int n_f, const float *verts, const int32_t *faces, const ao::Grid *grid, const uint32_t *start, uint32_t *cursor,
                          int32_t cap_entries, int32_t *items) {
  int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_f) return;
  const ao::Grid g = *grid;
  ao::for_face_cells(g, verts, faces, f, [&](int32_t cell) {
    const uint64_t at = (uint64_t)start[cell] + atomicAdd(&cursor[cell], 1u);
    if (at < (uint64_t)cap_entries) items[at] = f;  // past the capacity nothing is written; k_ao_trace sees the total and says so
  });
}

// ---- trace

__global__ void __launch_bounds__(TPB) k_ao_trace(int n_cov, const int32_t *cov_list, const int32_t *cov_face, const float *cov_bary,
                                                  const float *verts, const int32_t *faces, const float *rot, int S, const float *dirs,
                                                  const ao::Grid *grid, const uint32_t *start, const int32_t *items, int32_t cap_cells,
                                                  int32_t cap_entries, const ao::Tri *tri, float bias, float tmax, float *out) {
  const int w = blockIdx.x * (TPB / WAVE) + (int)threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
  if (w >= n_cov) return;  // the whole wave
  const int texel = cov_list[w];
  if (start[cap_cells] > (uint32_t)cap_entries) {  // this frame's grid did not fit
    if (lane == 0) out[texel] = NAN;
    return;
  }
  const int32_t own = cov_face[texel];
  const ao::Frame fr = frame_of(texel, own, verts, faces, cov_bary, rot);
  if (!fr.ok) {
    if (lane == 0) out[texel] = 0.f;
    return;
  }
  const ao::Grid g = *grid;
  int occluded = 0;
  for (int base = 0; base < S; base += WAVE) {  // every lane takes every turn: the ballot needs the whole wave
    const int i = base + lane;
    bool hit = false;
    if (i < S) hit = ao::ray_occluded(g, start, items, tri, own, fr.p, ao::ray_dir(fr, dirs, i), bias, tmax);
    occluded += __builtin_popcountll(__ballot(hit));
  }
  if (lane == 0) out[texel] = ao::ao_value(occluded, S);
}

__global__ void k_ao_margin(int H, int W, const float *in_val, const uint8_t *in_mask, float *out_val, uint8_t *out_mask) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= H * W) return;
  ao::margin_texel(t, H, W, in_val, in_mask, out_val, out_mask);
}

bool map_ok(int32_t H, int32_t W) { return H > 0 && W > 0 && (int64_t)H * W < INT32_MAX; }
bool caps_ok(int32_t n_faces, int32_t cap_cells, int32_t cap_entries) { return n_faces >= 0 && cap_cells >= 1 && cap_cells < INT32_MAX && cap_entries >= 1; }

}  // namespace

extern "C" {

int mpmhip_ao_coverage(int32_t device, void *stream, const int32_t *faces, const int32_t *ft, int32_t n_faces, const float *vt, int32_t n_vt,
                       int32_t map_h, int32_t map_w, int32_t *cov_face, float *cov_bary) {
  if (n_faces < 0 || n_vt < 0 || !map_ok(map_h, map_w) || !cov_face || !cov_bary) return MPMHIP_ERR_INVALID;
  if (n_faces > 0 && (!faces || !ft || !vt || n_vt == 0)) return MPMHIP_ERR_INVALID;
  if (int rc = select_device(device)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int n_t = map_h * map_w;
  hipLaunchKernelGGL(k_ao_cov_clear, blocks(n_t, TPB), TPB, 0, st, n_t, cov_face);
  ENTRY_CHECK(hipGetLastError());
  if (n_faces > 0) {
    hipLaunchKernelGGL(k_ao_cov_claim, blocks(n_faces, TPB), TPB, 0, st, n_faces, faces, ft, vt, map_h, map_w, cov_face);
    ENTRY_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_ao_cov_finish, blocks(n_t, TPB), TPB, 0, st, n_t, ft, vt, map_h, map_w, cov_face, cov_bary);
  return check(hipGetLastError());
}

int mpmhip_ao_scratch_bytes(int32_t device, int32_t n_faces, int32_t cap_cells, int32_t cap_entries, int64_t *out_bytes) {
  if (!out_bytes || !caps_ok(n_faces, cap_cells, cap_entries)) return MPMHIP_ERR_INVALID;
  if (int rc = select_device(device)) return rc;
  size_t tmp = 0;
  if (int rc = scan_tmp_bytes(cap_cells, nullptr, &tmp)) return rc;
  *out_bytes = (int64_t)layout(n_faces, cap_cells, cap_entries, tmp).bytes;
  return MPMHIP_OK;
}

int mpmhip_ao_texel_frames(int32_t device, void *stream, const float *verts, const int32_t *faces, int32_t n_faces, int32_t map_h,
                           int32_t map_w, const int32_t *cov_face, const float *cov_bary, const float *rot, float *origin, float *normal,
                           float *tangent) {
  if (n_faces < 0 || !map_ok(map_h, map_w) || !cov_face || !cov_bary || !rot || !origin || !normal || !tangent) return MPMHIP_ERR_INVALID;
  if (n_faces > 0 && (!verts || !faces)) return MPMHIP_ERR_INVALID;
  if (int rc = select_device(device)) return rc;
  const int n_t = map_h * map_w;
  hipLaunchKernelGGL(k_ao_texel_frames, blocks(n_t, TPB), TPB, 0, (hipStream_t)stream, n_t, verts, faces, cov_face, cov_bary, rot, origin,
                     normal, tangent);
  return check(hipGetLastError());
}

int mpmhip_ao_build_grid(int32_t device, void *stream, const float *verts, const int32_t *faces, int32_t n_faces, int32_t cap_cells,
                         int32_t cap_entries, void *scratch, int64_t scratch_bytes) {
  if (!caps_ok(n_faces, cap_cells, cap_entries) || !scratch || (n_faces > 0 && (!verts || !faces))) return MPMHIP_ERR_INVALID;
  if (int rc = select_device(device)) return rc;
  hipStream_t st = (hipStream_t)stream;
  size_t tmp = 0;
  if (int rc = scan_tmp_bytes(cap_cells, st, &tmp)) return rc;
  const Layout l = layout(n_faces, cap_cells, cap_entries, tmp);
  if (scratch_bytes < 0 || (size_t)scratch_bytes < l.bytes) return MPMHIP_ERR_INVALID;
  char *base = (char *)scratch;
  ao::Tri *tri = (ao::Tri *)(base + l.tri);
  float *partial = (float *)(base + l.partial);
  ao::Grid *grid = (ao::Grid *)(base + l.grid);
  uint32_t *count = (uint32_t *)(base + l.count), *start = (uint32_t *)(base + l.start);
  int32_t *items = (int32_t *)(base + l.items);
  const size_t counters = ((size_t)cap_cells + 1) * sizeof(uint32_t);
  hipLaunchKernelGGL(k_ao_prepare, PREP_BLOCKS, TPB, 0, st, n_faces, verts, faces, tri, partial);
  ENTRY_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_ao_grid_setup, 1, WAVE, 0, st, n_faces, partial, cap_cells, grid);
  ENTRY_CHECK(hipGetLastError());
  ENTRY_CHECK(hipMemsetAsync(count, 0, counters, st));
  if (n_faces > 0) {
    hipLaunchKernelGGL(k_ao_count, blocks(n_faces, TPB), TPB, 0, st, n_faces, verts, faces, grid, count);
    ENTRY_CHECK(hipGetLastError());
  }
  ENTRY_CHECK(rocprim::exclusive_scan(base + l.scan_tmp, tmp, count, start, 0u, (size_t)cap_cells + 1, SatAdd(), st));
  ENTRY_CHECK(hipMemsetAsync(count, 0, counters, st));  // the counters become the cursors
  if (n_faces > 0) {
    hipLaunchKernelGGL(k_ao_fill, blocks(n_faces, TPB), TPB, 0, st, n_faces, verts, faces, grid, start, count, cap_entries, items);
    ENTRY_CHECK(hipGetLastError());
  }
  return MPMHIP_OK;
}

int mpmhip_ao_trace(int32_t device, void *stream, const float *verts, const int32_t *faces, int32_t n_faces, const int32_t *cov_face,
                    const float *cov_bary, const int32_t *cov_list, int32_t n_cov, const float *rot, const float *dirs, int32_t samples,
                    float bias, float max_distance, int32_t cap_cells, int32_t cap_entries, void *scratch, int64_t scratch_bytes, float *ao_out) {
  if (!caps_ok(n_faces, cap_cells, cap_entries) || n_cov < 0 || samples < 1 || samples > ao::MAX_SAMPLES || !scratch || !ao_out)
    return MPMHIP_ERR_INVALID;
  if (n_cov > 0 && (!verts || !faces || !cov_face || !cov_bary || !cov_list || !rot || !dirs || n_faces == 0)) return MPMHIP_ERR_INVALID;
  if (int rc = select_device(device)) return rc;
  hipStream_t st = (hipStream_t)stream;
  size_t tmp = 0;
  if (int rc = scan_tmp_bytes(cap_cells, st, &tmp)) return rc;
  const Layout l = layout(n_faces, cap_cells, cap_entries, tmp);
  if (scratch_bytes < 0 || (size_t)scratch_bytes < l.bytes) return MPMHIP_ERR_INVALID;
  if (n_cov == 0) return MPMHIP_OK;
  char *base = (char *)scratch;
  hipLaunchKernelGGL(k_ao_trace, blocks(n_cov, TPB / WAVE), TPB, 0, st, n_cov, cov_list, cov_face, cov_bary, verts, faces, rot, samples, dirs,
                     (const ao::Grid *)(base + l.grid), (const uint32_t *)(base + l.start), (const int32_t *)(base + l.items), cap_cells,
                     cap_entries, (const ao::Tri *)(base + l.tri), bias, max_distance, ao_out);
  return check(hipGetLastError());
}

int mpmhip_ao_margin(int32_t device, void *stream, int32_t map_h, int32_t map_w, const float *in_val, const uint8_t *in_mask, float *out_val,
                     uint8_t *out_mask) {
  if (!map_ok(map_h, map_w) || !in_val || !in_mask || !out_val || !out_mask || in_val == out_val || in_mask == out_mask) return MPMHIP_ERR_INVALID;
  if (int rc = select_device(device)) return rc;
  hipLaunchKernelGGL(k_ao_margin, blocks((int64_t)map_h * map_w, TPB), TPB, 0, (hipStream_t)stream, map_h, map_w, in_val, in_mask, out_val, out_mask);
  return check(hipGetLastError());
}

}  // extern "C"
