// shade.hip -- the colours of the appearance loop on the device (train_appearance.py:120-123): mpmhip_shade_colors and
// mpmhip_shade_colors_backward.  The math is shade_math.hpp; the kernels here are one thread per item over it.  HBM-bound rows, no
// LDS: each lane reads its own coefficient rows (12 B + 12 B per coefficient in use above the first), as k_raster_preprocess does for shs.
// Per Gaussian, degree 3 and a map: forward 4 B binding + 8 B uv + 16 B taps (gathered) + 12 B mean + 192 B coefficients in, 12 B out
// = 244 B; backward stage 1 the same 232 B + 12 B upstream in, 192 B + 12 B + 4 B out = 452 B.  Stage 2 per face: 8 B of table +
// 8 B per Gaussian of the face in, 4 B out.  Stage 3 per texel: 8 B of table + 16 B per tap (item, uv, dS) in, 4 B out.
// The two per-Gaussian kernels are compiled once per degree, so that the coefficient loops unroll and the rows stay in registers.
// No floating-point atomics: stages 2 and 3 are serial walks of a CSR segment in ascending index, so two runs give the same bits
// whatever the launch geometry.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "entry.hpp"
#include "shade_math.hpp"

namespace {

using namespace entry;
constexpr int TPB = 256;

template <int DEG>
__global__ void __launch_bounds__(TPB) k_shade_forward(int n, int n_f, const int32_t *binding, const float *means3D, const float *campos, int n_coeffs,
                                const float *dc, const float *rest, const float *map, int H, int W, const float *face_uv,
                                float *colors) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  shade::forward(i, n_f, binding, means3D, campos, DEG, n_coeffs, dc, rest, map, H, W, face_uv, colors);
}

template <int DEG>
__global__ void __launch_bounds__(TPB) k_shade_backward_gaussian(int n, int n_f, const int32_t *binding, const float *means3D, const float *campos,
                                          int n_coeffs, const float *dc, const float *rest, const float *map, int H, int W,
                                          const float *face_uv, const float *g_colors, float *d_dc, float *d_rest, float *d_means3D,
                                          float *ds) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  shade::backward_gaussian(i, n_f, binding, means3D, campos, DEG, n_coeffs, dc, rest, map, H, W, face_uv, g_colors, d_dc, d_rest,
                           d_means3D, ds);
}

__global__ void k_shade_face_sum(int n_f, const int32_t *face_start, const int32_t *face_items, const float *ds, float *dS) {
  int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_f) return;
  shade::face_sum(f, face_start, face_items, ds, dS);
}

__global__ void k_shade_texel_sum(int n_t, const int32_t *texel_start, const int32_t *texel_items, int H, int W, const float *face_uv,
                                  const float *dS, float *d_map) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_t) return;
  shade::texel_sum(t, texel_start, texel_items, H, W, face_uv, dS, d_map);
}

// what both entry points require of the inputs they share; n_faces counts only where a map is given
int check_inputs(int32_t n, int32_t n_faces, const int32_t *binding, const float *means3D, const float *campos, int32_t sh_degree,
                 int32_t n_sh_coeffs, const float *features_dc, const float *features_rest, const float *shadow_map, int32_t map_h,
                 int32_t map_w, const float *face_uv) {
  if (n < 0 || n_faces < 0) return MPMHIP_ERR_INVALID;
  if (!features_dc && !shadow_map) return MPMHIP_ERR_INVALID;
  if (features_dc) {
    if (sh_degree < 0 || sh_degree > 3 || n_sh_coeffs < (sh_degree + 1) * (sh_degree + 1)) return MPMHIP_ERR_INVALID;
    if (!campos || (n > 0 && (!means3D || (n_sh_coeffs > 1 && !features_rest)))) return MPMHIP_ERR_INVALID;
  }
  if (shadow_map) {
    if (map_h <= 0 || map_w <= 0 || (int64_t)map_h * map_w >= INT32_MAX) return MPMHIP_ERR_INVALID;
    if ((n_faces > 0 && !face_uv) || (n > 0 && !binding)) return MPMHIP_ERR_INVALID;
  }
  return MPMHIP_OK;
}

}  // namespace

extern "C" {

int mpmhip_shade_colors(int32_t device, void *stream, int32_t n, int32_t n_faces, const int32_t *binding, const float *means3D,
                        const float *campos, int32_t sh_degree, int32_t n_sh_coeffs, const float *features_dc, const float *features_rest,
                        const float *shadow_map, int32_t map_h, int32_t map_w, const float *face_uv, float *out_colors) {
  if (int rc = check_inputs(n, n_faces, binding, means3D, campos, sh_degree, n_sh_coeffs, features_dc, features_rest, shadow_map, map_h,
                            map_w, face_uv))
    return rc;
  if (!out_colors) return MPMHIP_ERR_INVALID;
  if (int rc = device_in_range(device)) return rc;
  if (n == 0) return MPMHIP_OK;
  ENTRY_CHECK(hipSetDevice(device));
  auto *kernel = k_shade_forward<0>;  // without features the degree plays no part
  if (features_dc) kernel = sh_degree == 1 ? k_shade_forward<1> : sh_degree == 2 ? k_shade_forward<2> : sh_degree == 3 ? k_shade_forward<3> : kernel;
  hipLaunchKernelGGL(kernel, blocks(n, TPB), TPB, 0, (hipStream_t)stream, n, n_faces, binding, means3D, campos, n_sh_coeffs, features_dc,
                     features_rest, shadow_map, map_h, map_w, face_uv, out_colors);
  return check(hipGetLastError());
}

int mpmhip_shade_colors_backward(int32_t device, void *stream, int32_t n, int32_t n_faces, const int32_t *binding, const float *means3D,
                                 const float *campos, int32_t sh_degree, int32_t n_sh_coeffs, const float *features_dc,
                                 const float *features_rest, const float *shadow_map, int32_t map_h, int32_t map_w, const float *face_uv,
                                 const float *g_colors, float *d_features_dc, float *d_features_rest, float *d_means3D,
                                 const int32_t *face_start, const int32_t *face_items, const int32_t *texel_start,
                                 const int32_t *texel_items, float *d_shadow_map, float *scratch) {
  if (int rc = check_inputs(n, n_faces, binding, means3D, campos, sh_degree, n_sh_coeffs, features_dc, features_rest, shadow_map, map_h,
                            map_w, face_uv))
    return rc;
  if (d_shadow_map) {  // the two tables and the scratch are needed only here
    if (!shadow_map || !face_start || !texel_start || !scratch) return MPMHIP_ERR_INVALID;
    if (n > 0 && !face_items) return MPMHIP_ERR_INVALID;
    if (n_faces > 0 && !texel_items) return MPMHIP_ERR_INVALID;
  }
  if (!features_dc && (d_features_dc || d_features_rest)) return MPMHIP_ERR_INVALID;
  if (d_features_rest && n_sh_coeffs < 2) return MPMHIP_ERR_INVALID;
  const bool per_gaussian = n > 0 && (d_features_dc || d_features_rest || d_means3D || d_shadow_map);
  if (int rc = device_in_range(device)) return rc;
  if (!d_shadow_map && !per_gaussian) return MPMHIP_OK;
  ENTRY_CHECK(hipSetDevice(device));
  float *ds = d_shadow_map ? scratch : nullptr, *dS = d_shadow_map ? scratch + n : nullptr;
  if (per_gaussian) {
    auto *kernel = k_shade_backward_gaussian<0>;
    if (features_dc)
      kernel = sh_degree == 1 ? k_shade_backward_gaussian<1> : sh_degree == 2 ? k_shade_backward_gaussian<2>
               : sh_degree == 3 ? k_shade_backward_gaussian<3> : kernel;
    hipLaunchKernelGGL(kernel, blocks(n, TPB), TPB, 0, (hipStream_t)stream, n, n_faces, binding, means3D, campos, n_sh_coeffs, features_dc, features_rest, shadow_map, map_h, map_w, face_uv, g_colors,
                       d_features_dc, d_features_rest, d_means3D, ds);
    ENTRY_CHECK(hipGetLastError());
  }
  if (d_shadow_map) {
    if (n_faces > 0) {
      hipLaunchKernelGGL(k_shade_face_sum, blocks(n_faces, TPB), TPB, 0, (hipStream_t)stream, n_faces, face_start, face_items, ds, dS);
      ENTRY_CHECK(hipGetLastError());
    }
    const int n_t = map_h * map_w;
    hipLaunchKernelGGL(k_shade_texel_sum, blocks(n_t, TPB), TPB, 0, (hipStream_t)stream, n_t, texel_start, texel_items, map_h, map_w,
                       face_uv, dS, d_shadow_map);
    ENTRY_CHECK(hipGetLastError());
  }
  return MPMHIP_OK;
}

}  // extern "C"
