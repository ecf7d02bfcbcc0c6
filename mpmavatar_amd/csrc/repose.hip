// repose.hip -- re-posing on the device (utils/smplx_deformer.py:164-337): the k-nearest search (knn_device.hpp), Shepard's weights
// over it with the gather of the body's skinning weights, and linear-blend skinning to a pose and back to the T-pose.  The math is
// repose_math.hpp.
//   k_shepard  one lane per (point, joint), joints fastest: W[p, j] = sum_k w_k lbs[idx_k, j].  The K weights are recomputed by
//              every lane of a point (K clamps, K reciprocals); no [P, K, J] tensor exists.  Without lbs the lanes of a point write
//              the K weights themselves (weights_from_k_closest_verts).
//   k_skin     grid x = tile of SKIN_TPB points (one per lane), y = chunk of SKIN_FRAMES frames.  The tile's rows of W are read once,
//              coalesced, into LDS (row stride J | 1, so that a lane reading its own row meets no bank conflict) and stay there for
//              the whole frame chunk; A[b] is wave-uniform and read straight from memory (scalar loads).  Per frame a lane blends its
//              T (16 fma per joint, ascending j), inverts it on the way to the T-pose, transforms its point and, only when asked,
//              writes the 16 entries of T.  W [1, P, J] serves every frame: the reference's repeat is never materialised.
// No atomics, a fixed summation order: the same input gives the same bits.  Nothing here allocates or synchronises.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "entry.hpp"
#include "knn_device.hpp"
#include "repose_math.hpp"

namespace {

using namespace entry;
constexpr int TPB = 256;
constexpr int SKIN_TPB = 128;
constexpr int SKIN_FRAMES = 8;
constexpr int SKIN_MAX_JOINTS = MPMHIP_SKIN_MAX_JOINTS;
static_assert(SKIN_TPB * (SKIN_MAX_JOINTS | 1) * 4 <= 64 * 1024, "the W tile fits the default dynamic LDS limit");

__global__ __launch_bounds__(TPB) void k_shepard(int n, int k, int power, const float *__restrict__ d2, const int32_t *__restrict__ idx,
                                                 const float *__restrict__ lbs, int n_verts, int n_joints, float *__restrict__ out) {
  const int64_t g = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (g >= (int64_t)n * n_joints) return;
  const int64_t p = g / n_joints;
  const int j = (int)(g - p * n_joints);
  float w[knn::MAX_K];
  rp::shepard_weights(d2 + (size_t)p * k, k, power, w);
  if (lbs) {
    out[g] = rp::shepard_entry(w, idx + (size_t)p * k, k, lbs, n_verts, n_joints, j);
  } else {  // the weights themselves (n_joints == k here); a select, so that w is never indexed dynamically
    float r = 0.f;
#pragma unroll
    for (int i = 0; i < knn::MAX_K; ++i) r = i == j ? w[i] : r;
    out[g] = r;
  }
}

// verts [vb ? B : 1][P][3], W [wb ? B : 1][P][J], A [B][J][16], transl [B][3] or NULL, scale [sb ? B : 1] or NULL
template <bool INVERSE>
__global__ __launch_bounds__(SKIN_TPB) void k_skin(int n_frames, int n_points, int n_joints, const float *__restrict__ verts, int vb,
                                                   const float *__restrict__ W, int wb, const float *__restrict__ A,
                                                   const float *__restrict__ transl, const float *__restrict__ scale, int sb,
                                                   float *__restrict__ out, float *__restrict__ out_T) {
  extern __shared__ __attribute__((aligned(16))) float wl[];  // [SKIN_TPB][js]
  const int js = n_joints | 1;
  const int tid = threadIdx.x;
  const int64_t p0 = (int64_t)blockIdx.x * SKIN_TPB;
  const int np = (int)min((int64_t)SKIN_TPB, (int64_t)n_points - p0);
  const int64_t p = p0 + tid;
  const int b0 = blockIdx.y * SKIN_FRAMES, b1 = min(b0 + SKIN_FRAMES, n_frames);
  const int tile_items = np * n_joints;

  for (int b = b0; b < b1; ++b) {
    if (b == b0 || wb) {  // uniform over the workgroup
      __syncthreads();
      const float *wt = W + ((size_t)(wb ? b : 0) * n_points + (size_t)p0) * n_joints;
      for (int t = tid; t < tile_items; t += SKIN_TPB) {
        const int r = t / n_joints;
        wl[r * js + (t - r * n_joints)] = wt[t];
      }
      __syncthreads();
    }
    if (p >= n_points) continue;  // after the barriers of this frame; the next frame's barriers are still reached by every lane
    float T[16], v[3], o[3];
    rp::blend(wl + tid * js, n_joints, A + (size_t)b * n_joints * 16, T);
    const float *vp = verts + ((size_t)(vb ? b : 0) * n_points + (size_t)p) * 3;
    v[0] = vp[0]; v[1] = vp[1]; v[2] = vp[2];
    const float *tr = transl ? transl + 3 * (size_t)b : nullptr;
    const float *sc = scale ? scale + (sb ? b : 0) : nullptr;
    const size_t row = (size_t)b * n_points + (size_t)p;
    if (INVERSE) {
      float Ti[16];
      rp::to_tpose(T, v, tr, sc, Ti, o);
      if (out_T) {
#pragma unroll
        for (int e = 0; e < 16; ++e) out_T[row * 16 + e] = Ti[e];
      }
    } else {
      rp::to_pose(T, v, tr, sc, o);
      if (out_T) {
#pragma unroll
        for (int e = 0; e < 16; ++e) out_T[row * 16 + e] = T[e];
      }
    }
    out[row * 3] = o[0]; out[row * 3 + 1] = o[1]; out[row * 3 + 2] = o[2];
  }
}

int skin(bool inverse, int32_t device, void *stream, const float *verts, int32_t verts_batched, const float *w, int32_t w_batched,
         const float *A, int32_t n_frames, int32_t n_points, int32_t n_joints, const float *transl, const float *scale, int32_t scale_batched,
         float *out_points, float *out_T) {
  if (n_frames < 0 || n_points < 0 || n_joints < 1 || n_joints > SKIN_MAX_JOINTS) return MPMHIP_ERR_INVALID;
  if ((int64_t)n_frames * n_points > INT32_MAX / 16) return MPMHIP_ERR_INVALID;  // rows of T stay an int32 count of floats
  const bool work = n_frames > 0 && n_points > 0;
  if (work && (!verts || !w || !A || !out_points)) return MPMHIP_ERR_INVALID;
  if (int rc = device_in_range(device)) return rc;
  if (!work) return MPMHIP_OK;
  ENTRY_CHECK(hipSetDevice(device));
  const dim3 grid(blocks(n_points, SKIN_TPB), blocks(n_frames, SKIN_FRAMES));
  if (grid.y > 65535) return MPMHIP_ERR_INVALID;
  const size_t lds = (size_t)SKIN_TPB * (n_joints | 1) * sizeof(float);
  if (inverse)
    hipLaunchKernelGGL(k_skin<true>, grid, SKIN_TPB, lds, (hipStream_t)stream, n_frames, n_points, n_joints, verts, verts_batched, w, w_batched, A,
                       transl, scale, scale_batched, out_points, out_T);
  else
    hipLaunchKernelGGL(k_skin<false>, grid, SKIN_TPB, lds, (hipStream_t)stream, n_frames, n_points, n_joints, verts, verts_batched, w, w_batched, A,
                       transl, scale, scale_batched, out_points, out_T);
  return check(hipGetLastError());
}

bool knn_args_ok(int32_t n, int32_t m, int32_t dim, int32_t k, int32_t slices) {
  return n >= 0 && m >= 1 && (dim == 3 || dim == 6) && k >= 1 && k <= knn::MAX_K && k <= m && slices >= 0;
}

}  // namespace

extern "C" {

int mpmhip_knn_scratch(int32_t n, int32_t m, int32_t dim, int32_t k, int32_t slices, int64_t *out_len) {
  if (!knn_args_ok(n, m, dim, k, slices) || !out_len) return MPMHIP_ERR_INVALID;
  const knn::Plan p = knn::plan(n, m, slices);
  *out_len = (int64_t)p.slices * n * k;
  return MPMHIP_OK;
}

int mpmhip_knn(int32_t device, void *stream, const float *queries, int32_t n, const float *targets, int32_t m, int32_t dim, int32_t k,
               int32_t slices, uint64_t *scratch, int64_t scratch_len, float *out_dists, int32_t *out_idx) {
  if (!knn_args_ok(n, m, dim, k, slices) || !targets) return MPMHIP_ERR_INVALID;
  const knn::Plan p = knn::plan(n, m, slices);
  if (n > 0 && (!queries || !scratch || !out_dists || !out_idx || scratch_len < (int64_t)p.slices * n * k)) return MPMHIP_ERR_INVALID;
  if (int rc = device_in_range(device)) return rc;
  if (n == 0) return MPMHIP_OK;
  ENTRY_CHECK(hipSetDevice(device));
  return knn::launch_knn((hipStream_t)stream, queries, n, targets, m, dim, k, p, scratch, out_dists, out_idx);
}

int mpmhip_shepard_weights(int32_t device, void *stream, const float *dists, const int32_t *idx, int32_t n, int32_t k, int32_t power,
                           const float *lbs_weights, int32_t n_verts, int32_t n_joints, float *out_w) {
  if (n < 0 || k < 1 || k > knn::MAX_K || power < 0) return MPMHIP_ERR_INVALID;
  if (lbs_weights && (n_verts < 1 || n_joints < 1)) return MPMHIP_ERR_INVALID;
  if (!lbs_weights) n_joints = k;  // the weights alone
  if ((int64_t)n * n_joints > INT32_MAX) return MPMHIP_ERR_INVALID;
  if (n > 0 && (!dists || !out_w || (lbs_weights && !idx))) return MPMHIP_ERR_INVALID;
  if (int rc = device_in_range(device)) return rc;
  if (n == 0) return MPMHIP_OK;
  ENTRY_CHECK(hipSetDevice(device));
  hipLaunchKernelGGL(k_shepard, blocks((int64_t)n * n_joints, TPB), TPB, 0, (hipStream_t)stream, n, k, power, dists, idx, lbs_weights, n_verts,
                     n_joints, out_w);
  return check(hipGetLastError());
}

int mpmhip_skin_to_pose(int32_t device, void *stream, const float *verts, int32_t verts_batched, const float *w, int32_t w_batched,
                        const float *A, int32_t n_frames, int32_t n_points, int32_t n_joints, const float *transl, const float *scale,
                        int32_t scale_batched, float *out_points, float *out_T) {
  return skin(false, device, stream, verts, verts_batched, w, w_batched, A, n_frames, n_points, n_joints, transl, scale, scale_batched, out_points,
              out_T);
}

int mpmhip_skin_to_tpose(int32_t device, void *stream, const float *verts, int32_t verts_batched, const float *w, int32_t w_batched,
                         const float *A, int32_t n_frames, int32_t n_points, int32_t n_joints, const float *transl, const float *scale,
                         int32_t scale_batched, float *out_points, float *out_T) {
  return skin(true, device, stream, verts, verts_batched, w, w_batched, A, n_frames, n_points, n_joints, transl, scale, scale_batched, out_points,
              out_T);
}

}  // extern "C"
