// densify.hip -- densification of the bound Gaussians on the device (scene/gaussian_model.py:378-526, train_appearance.py:245-257):
// mpmhip_densify_stats_add (add_densification_stats and the max_radii2D line, one launch per iteration), mpmhip_densify_plan and
// mpmhip_densify_emit (densify_and_prune: clone, split, prune and the face rule, in the reference's row order) and
// mpmhip_reset_opacity.  The math is densify_math.hpp; the kernels here are one thread per Gaussian, or per output element, over it.
// Plan (nothing of the output exists yet): k_classify takes the bits of every original and adds its rows and flagged rows to its
// face (integer atomics), k_resolve applies the face rule and writes three 0/1 columns -- the original stays, its clone stays, its
// children stay -- into one array [3 n + 1], rocprim::exclusive_scan over that array gives every surviving row its place in
// [kept originals | clones | first children | second children], and k_counts leaves the eight integers the caller reads back: the
// only synchronisation of a densification.  Emit (the caller has sized the output): k_emit writes src, kind, binding and the
// per-face counts, k_gather writes every row-aligned tensor from a descriptor table in one launch (grid.y = tensor).
// Integer atomics only: the same input gives the same bits.  Nothing here allocates or synchronises.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <rocprim/device/device_scan.hpp>

#include "densify_math.hpp"
#include "entry.hpp"

namespace {

using namespace entry;
constexpr int TPB = 256;
constexpr int MAX_T = MPMHIP_DENSIFY_MAX_TENSORS;

// the caller's scratch, cut up; every section 256-byte aligned
struct Layout {
  size_t bits, face_rows, face_flagged, keep, at, scan_tmp, bytes;
};
Layout layout(int32_t n, int32_t n_faces, size_t scan_tmp_bytes) {
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  Layout l;
  size_t at = 0;
  l.bits = at; at = up(at + (size_t)n);
  l.face_rows = at; at = up(at + (size_t)n_faces * sizeof(int32_t));
  l.face_flagged = at; at = up(at + (size_t)n_faces * sizeof(int32_t));
  l.keep = at; at = up(at + (3 * (size_t)n + 1) * sizeof(uint32_t));
  l.at = at; at = up(at + (3 * (size_t)n + 1) * sizeof(uint32_t));
  l.scan_tmp = at; at = up(at + scan_tmp_bytes);
  l.bytes = at;
  return l;
}

int scan_tmp_bytes(int32_t n, hipStream_t st, size_t *bytes) {
  *bytes = 0;
  return check(rocprim::exclusive_scan(nullptr, *bytes, (uint32_t *)nullptr, (uint32_t *)nullptr, 0u, 3 * (size_t)n + 1, rocprim::plus<uint32_t>(), st));
}

bool sizes_ok(int32_t n, int32_t n_faces) { return n >= 0 && n_faces >= 0 && (int64_t)n * 3 + 1 <= INT32_MAX; }

__global__ __launch_bounds__(TPB) void k_stats_add(int n, const float *__restrict__ grad, const int32_t *__restrict__ radii,
                                                   const uint8_t *__restrict__ mask, float *__restrict__ accum, float *__restrict__ denom,
                                                   float *__restrict__ max_radii) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  densify::stats_add(i, grad, radii, mask, accum, denom, max_radii);
}

__global__ __launch_bounds__(TPB) void k_classify(int n, int n_faces, const float *__restrict__ scaling, const float *__restrict__ opacity,
                                                  const int32_t *__restrict__ binding, const float *__restrict__ face_scaling,
                                                  const float *__restrict__ accum, const float *__restrict__ denom, densify::Limits lim,
                                                  uint8_t *__restrict__ bits, int32_t *__restrict__ face_rows,
                                                  int32_t *__restrict__ face_flagged, int32_t *__restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const uint8_t b = densify::classify(i, n_faces, scaling, opacity, binding, face_scaling, accum, denom, lim);
  bits[i] = b;
  if (b & densify::BAD) {
    atomicOr(&counts[densify::ERROR], 1);
    return;
  }
  int32_t rows, flagged;
  densify::face_votes(b, &rows, &flagged);
  const int32_t f = binding[i];
  atomicAdd(&face_rows[f], rows);
  if (flagged) atomicAdd(&face_flagged[f], flagged);
  if (b & densify::CLONE) atomicAdd(&counts[densify::N_CLONED], 1);
  if (b & densify::SPLIT) atomicAdd(&counts[densify::N_SPLIT], 1);
}

// keep [3 n + 1]: column 0 the originals, 1 the clones, 2 the pairs of children; the last entry is 0 and receives the total
__global__ __launch_bounds__(TPB) void k_resolve(int n, const uint8_t *__restrict__ bits, const int32_t *__restrict__ binding,
                                                 const int32_t *__restrict__ face_rows, const int32_t *__restrict__ face_flagged,
                                                 uint32_t *__restrict__ keep) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i == 0) keep[3 * (int64_t)n] = 0u;
  if (i >= n) return;
  const uint8_t b = bits[i];
  uint8_t k = 0;
  if (!(b & densify::BAD)) {
    const int32_t f = binding[i];
    k = densify::keeps(b, face_rows[f], face_flagged[f]);
  }
  keep[i] = (k & densify::KEEP_SELF) ? 1u : 0u;
  keep[(int64_t)n + i] = (k & densify::KEEP_CLONE) ? 1u : 0u;
  keep[2 * (int64_t)n + i] = (k & densify::KEEP_CHILDREN) ? 1u : 0u;
}

// one thread: the places where the blocks of the output begin, and the counts.  counts[N_CLONED], [N_SPLIT], [ERROR] are k_classify's.
__global__ void k_counts(int n, const uint32_t *__restrict__ at, int32_t *__restrict__ counts) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const int32_t clones = (int32_t)at[n], first = (int32_t)at[2 * (int64_t)n], second = (int32_t)at[3 * (int64_t)n];
  const int32_t n_out = second + (second - first);
  counts[densify::AT_CLONES] = clones;
  counts[densify::AT_FIRST] = first;
  counts[densify::AT_SECOND] = second;
  counts[densify::N_OUT] = n_out;
  counts[densify::N_PRUNED] = n + counts[densify::N_CLONED] + counts[densify::N_SPLIT] - n_out;  // n - s + c + 2 s rows before the prune
}

__global__ __launch_bounds__(TPB) void k_emit(int n, int n_out, const int32_t *__restrict__ binding, const uint32_t *__restrict__ keep,
                                              const uint32_t *__restrict__ at, int32_t *__restrict__ src, int32_t *__restrict__ kind,
                                              int32_t *__restrict__ out_binding, int32_t *__restrict__ counter) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const int32_t f = binding[i];
  const int64_t pairs = (int64_t)at[3 * (int64_t)n] - (int64_t)at[2 * (int64_t)n];
  int32_t rows = 0;
  auto put = [&](int64_t row, int32_t k) {
    if (row >= n_out) return;  // a caller whose n_out is not the plan's writes nothing out of bounds
    src[row] = (int32_t)i;
    kind[row] = k;
    out_binding[row] = f;
    ++rows;
  };
  if (keep[i]) put(at[i], densify::KEPT);
  if (keep[(int64_t)n + i]) put(at[(int64_t)n + i], densify::CLONED);
  if (keep[2 * (int64_t)n + i]) {
    put(at[2 * (int64_t)n + i], densify::CHILD);
    put((int64_t)at[2 * (int64_t)n + i] + pairs, densify::CHILD);
  }
  if (rows) atomicAdd(&counter[f], rows);
}

struct Table {
  const float *in[MAX_T];
  float *out[MAX_T];
  int32_t width[MAX_T], mode[MAX_T];
};

// blockIdx.y names the tensor, a thread one element of its output; rows of `width` floats, so the stores are contiguous and the
// loads contiguous within a row
__global__ __launch_bounds__(TPB) void k_gather(int n, int n_out, Table t, const int32_t *__restrict__ src, const int32_t *__restrict__ kind,
                                                const uint32_t *__restrict__ at, const float *__restrict__ xyz,
                                                const float *__restrict__ scaling, const float *__restrict__ rotation,
                                                const int32_t *__restrict__ binding, const float *__restrict__ face_scaling,
                                                const float *__restrict__ noise) {
  const int32_t width = t.width[blockIdx.y], mode = t.mode[blockIdx.y];
  const int64_t e = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (e >= (int64_t)n_out * width) return;
  const int64_t row = e / width;
  const int32_t col = (int32_t)(e - row * width);
  const int64_t i = src[row];
  if (i < 0 || i >= n) return;
  const bool second = row >= (int64_t)at[3 * (int64_t)n];
  t.out[blockIdx.y][e] = densify::gathered(mode, width, i, col, kind[row], second, t.in[blockIdx.y], xyz, scaling, rotation, binding,
                                           face_scaling, noise);
}

__global__ __launch_bounds__(TPB) void k_reset_opacity(int64_t n, const float *__restrict__ opacity, float *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  out[i] = densify::reset_opacity(opacity[i]);
}

}  // namespace

extern "C" {

int mpmhip_densify_stats_add(int32_t device, void *stream, int32_t n, const float *viewspace_grad, const int32_t *radii,
                             const uint8_t *visible, float *xyz_gradient_accum, float *denom, float *max_radii2D) {
  if (n < 0 || (radii != nullptr) == (visible != nullptr)) return MPMHIP_ERR_INVALID;
  if (n > 0 && (!viewspace_grad || !xyz_gradient_accum || !denom || !max_radii2D)) return MPMHIP_ERR_INVALID;
  if (int rc = device_in_range(device)) return rc;
  if (n == 0) return MPMHIP_OK;
  ENTRY_CHECK(hipSetDevice(device));
  hipLaunchKernelGGL(k_stats_add, blocks(n, TPB), TPB, 0, (hipStream_t)stream, n, viewspace_grad, radii, visible, xyz_gradient_accum, denom,
                     max_radii2D);
  return check(hipGetLastError());
}

int mpmhip_densify_scratch_bytes(int32_t device, int32_t n, int32_t n_faces, int64_t *out_bytes) {
  if (!out_bytes || !sizes_ok(n, n_faces)) return MPMHIP_ERR_INVALID;
  if (int rc = select_device(device)) return rc;
  size_t tmp = 0;
  if (int rc = scan_tmp_bytes(n, nullptr, &tmp)) return rc;
  *out_bytes = (int64_t)layout(n, n_faces, tmp).bytes;
  return MPMHIP_OK;
}

int mpmhip_densify_plan(int32_t device, void *stream, int32_t n, int32_t n_faces, const float *scaling, const float *opacity,
                        const int32_t *binding, const float *face_scaling, const float *xyz_gradient_accum, const float *denom,
                        float max_grad, float dense_limit, float min_opacity, float world_limit, int32_t prune_big, void *scratch,
                        int64_t scratch_bytes, int32_t *out_counts) {
  if (!sizes_ok(n, n_faces) || !scratch || !out_counts) return MPMHIP_ERR_INVALID;
  if (n > 0 && (!scaling || !opacity || !binding || !face_scaling || !xyz_gradient_accum || !denom)) return MPMHIP_ERR_INVALID;
  if (int rc = select_device(device)) return rc;
  hipStream_t st = (hipStream_t)stream;
  size_t tmp = 0;
  if (int rc = scan_tmp_bytes(n, st, &tmp)) return rc;
  const Layout l = layout(n, n_faces, tmp);
  if (scratch_bytes < 0 || (size_t)scratch_bytes < l.bytes) return MPMHIP_ERR_INVALID;
  char *base = (char *)scratch;
  uint8_t *bits = (uint8_t *)(base + l.bits);
  int32_t *face_rows = (int32_t *)(base + l.face_rows), *face_flagged = (int32_t *)(base + l.face_flagged);
  uint32_t *keep = (uint32_t *)(base + l.keep), *at = (uint32_t *)(base + l.at);
  const densify::Limits lim{max_grad, dense_limit, min_opacity, world_limit, prune_big};
  ENTRY_CHECK(hipMemsetAsync(out_counts, 0, densify::N_COUNTS * sizeof(int32_t), st));
  // face_rows and face_flagged are neighbours in the layout: one memset over both
  if (n_faces > 0) ENTRY_CHECK(hipMemsetAsync(face_rows, 0, l.keep - l.face_rows, st));
  if (n > 0) {
    hipLaunchKernelGGL(k_classify, blocks(n, TPB), TPB, 0, st, n, n_faces, scaling, opacity, binding, face_scaling, xyz_gradient_accum, denom,
                       lim, bits, face_rows, face_flagged, out_counts);
    ENTRY_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_resolve, blocks(n > 0 ? n : 1, TPB), TPB, 0, st, n, (const uint8_t *)bits, binding, (const int32_t *)face_rows,
                     (const int32_t *)face_flagged, keep);
  ENTRY_CHECK(hipGetLastError());
  ENTRY_CHECK(rocprim::exclusive_scan(base + l.scan_tmp, tmp, keep, at, 0u, 3 * (size_t)n + 1, rocprim::plus<uint32_t>(), st));
  hipLaunchKernelGGL(k_counts, 1, 64, 0, st, n, (const uint32_t *)at, out_counts);
  return check(hipGetLastError());
}

int mpmhip_densify_emit(int32_t device, void *stream, int32_t n, int32_t n_faces, int32_t n_out, const float *xyz, const float *scaling,
                        const float *rotation, const int32_t *binding, const float *face_scaling, const float *noise, const void *scratch,
                        int64_t scratch_bytes, int32_t n_tensors, const float *const *in, float *const *out, const int32_t *widths,
                        const int32_t *modes, int32_t *out_src, int32_t *out_kind, int32_t *out_binding, int32_t *out_binding_counter) {
  if (!sizes_ok(n, n_faces) || n_out < 0 || n_tensors < 0 || n_tensors > MAX_T || !scratch) return MPMHIP_ERR_INVALID;
  if (n_tensors > 0 && (!in || !out || !widths || !modes)) return MPMHIP_ERR_INVALID;
  if (n > 0 && (!xyz || !scaling || !rotation || !binding || !face_scaling || !noise)) return MPMHIP_ERR_INVALID;
  if (n_out > 0 && (!out_src || !out_kind || !out_binding)) return MPMHIP_ERR_INVALID;
  if (n_faces > 0 && !out_binding_counter) return MPMHIP_ERR_INVALID;
  Table t;
  int64_t widest = 0;
  for (int k = 0; k < n_tensors; ++k) {
    if (widths[k] <= 0 || modes[k] < densify::MODE_COPY || modes[k] > densify::MODE_SCALING || !out[k] || (n > 0 && !in[k]))
      return MPMHIP_ERR_INVALID;
    if ((modes[k] == densify::MODE_XYZ || modes[k] == densify::MODE_SCALING) && widths[k] != 3) return MPMHIP_ERR_INVALID;
    t.in[k] = in[k]; t.out[k] = out[k]; t.width[k] = widths[k]; t.mode[k] = modes[k];
    widest = widths[k] > widest ? widths[k] : widest;
  }
  for (int k = n_tensors; k < MAX_T; ++k) { t.in[k] = nullptr; t.out[k] = nullptr; t.width[k] = 0; t.mode[k] = 0; }
  if (int rc = select_device(device)) return rc;
  hipStream_t st = (hipStream_t)stream;
  size_t tmp = 0;
  if (int rc = scan_tmp_bytes(n, st, &tmp)) return rc;
  const Layout l = layout(n, n_faces, tmp);
  if (scratch_bytes < 0 || (size_t)scratch_bytes < l.bytes) return MPMHIP_ERR_INVALID;
  const char *base = (const char *)scratch;
  const uint32_t *keep = (const uint32_t *)(base + l.keep), *at = (const uint32_t *)(base + l.at);
  if (n_faces > 0) ENTRY_CHECK(hipMemsetAsync(out_binding_counter, 0, (size_t)n_faces * sizeof(int32_t), st));
  if (n == 0 || n_out == 0) return MPMHIP_OK;
  hipLaunchKernelGGL(k_emit, blocks(n, TPB), TPB, 0, st, n, n_out, binding, keep, at, out_src, out_kind, out_binding, out_binding_counter);
  ENTRY_CHECK(hipGetLastError());
  if (n_tensors > 0) {
    hipLaunchKernelGGL(k_gather, dim3(blocks((int64_t)n_out * widest, TPB), (unsigned)n_tensors), TPB, 0, st, n, n_out, t,
                       (const int32_t *)out_src, (const int32_t *)out_kind, at, xyz, scaling, rotation, binding, face_scaling, noise);
    ENTRY_CHECK(hipGetLastError());
  }
  return MPMHIP_OK;
}

int mpmhip_reset_opacity(int32_t device, void *stream, int64_t n, const float *opacity, float *out) {
  if (n < 0 || (n > 0 && (!opacity || !out))) return MPMHIP_ERR_INVALID;
  if (int rc = device_in_range(device)) return rc;
  if (n == 0) return MPMHIP_OK;
  ENTRY_CHECK(hipSetDevice(device));
  hipLaunchKernelGGL(k_reset_opacity, blocks(n, TPB), TPB, 0, (hipStream_t)stream, n, opacity, out);
  return check(hipGetLastError());
}

}  // extern "C"
