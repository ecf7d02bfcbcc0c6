// adam.hip -- mpmhip_adam_step: the optimiser step of the appearance loop (train_appearance.py:260) for any number of tensors in
// one launch per adam::MAX_TENSORS of them.  The math and the layout of the launch are adam_math.hpp; k_adam is a workgroup of 256
// threads per chunk of one tensor, found from the table that is the kernel's argument: no device-side table, no copy, no
// allocation and no synchronisation, so a gradient that is a new tensor every iteration costs nothing.
// Pure streaming: per element 12 B of g, m, v in and 8 B of m, v out, and 4 B of p each way where the learning rate is not zero.
// A thread issues all loads of its chunk -- ACCESSES of 16 bytes per stream -- before the first use, computes, and stores 16 bytes
// at a time.  No LDS, no atomics, every element is owned by one thread: the same input gives the same bits.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "adam_math.hpp"
#include "entry.hpp"

namespace {

using namespace entry;
using adam::ACCESSES;
using adam::TPB;
using adam::VEC;
static_assert(adam::CHUNK == MPMHIP_ADAM_CHUNK || MPMHIP_ADAM_ACCESSES != 4, "mpmhip.h states the chunk of the default build");
static_assert(adam::MAX_TENSORS == MPMHIP_ADAM_MAX_TENSORS, "mpmhip.h states the tensors of a launch");

__device__ __forceinline__ float4 ld4(const float *a) { return *reinterpret_cast<const float4 *>(a); }
__device__ __forceinline__ void st4(float *a, float4 x) { *reinterpret_cast<float4 *>(a) = x; }

template <bool UPDATE>
__device__ __forceinline__ void one(const adam::Tensor &x, int64_t e) {
  float m = x.m[e], v = x.v[e];
  adam::moments(x.g[e], m, v, x.s);
  x.m[e] = m;
  x.v[e] = v;
  if (UPDATE) x.p[e] = adam::step(x.p[e], m, v, x.s);
}

template <bool UPDATE>
__device__ __forceinline__ void four(float4 &p, const float4 &g, float4 &m, float4 &v, const adam::Scalars &s) {
  adam::moments(g.x, m.x, v.x, s);
  adam::moments(g.y, m.y, v.y, s);
  adam::moments(g.z, m.z, v.z, s);
  adam::moments(g.w, m.w, v.w, s);
  if (UPDATE) {
    p.x = adam::step(p.x, m.x, v.x, s);
    p.y = adam::step(p.y, m.y, v.y, s);
    p.z = adam::step(p.z, m.z, v.z, s);
    p.w = adam::step(p.w, m.w, v.w, s);
  }
}

// 16-byte accesses.  WHOLE: every access of the chunk lies inside the tensor, and nothing is tested per access.
template <bool UPDATE, bool WHOLE>
__device__ __forceinline__ void chunk_vec(const adam::Tensor &x, int64_t chunk, int t) {
  float4 p[ACCESSES], g[ACCESSES], m[ACCESSES], v[ACCESSES];
  int64_t e[ACCESSES];
#pragma unroll
  for (int u = 0; u < ACCESSES; ++u) {
    e[u] = adam::vec_elem(chunk, u, t);
    if (WHOLE || e[u] + VEC <= x.count) {
      g[u] = ld4(x.g + e[u]);
      m[u] = ld4(x.m + e[u]);
      v[u] = ld4(x.v + e[u]);
      if (UPDATE) p[u] = ld4(x.p + e[u]);
    }
  }
#pragma unroll
  for (int u = 0; u < ACCESSES; ++u) {
    if (WHOLE || e[u] + VEC <= x.count) {
      four<UPDATE>(p[u], g[u], m[u], v[u], x.s);
      st4(x.m + e[u], m[u]);
      st4(x.v + e[u], v[u]);
      if (UPDATE) st4(x.p + e[u], p[u]);
    } else {
      for (int64_t i = e[u]; i < x.count; ++i) one<UPDATE>(x, i);  // the tail: at most three elements, in one thread of the tensor
    }
  }
}

// 4-byte accesses, for a tensor with a pointer that is not 16-byte aligned (a view into a larger buffer)
template <bool UPDATE>
__device__ __forceinline__ void chunk_scalar(const adam::Tensor &x, int64_t chunk, int t) {
  constexpr int N = VEC * ACCESSES;
  float p[N], g[N], m[N], v[N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const int64_t e = adam::scalar_elem(chunk, j, t);
    if (e < x.count) {
      g[j] = x.g[e];
      m[j] = x.m[e];
      v[j] = x.v[e];
      if (UPDATE) p[j] = x.p[e];
    }
  }
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const int64_t e = adam::scalar_elem(chunk, j, t);
    if (e < x.count) {
      adam::moments(g[j], m[j], v[j], x.s);
      x.m[e] = m[j];
      x.v[e] = v[j];
      if (UPDATE) x.p[e] = adam::step(p[j], m[j], v[j], x.s);
    }
  }
}

template <bool UPDATE>
__device__ __forceinline__ void chunk_any(const adam::Tensor &x, int64_t chunk, int t) {
  if (!adam::aligned16(x)) chunk_scalar<UPDATE>(x, chunk, t);
  else if ((chunk + 1) * adam::CHUNK <= x.count) chunk_vec<UPDATE, true>(x, chunk, t);
  else chunk_vec<UPDATE, false>(x, chunk, t);
}

// every branch but the per-access tests of a tensor's last chunk is the same for the whole workgroup
__global__ __launch_bounds__(TPB) void k_adam(const adam::Table T) {
  for (int64_t c = blockIdx.x; c < T.n_chunks; c += gridDim.x) {
    const int i = adam::find_tensor(T.first_chunk, T.n_tensors, (int32_t)c);
    const adam::Tensor x = T.t[i];
    const int64_t chunk = c - T.first_chunk[i];
    if (x.p) chunk_any<true>(x, chunk, threadIdx.x); else chunk_any<false>(x, chunk, threadIdx.x);
  }
}

int launch(const adam::Table &T, hipStream_t s) {
  hipLaunchKernelGGL(k_adam, adam::grid(T.n_chunks), TPB, 0, s, T);
  return check(hipGetLastError());
}

}  // namespace

extern "C" int mpmhip_adam_step(int32_t device, void *stream, int32_t n_tensors, void *const *params, const void *const *grads,
                                void *const *exp_avg, void *const *exp_avg_sq, const int64_t *counts, const float *step_size,
                                const float *bc2_sqrt, const float *w1, const float *beta2, const float *w2, const float *eps,
                                const uint8_t *update_param) {
  if (n_tensors < 0) return MPMHIP_ERR_INVALID;
  if (n_tensors > 0 && (!params || !grads || !exp_avg || !exp_avg_sq || !counts || !step_size || !bc2_sqrt || !w1 || !beta2 || !w2 || !eps ||
                        !update_param))
    return MPMHIP_ERR_INVALID;
  bool any = false;
  for (int32_t i = 0; i < n_tensors; ++i) {
    if (counts[i] < 0 || counts[i] > adam::MAX_COUNT) return MPMHIP_ERR_INVALID;
    if (counts[i] > 0 && (!params[i] || !grads[i] || !exp_avg[i] || !exp_avg_sq[i])) return MPMHIP_ERR_INVALID;
    any = any || counts[i] > 0;
  }
  if (int rc = device_in_range(device)) return rc;
  if (!any) return MPMHIP_OK;
  ENTRY_CHECK(hipSetDevice(device));
  adam::Table T = {};
  for (int32_t i = 0; i < n_tensors; ++i) {
    if (counts[i] == 0) continue;
    adam::Tensor x;
    x.p = update_param[i] ? (float *)params[i] : nullptr;
    x.g = (const float *)grads[i];
    x.m = (float *)exp_avg[i];
    x.v = (float *)exp_avg_sq[i];
    x.count = counts[i];
    x.s = adam::Scalars{step_size[i], bc2_sqrt[i], w1[i], beta2[i], w2[i], eps[i]};
    adam::push(T, x);
    if (T.n_tensors == adam::MAX_TENSORS) {
      if (int rc = launch(T, (hipStream_t)stream)) return rc;
      T.n_tensors = T.n_chunks = 0;
    }
  }
  return T.n_tensors ? launch(T, (hipStream_t)stream) : MPMHIP_OK;
}
