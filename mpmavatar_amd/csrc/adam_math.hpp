// adam_math.hpp -- the optimiser step of the appearance loop (train_appearance.py:260, torch.optim.Adam as scene/gaussian_model.py:222
// constructs it: no amsgrad, no weight decay), per element, and which workgroup of the launch works on which elements.
//   m' = m + w1 (g - m)                  w1 = fp32(1 - beta1)
//   v' = v beta2 + w2 g g                w2 = fp32(1 - beta2)
//   d  = sqrt(v') / bc2_sqrt + eps       bc2_sqrt = fp32(sqrt(1 - beta2^step))
//   p' = p - step_size (m' / d)          step_size = fp32(lr / (1 - beta1^step))
// The operations and their order are those of torch's single-tensor Adam (exp_avg.lerp_, exp_avg_sq.mul_().addcmul_(), the
// denominator, then the step).  All scalars are computed by the caller in double and rounded to fp32 once.  fp32 throughout, with
// contraction off in every function of this header (the pragma reaches the enclosing compound statement and nothing it calls, so
// each function carries its own); division and square root are the correctly rounded ones.
// The launch: the tensors of a step sit in a table that travels by value as the kernel argument.  A tensor is cut into chunks of
// CHUNK elements, the chunks of all tensors are numbered in table order, and a workgroup takes chunks blockIdx.x, blockIdx.x +
// gridDim.x, ...  Within a chunk, thread t makes ACCESSES 16-byte accesses u = 0 .. ACCESSES - 1 at elements vec_elem(chunk, u, t)
// (a run of 256 threads reads 4 KB contiguously); a tensor whose pointers are not all 16-byte aligned is walked element by element
// at scalar_elem(chunk, j, t), j = 0 .. VEC * ACCESSES - 1.  The up to three elements behind the last whole group of four are
// taken one by one by the thread whose access they begin.
// Plain C++ for the device (adam.hip) and the host (tests/hostadam/) alike: the host lays the launch out with it, the kernel
// decodes with it, the host test walks it.
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

namespace adam {

constexpr int TPB = 256;
constexpr int VEC = 4;  // floats of a 16-byte access
#ifndef MPMHIP_ADAM_ACCESSES
#define MPMHIP_ADAM_ACCESSES 4  // (experiment switch: 16-byte loads in flight per thread and stream; tools/optim_bench.py --variant)
#endif
constexpr int ACCESSES = MPMHIP_ADAM_ACCESSES;
constexpr int CHUNK = TPB * VEC * ACCESSES;
#ifndef MPMHIP_ADAM_GRID_CAP
#define MPMHIP_ADAM_GRID_CAP 2048  // (experiment switch: workgroups of a launch, the rest by stride; 0 = one workgroup per chunk)
#endif
constexpr int GRID_CAP = MPMHIP_ADAM_GRID_CAP;
// The argument block of a kernel is limited to 4 KB: 48 tensors of 64 B, 49 chunk offsets and two counts are 3,276 B, which leaves
// room for the arguments the runtime appends.
constexpr int MAX_TENSORS = 48;
// elements of one tensor: MAX_TENSORS of them still number their chunks in an int32
constexpr int64_t MAX_COUNT = (int64_t)(INT32_MAX / MAX_TENSORS) * CHUNK;

struct Scalars {
  float step_size, bc2_sqrt, w1, beta2, w2, eps;
};

// p == nullptr: the group's learning rate is zero; the parameter is neither read nor written and the moments still move
struct Tensor {
  float *p;
  const float *g;
  float *m, *v;
  int64_t count;
  Scalars s;
};

// first_chunk [n_tensors + 1]: the running chunk offset, strictly ascending (a tensor without elements is not in the table)
struct Table {
  Tensor t[MAX_TENSORS];
  int32_t first_chunk[MAX_TENSORS + 1];
  int32_t n_tensors, n_chunks;
};
static_assert(sizeof(Tensor) == 64 && sizeof(Table) <= 4096 - 512, "the table is a kernel argument");

__host__ __device__ __forceinline__ void moments(float g, float &m, float &v, const Scalars &s) {
#pragma clang fp contract(off)
  m = m + s.w1 * (g - m);
  v = v * s.beta2 + s.w2 * g * g;
}

__host__ __device__ __forceinline__ float step(float p, float m, float v, const Scalars &s) {
#pragma clang fp contract(off)
  const float d = sqrtf(v) / s.bc2_sqrt + s.eps;
  return p - s.step_size * (m / d);
}

__host__ __device__ __forceinline__ int64_t n_chunks(int64_t count) { return (count + CHUNK - 1) / CHUNK; }

// appends a tensor (count > 0) to a table that has room
__host__ __device__ inline void push(Table &T, const Tensor &x) {
  T.t[T.n_tensors] = x;
  T.first_chunk[T.n_tensors] = T.n_chunks;
  T.n_chunks += (int32_t)n_chunks(x.count);
  T.first_chunk[++T.n_tensors] = T.n_chunks;
}

__host__ __device__ __forceinline__ unsigned grid(int32_t chunks) {
  return (unsigned)(GRID_CAP > 0 && chunks > GRID_CAP ? GRID_CAP : chunks);
}

// the tensor of chunk c < first_chunk[n]: the last i with first_chunk[i] <= c.  The same for every lane of a workgroup.
__host__ __device__ __forceinline__ int find_tensor(const int32_t *first_chunk, int n, int32_t c) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (first_chunk[mid] <= c) lo = mid; else hi = mid;
  }
  return lo;
}

__host__ __device__ __forceinline__ bool aligned16(const Tensor &x) {
  return ((((uintptr_t)x.p) | ((uintptr_t)x.g) | ((uintptr_t)x.m) | ((uintptr_t)x.v)) & 15) == 0;
}

// chunk: the index within the tensor
__host__ __device__ __forceinline__ int64_t vec_elem(int64_t chunk, int u, int t) { return chunk * CHUNK + ((int64_t)u * TPB + t) * VEC; }
__host__ __device__ __forceinline__ int64_t scalar_elem(int64_t chunk, int j, int t) { return chunk * CHUNK + (int64_t)j * TPB + t; }

}  // namespace adam
