// The optimiser step (mpmavatar_amd/csrc/adam_math.hpp) compiled for the host (tests/test_optim_host.py; the stand-in for
// <hip/hip_runtime.h> is tests/hostmath/stub): mpmhip_adam_step and k_adam of adam.hip restated as serial loops -- the same tables
// of at most MAX_TENSORS tensors, the same grid, the same stride over chunks, the same search for a chunk's tensor, and per
// "thread" the same accesses: groups of four where every pointer of the tensor is 16-byte aligned, the tail behind the last whole
// group in the thread whose access it begins, single elements for a misaligned tensor.  visits (optional, per tensor, as long as
// the tensor) counts how often an element is taken.
#include "adam_math.hpp"

#include <cstdint>

namespace {

void one(const adam::Tensor &x, int64_t e, int32_t *visits) {
  float m = x.m[e], v = x.v[e];
  adam::moments(x.g[e], m, v, x.s);
  x.m[e] = m;
  x.v[e] = v;
  if (x.p) x.p[e] = adam::step(x.p[e], m, v, x.s);
  if (visits) ++visits[e];
}

void launch(const adam::Table &T, int32_t *const *visits) {
  const int64_t grid = adam::grid(T.n_chunks);
  for (int64_t b = 0; b < grid; ++b)
    for (int64_t c = b; c < T.n_chunks; c += grid) {
      const int i = adam::find_tensor(T.first_chunk, T.n_tensors, (int32_t)c);
      const adam::Tensor &x = T.t[i];
      const int64_t chunk = c - T.first_chunk[i];
      int32_t *vis = visits ? visits[i] : nullptr;
      for (int t = 0; t < adam::TPB; ++t) {
        if (!adam::aligned16(x)) {
          for (int j = 0; j < adam::VEC * adam::ACCESSES; ++j) {
            const int64_t e = adam::scalar_elem(chunk, j, t);
            if (e < x.count) one(x, e, vis);
          }
          continue;
        }
        for (int u = 0; u < adam::ACCESSES; ++u) {
          const int64_t e = adam::vec_elem(chunk, u, t);
          const int64_t end = e + adam::VEC <= x.count ? e + adam::VEC : x.count;
          for (int64_t k = e; k < end; ++k) one(x, k, vis);
        }
      }
    }
}

}  // namespace

// the arguments of mpmhip_adam_step behind (device, stream), and visits; the argument checks are the entry point's own.
// -> the number of "launches"
extern "C" int ha_adam_step(int32_t n_tensors, void *const *params, const void *const *grads, void *const *exp_avg, void *const *exp_avg_sq,
                            const int64_t *counts, const float *step_size, const float *bc2_sqrt, const float *w1, const float *beta2,
                            const float *w2, const float *eps, const uint8_t *update_param, int32_t *const *visits) {
  adam::Table T = {};
  int32_t *vis[adam::MAX_TENSORS] = {};
  int launches = 0;
  for (int32_t i = 0; i < n_tensors; ++i) {
    if (counts[i] == 0) continue;
    adam::Tensor x;
    x.p = update_param[i] ? (float *)params[i] : nullptr;
    x.g = (const float *)grads[i];
    x.m = (float *)exp_avg[i];
    x.v = (float *)exp_avg_sq[i];
    x.count = counts[i];
    x.s = adam::Scalars{step_size[i], bc2_sqrt[i], w1[i], beta2[i], w2[i], eps[i]};
    vis[T.n_tensors] = visits ? visits[i] : nullptr;
    adam::push(T, x);
    if (T.n_tensors == adam::MAX_TENSORS) {
      launch(T, visits ? vis : nullptr);
      ++launches;
      T.n_tensors = T.n_chunks = 0;
    }
  }
  if (T.n_tensors) {
    launch(T, visits ? vis : nullptr);
    ++launches;
  }
  return launches;
}

extern "C" int ha_chunk() { return adam::CHUNK; }
extern "C" int ha_max_tensors() { return adam::MAX_TENSORS; }
extern "C" int ha_grid_cap() { return adam::GRID_CAP; }
extern "C" int64_t ha_table_bytes() { return (int64_t)sizeof(adam::Table); }
