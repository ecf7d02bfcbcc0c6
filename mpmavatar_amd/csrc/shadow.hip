// shadow.hip -- the shadow network of the appearance loop on the device (scene/shadow.py:14-181 over scene/network.py; the call is
// train_appearance.py:120 and :201): mpmhip_shadow_workspace_bytes, mpmhip_shadow_forward, mpmhip_shadow_backward.  The math, the
// tables and the layouts are shadow_math.hpp; this file is the kernels over it and the launches.
//
// Four channels (eight at most), nine 3 x 3 convolutions over maps of at most 1 MB: plain fp32 VALU work on a working set that lives
// in L2.  What counts is the number of launches and one pass over each activation:
//   forward   k_shadow_wn (all nine weight tensors, one workgroup each) + nine k_shadow_layer + k_shadow_resize unless U == S  = 10 / 11
//   backward  k_shadow_head_dz + nine k_shadow_layer_backward + k_shadow_reduce + k_shadow_wn_backward                          = 12
// k_shadow_layer: one 32 x 8 output tile per workgroup of 256 lanes (a wave reads two whole LDS rows of 32, so no two lanes of a
// half-wave meet on a bank), the input tile with its halo in LDS, filled THROUGH the layer's input transform (nearest resize minus
// ao_mean; bilinear down; bilinear up beside the skip), so that no resampled or concatenated tensor exists; the weights are read with
// wave-uniform addresses; the epilogue adds the untied bias and applies LeakyReLU (the head: bias, beta, sigmoid, and the copy to
// shadow_map where U == S).
// k_shadow_layer_backward: one tile per workgroup, the batch walked inside it.  The tile of dPre = dY lrelu'(Y) is filled by GATHERING
// dY from the input gradients of the layers that read this one (through the inverse tables where they read it resampled); its
// centre, summed over the batch, IS the untied-bias gradient and is written as such; dX comes from the flipped, transposed weights;
// the tile's share of dW goes to a per-tile slot, one lane per weight entry walking the tile in row-major order.  k_shadow_reduce adds
// the slots, one wave per entry, in a fixed tree.  No floating-point atomics: the same input gives the same bits.
// Accesses are 4-byte and coalesced (a tile row of 32 floats is 128 B); a tile row with its halo starts one float in front of a
// 16-byte boundary, so wider loads would need a shuffle the launch-bound kernels do not repay.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "entry.hpp"
#include "shadow_math.hpp"

namespace {

using namespace entry;
using namespace shadow;

struct WnArgs {
  const float *v[LAYERS], *g[LAYERS];
  float *w[LAYERS], *norm;
  int32_t count[LAYERS], per_o[LAYERS];
};

__global__ void __launch_bounds__(TPB) k_shadow_wn(WnArgs a) {
  __shared__ float part[TPB];
  const int L = blockIdx.x, t = threadIdx.x, count = a.count[L], per_o = a.per_o[L];
  const float *v = a.v[L], *g = a.g[L];
  part[t] = wn_partial(v, count, t);
  __syncthreads();
  for (int s = TPB / 2; s > 0; s >>= 1) {
    if (t < s) part[t] += part[t + s];
    __syncthreads();
  }
  const float norm = sqrtf(part[0]);
  if (t == 0) a.norm[L] = norm;
  for (int i = t; i < count; i += TPB) a.w[L][i] = wn_weight(v[i], g[i / per_o], norm);
}

struct LayerFwd {
  LayerIn in;
  const float *w, *bias;
  int32_t bias_tied;
  float slope, beta;
  float *out, *out2, *ao_out;
};

template <int CA, int CB, int COUT, bool IS_HEAD>
__global__ void __launch_bounds__(TPB) k_shadow_layer(LayerFwd a) {
  constexpr int CIN = CA + CB;
  __shared__ float tile[CIN * PLANE];
  const int n = blockIdx.z, ty0 = blockIdx.y * TILE_H, tx0 = blockIdx.x * TILE_W, t = threadIdx.x, s = a.in.size;
  for (int idx = t; idx < CIN * PLANE; idx += TPB) tile[idx] = input_tile_at(a.in, n, idx, ty0, tx0);
  __syncthreads();
  const int ly = t / TILE_W, lx = t % TILE_W, y = ty0 + ly, x = tx0 + lx;
  if (y >= s || x >= s) return;
  float acc[COUT];
  conv_at<CIN, COUT>(tile, a.w, ly, lx, acc);
  if (IS_HEAD) {
    const float z = acc[0] + (a.bias_tied ? a.bias[0] : a.bias[y * s + x]);
    const float v = sigmoid(z + a.beta);
    const int64_t at = ((int64_t)n * s + y) * s + x;
    a.out[at] = v;
    if (a.out2) a.out2[at] = v;
  } else {
#pragma unroll
    for (int o = 0; o < COUT; ++o)
      a.out[(((int64_t)n * COUT + o) * s + y) * s + x] = lrelu(acc[o] + a.bias[(o * s + y) * s + x], a.slope);
    if (a.ao_out) a.ao_out[((int64_t)n * s + y) * s + x] = a.in.ao[((int64_t)n * a.in.in_h + a.in.ny[y]) * a.in.in_w + a.in.nx[x]];
  }
}

__global__ void __launch_bounds__(TPB) k_shadow_resize(Resample fin, int n_total, const float *low, float *map) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x, per = (int64_t)fin.out * fin.out;
  if (i >= n_total * per) return;
  const int n = (int)(i / per), r = (int)(i % per);
  map[i] = final_at(fin, low, n, r / fin.out, r % fin.out);
}

__global__ void __launch_bounds__(TPB) k_shadow_head_dz(Resample fin, int identity, int n_total, const float *g_map, const float *g_low,
                                                        const float *low, float *dz) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x, per = (int64_t)fin.in * fin.in;
  if (i >= n_total * per) return;
  const int n = (int)(i / per), r = (int)(i % per);
  dz[i] = head_dz_at(fin, identity, g_map, g_low, low, n, r / fin.in, r % fin.in);
}

struct LayerBwd {
  LayerIn in;
  LayerGrad gr;
  const float *w;
  int32_t n, want_dw, bias_tied, tiles;
  float *dx, *d_bias, *part, *part_bias;
};

template <int CA, int CB, int COUT>
__global__ void __launch_bounds__(TPB) k_shadow_layer_backward(LayerBwd a) {
  constexpr int CIN = CA + CB, NW = COUT * CIN * 9, ROUNDS = (NW + TPB - 1) / TPB;
  __shared__ float xin[CIN * PLANE];
  __shared__ float dpre[COUT * PLANE];
  const int ty0 = blockIdx.y * TILE_H, tx0 = blockIdx.x * TILE_W, t = threadIdx.x, s = a.in.size;
  const int tile = blockIdx.y * gridDim.x + blockIdx.x;
  const int ly = t / TILE_W, lx = t % TILE_W, y = ty0 + ly, x = tx0 + lx;
  const bool inside = y < s && x < s;
  float db[COUT], dw[ROUNDS], tile_bias = 0.f;
  for (int o = 0; o < COUT; ++o) db[o] = 0.f;
  for (int r = 0; r < ROUNDS; ++r) dw[r] = 0.f;
  for (int n = 0; n < a.n; ++n) {
    if (a.want_dw)
      for (int idx = t; idx < CIN * PLANE; idx += TPB) xin[idx] = input_tile_at(a.in, n, idx, ty0, tx0);
    for (int idx = t; idx < COUT * PLANE; idx += TPB) dpre[idx] = dpre_tile_at(a.gr, s, COUT, n, idx, ty0, tx0);
    __syncthreads();
    if (inside) {
#pragma unroll
      for (int o = 0; o < COUT; ++o) db[o] += dpre[o * PLANE + (ly + 1) * HALO_W + lx + 1];
      if (a.dx) {
        float dx[CIN];
        conv_transpose_at<CIN, COUT>(dpre, a.w, ly, lx, dx);
#pragma unroll
        for (int c = 0; c < CIN; ++c) a.dx[(((int64_t)n * CIN + c) * s + y) * s + x] = dx[c];
      }
    }
    if (a.want_dw) {
#pragma unroll
      for (int r = 0; r < ROUNDS; ++r) {
        const int e = t + r * TPB;
        if (e < NW) dw[r] += dw_tile_sum<CIN>(xin, dpre, e);
      }
    }
    if (a.part_bias && t == TPB - 1) tile_bias += tile_sum(dpre);
    __syncthreads();
  }
  if (inside && a.d_bias && !a.bias_tied) {
#pragma unroll
    for (int o = 0; o < COUT; ++o) a.d_bias[(o * s + y) * s + x] = db[o];
  }
  if (a.want_dw) {
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
      const int e = t + r * TPB;
      if (e < NW) a.part[(int64_t)e * a.tiles + tile] = dw[r];
    }
  }
  if (a.part_bias && t == TPB - 1) a.part_bias[tile] = tile_bias;
}

constexpr int SLOTS = LAYERS + 1;  // the nine dW and the tied head bias

struct ReduceArgs {
  const float *part[SLOTS];
  float *out[SLOTS];
  int32_t tiles[SLOTS], first[SLOTS + 1];  // the waves first[k] .. first[k + 1] - 1 take the entries of slot k
};

// one wave per entry: lane l adds the slots of tiles l, l + 64, .. in ascending order, then a fixed tree over the 64 lanes
__global__ void __launch_bounds__(TPB) k_shadow_reduce(ReduceArgs a) {
  const int wave = (blockIdx.x * TPB + threadIdx.x) / 64, lane = threadIdx.x & 63;
  if (wave >= a.first[SLOTS]) return;  // the same for every lane of a wave
  int k = 0;
  while (wave >= a.first[k + 1]) ++k;
  const int e = wave - a.first[k], tiles = a.tiles[k];
  const float *p = a.part[k] + (int64_t)e * tiles;
  float acc = 0.f;
  for (int i = lane; i < tiles; i += 64) acc += p[i];
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if (lane == 0) a.out[k][e] = acc;
}

struct WnBack {
  const float *v[LAYERS], *g[LAYERS], *dw[LAYERS], *norm;
  float *dv[LAYERS], *dg[LAYERS];
  int32_t count[LAYERS], per_o[LAYERS];
};

__global__ void __launch_bounds__(TPB) k_shadow_wn_backward(WnBack a) {
  __shared__ float dot[MAX_C];
  __shared__ float total;
  const int L = blockIdx.x, t = threadIdx.x, count = a.count[L], per_o = a.per_o[L], cout = count / per_o;
  if (!a.dv[L] && !a.dg[L]) return;
  const float *v = a.v[L], *g = a.g[L], *dw = a.dw[L];
  const float norm = a.norm[L];
  if (t < cout) dot[t] = wn_dot(dw, v, t, per_o);
  __syncthreads();
  if (t == 0) {
    float acc = 0.f;
    for (int o = 0; o < cout; ++o) acc += g[o] * dot[o];
    total = acc;
  }
  __syncthreads();
  if (a.dg[L] && t < cout) a.dg[L][t] = wn_dg(dot[t], norm);
  if (a.dv[L])
    for (int i = t; i < count; i += TPB) a.dv[L][i] = wn_dv(dw[i], v[i], g[i / per_o], norm, total);
}

// ---- the host side -----------------------------------------------------------------------------------------------------------------------

constexpr int MAX_SIZE = 8192, MAX_BATCH = 65535;  // 2 * MAX_C * MAX_SIZE^2 < 2^31; the batch is a grid dimension

int check_sizes(const mpmhip_shadow_desc *d) {
  if (!d) return MPMHIP_ERR_INVALID;
  if (d->n < 0 || d->n > MAX_BATCH || d->in_h < 1 || d->in_w < 1 || d->in_h > MAX_SIZE || d->in_w > MAX_SIZE) return MPMHIP_ERR_INVALID;
  if (d->shadow_size < 8 || d->shadow_size > MAX_SIZE || d->uv_size < 1 || d->uv_size > MAX_SIZE) return MPMHIP_ERR_INVALID;
  if (d->n_dims != 4 && d->n_dims != 8) return MPMHIP_ERR_INVALID;
  if (d->untied_head_bias != 0 && d->untied_head_bias != 1) return MPMHIP_ERR_INVALID;
  return MPMHIP_OK;
}

int check_desc(const mpmhip_shadow_desc *d, const void *workspace, int64_t workspace_bytes) {
  if (int rc = check_sizes(d)) return rc;
  if (!(d->lrelu_slope >= 0.f) || !std::isfinite(d->lrelu_slope) || !std::isfinite(d->beta)) return MPMHIP_ERR_INVALID;
  if (!d->ao_mean || !d->tables || !workspace) return MPMHIP_ERR_INVALID;
  for (int L = 0; L < LAYERS; ++L)
    if (!d->weight_v[L] || !d->weight_g[L] || !d->bias[L]) return MPMHIP_ERR_INVALID;
  if (workspace_bytes < 4 * workspace_layout(d->n, d->shadow_size, d->n_dims).words) return MPMHIP_ERR_INVALID;
  return MPMHIP_OK;
}

template <int C>
void launch_layer(int L, dim3 grid, hipStream_t st, const LayerFwd &a) {
  if (L == 0) hipLaunchKernelGGL((k_shadow_layer<1, 0, C, false>), grid, TPB, 0, st, a);
  else if (L == HEAD) hipLaunchKernelGGL((k_shadow_layer<C, 0, 1, true>), grid, TPB, 0, st, a);
  else if (L >= 5) hipLaunchKernelGGL((k_shadow_layer<C, C, C, false>), grid, TPB, 0, st, a);
  else hipLaunchKernelGGL((k_shadow_layer<C, 0, C, false>), grid, TPB, 0, st, a);
}

template <int C>
void launch_layer_backward(int L, dim3 grid, hipStream_t st, const LayerBwd &a) {
  if (L == 0) hipLaunchKernelGGL((k_shadow_layer_backward<1, 0, C>), grid, TPB, 0, st, a);
  else if (L == HEAD) hipLaunchKernelGGL((k_shadow_layer_backward<C, 0, 1>), grid, TPB, 0, st, a);
  else if (L >= 5) hipLaunchKernelGGL((k_shadow_layer_backward<C, C, C>), grid, TPB, 0, st, a);
  else hipLaunchKernelGGL((k_shadow_layer_backward<C, 0, C>), grid, TPB, 0, st, a);
}

}  // namespace

extern "C" {

int mpmhip_shadow_workspace_bytes(int32_t device, void *stream, const mpmhip_shadow_desc *desc, int64_t *out_workspace_bytes,
                                  int64_t *out_table_bytes, void *host_tables) {
  (void)stream;
  if (int rc = check_sizes(desc)) return rc;
  if (!out_workspace_bytes || !out_table_bytes) return MPMHIP_ERR_INVALID;
  // host arithmetic: written whenever the arguments are valid, whatever the device
  *out_workspace_bytes = 4 * workspace_layout(desc->n, desc->shadow_size, desc->n_dims).words;
  *out_table_bytes = 4 * table_words(desc->shadow_size, desc->uv_size);
  if (host_tables) fill_tables((int32_t *)host_tables, desc->in_h, desc->in_w, desc->shadow_size, desc->uv_size);
  return device_in_range(device);
}

int mpmhip_shadow_forward(int32_t device, void *stream, const mpmhip_shadow_desc *desc, const float *ao_map, void *workspace,
                          int64_t workspace_bytes, float *out_ao_map, float *out_lowres, float *out_shadow_map) {
  if (int rc = check_desc(desc, workspace, workspace_bytes)) return rc;
  if (!ao_map || !out_lowres || !out_shadow_map) return MPMHIP_ERR_INVALID;
  if (int rc = device_in_range(device)) return rc;
  if (desc->n == 0) return MPMHIP_OK;
  ENTRY_CHECK(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  const int C = desc->n_dims, S = desc->shadow_size, U = desc->uv_size, N = desc->n;
  const Workspace ws = workspace_layout(N, S, C);
  const Tables tb = tables_at((const int32_t *)desc->tables, S, U);
  float *base = (float *)workspace;
  WnArgs wn;
  for (int L = 0; L < LAYERS; ++L) {
    wn.v[L] = desc->weight_v[L]; wn.g[L] = desc->weight_g[L]; wn.w[L] = base + ws.w[L];
    wn.count[L] = layer_nw(C, L); wn.per_o[L] = layer_cin(C, L) * 9;
  }
  wn.norm = base + ws.norm;
  hipLaunchKernelGGL(k_shadow_wn, LAYERS, TPB, 0, st, wn);
  ENTRY_CHECK(hipGetLastError());
  for (int L = 0; L < LAYERS; ++L) {
    LayerFwd a;
    a.in = layer_input(L, C, S, tb, ws, base, ao_map, desc->ao_mean, desc->in_h, desc->in_w);
    a.w = base + ws.w[L];
    a.bias = desc->bias[L];
    a.bias_tied = L == HEAD && !desc->untied_head_bias;
    a.slope = desc->lrelu_slope;
    a.beta = desc->beta;
    a.out = L == HEAD ? out_lowres : base + ws.act[L];
    a.out2 = L == HEAD && U == S ? out_shadow_map : nullptr;
    a.ao_out = L == 0 ? out_ao_map : nullptr;
    const dim3 grid(tiles_x(a.in.size), tiles_y(a.in.size), N);
    if (C == 4) launch_layer<4>(L, grid, st, a); else launch_layer<8>(L, grid, st, a);
    ENTRY_CHECK(hipGetLastError());
  }
  if (U != S) {
    hipLaunchKernelGGL(k_shadow_resize, blocks((int64_t)N * U * U, TPB), TPB, 0, st, tb.fin, N, out_lowres, out_shadow_map);
    ENTRY_CHECK(hipGetLastError());
  }
  return MPMHIP_OK;
}

int mpmhip_shadow_backward(int32_t device, void *stream, const mpmhip_shadow_desc *desc, const float *ao_map, const float *lowres,
                           const float *g_shadow_map, const float *g_lowres, void *workspace, int64_t workspace_bytes) {
  if (int rc = check_desc(desc, workspace, workspace_bytes)) return rc;
  if (!ao_map || !lowres) return MPMHIP_ERR_INVALID;
  bool wanted = false;
  for (int L = 0; L < LAYERS; ++L) wanted = wanted || desc->d_weight_v[L] || desc->d_weight_g[L] || desc->d_bias[L];
  if (int rc = device_in_range(device)) return rc;
  if (desc->n == 0 || !wanted) return MPMHIP_OK;
  ENTRY_CHECK(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  const int C = desc->n_dims, S = desc->shadow_size, U = desc->uv_size, N = desc->n;
  const Workspace ws = workspace_layout(N, S, C);
  const Tables tb = tables_at((const int32_t *)desc->tables, S, U);
  float *base = (float *)workspace;
  hipLaunchKernelGGL(k_shadow_head_dz, blocks((int64_t)N * S * S, TPB), TPB, 0, st, tb.fin, U == S ? 1 : 0, N, g_shadow_map, g_lowres,
                     lowres, base + ws.dz);
  ENTRY_CHECK(hipGetLastError());
  ReduceArgs red;
  std::memset(&red, 0, sizeof(red));
  for (int L = LAYERS - 1; L >= 0; --L) {
    LayerBwd a;
    std::memset(&a, 0, sizeof(a));
    a.in = layer_input(L, C, S, tb, ws, base, ao_map, desc->ao_mean, desc->in_h, desc->in_w);
    a.w = base + ws.w[L];
    a.n = N;
    a.want_dw = desc->d_weight_v[L] || desc->d_weight_g[L];
    a.bias_tied = L == HEAD && !desc->untied_head_bias;
    a.tiles = layer_tiles(S, L);
    a.dx = L == 0 ? nullptr : base + ws.dx[L];
    a.d_bias = desc->d_bias[L];
    a.part = base + ws.part[L];
    a.part_bias = a.bias_tied && a.d_bias ? base + ws.part_bias : nullptr;
    a.gr = layer_grad(L, C, tb, ws, base, desc->lrelu_slope);
    const dim3 grid(tiles_x(a.in.size), tiles_y(a.in.size), 1);
    if (C == 4) launch_layer_backward<4>(L, grid, st, a); else launch_layer_backward<8>(L, grid, st, a);
    ENTRY_CHECK(hipGetLastError());
    red.part[L] = a.part; red.out[L] = base + ws.dw[L]; red.tiles[L] = a.tiles;
    red.first[L + 1] = a.want_dw ? layer_nw(C, L) : 0;  // a count for now
    if (a.part_bias) { red.part[LAYERS] = a.part_bias; red.out[LAYERS] = a.d_bias; red.tiles[LAYERS] = a.tiles; red.first[SLOTS] = 1; }
  }
  for (int k = 0; k < SLOTS; ++k) red.first[k + 1] += red.first[k];
  if (red.first[SLOTS] > 0) {
    hipLaunchKernelGGL(k_shadow_reduce, blocks((int64_t)red.first[SLOTS] * 64, TPB), TPB, 0, st, red);
    ENTRY_CHECK(hipGetLastError());
  }
  if (red.first[LAYERS] > 0) {
    WnBack wb;
    for (int L = 0; L < LAYERS; ++L) {
      wb.v[L] = desc->weight_v[L]; wb.g[L] = desc->weight_g[L]; wb.dw[L] = base + ws.dw[L];
      wb.dv[L] = desc->d_weight_v[L]; wb.dg[L] = desc->d_weight_g[L];
      wb.count[L] = layer_nw(C, L); wb.per_o[L] = layer_cin(C, L) * 9;
    }
    wb.norm = base + ws.norm;
    hipLaunchKernelGGL(k_shadow_wn_backward, LAYERS, TPB, 0, st, wb);
    ENTRY_CHECK(hipGetLastError());
  }
  return MPMHIP_OK;
}

}  // extern "C"
