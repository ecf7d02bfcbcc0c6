// lpips.hip -- LPIPS of the appearance loop on the device (lpipsPyTorch, net_type 'vgg'; the call is train_appearance.py:133):
// mpmhip_lpips_prepare_weights, mpmhip_lpips_workspace_bytes, mpmhip_lpips_forward, mpmhip_lpips_backward.  The function, the K walk,
// the tile loads, the epilogues, the head and the workspace are lpips_math.hpp; this file is the kernels over it and the launches.
//
//   prepare   k_lpips_flip: the thirteen backward layouts [cin][cout][3][3], flipped and transposed                         = 1
//   forward   thirteen k_lpips_conv (x and y in the same launch) + five k_lpips_head + k_lpips_sum                         = 19
//   backward  five k_lpips_head_backward + thirteen k_lpips_conv over the backward layouts                                 = 18
//
// k_lpips_conv is an implicit GEMM on v_mfma_f32_32x32x2_f32: M = output channels, N = output pixels, K = 9 * input channels, NCHW.
// A workgroup of four waves owns 64 channels x (4 rows x 32 columns) of one image; a wave owns 32 channels x 2 rows, one 32 x 32
// accumulator block per row (a block's 32 pixels are one row of the tile, so its LDS reads are 32 consecutive floats).  K is walked in
// chunks of 8 input channels (72 k, 36 MFMA steps per block): the chunk's input tile with its halo [8][6][34] is filled THROUGH the
// layer's input rule (z-score; the 2 x 2 maximum of the map in front of a pooling, so that no pooled map exists; backward: the ReLU
// mask of the saved output over the arriving gradient, routed through the pooling, plus the tap's gradient), the weight slice lands
// in LDS as [k][m] with rows of 65 floats (the global read walks k, the operand read walks m; neither meets a bank twice within a
// half-wave).  Lane l feeds A[m = l & 31][k = l >> 5] and B[k = l >> 5][pixel = l & 31]; two consecutive k per instruction keep the
// chain in k order.  The epilogue adds the bias and applies ReLU (backward: nothing; the image: the division by std).
// No floating-point atomics; every sum has a fixed order.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "entry.hpp"
#include "lpips_math.hpp"

namespace {

using namespace entry;
using namespace lpips;

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct ConvArgs {
  Source src;
  Sink sink;
  const float *w;      // [m][k_total]: the forward layout of a layer, or its backward layout
  int32_t k_total;     // 9 * src.c
  int32_t m_tiles;     // workgroups along the output channels; blockIdx.z = image * m_tiles + m tile
};

template <int CK>   // input channels per K chunk: CHUNK_C, or 3 for the image layer
__global__ void __launch_bounds__(TPB) k_lpips_conv(ConvArgs a) {
  constexpr int KC = CK * 9, KCP = k_padded(KC);
  __shared__ float wl[KCP * W_STRIDE];
  __shared__ float tile[CK * PLANE];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, half = lane >> 5, col = lane & 31;
  const int b = blockIdx.z / a.m_tiles, m0 = (blockIdx.z % a.m_tiles) * TILE_M;
  const int ty0 = blockIdx.y * TILE_H, tx0 = blockIdx.x * TILE_W;
  const int mb = (wave & 1) * 32, r0 = (wave >> 1) * 2;
  f32x16 acc0, acc1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
  for (int c0 = 0; c0 < a.src.c; c0 += CK) {
    for (int idx = t; idx < CK * PLANE; idx += TPB) {
      const int c = idx / PLANE, r = idx % PLANE;
      tile[idx] = tile_value(a.src, b, c0 + c, ty0 + r / HALO_W - 1, tx0 + r % HALO_W - 1);
    }
    for (int idx = t; idx < TILE_M * KCP; idx += TPB) {
      const int m = idx / KCP, k = idx % KCP;
      wl[k * W_STRIDE + m] = (m0 + m < a.sink.m && k < KC) ? a.w[(int64_t)(m0 + m) * a.k_total + c0 * 9 + k] : 0.f;
    }
    __syncthreads();
    const float *wrow = wl + half * W_STRIDE + mb + col;
    const float *trow = tile + r0 * HALO_W + col;
#pragma unroll
    for (int kk = 0; kk < KCP / 2; ++kk) {
      const float av = wrow[2 * kk * W_STRIDE];
      float b0, b1;
      if (2 * kk + 1 < KC) {
        const int off = half ? k_offset(2 * kk + 1) : k_offset(2 * kk);
        b0 = trow[off];
        b1 = trow[off + HALO_W];
      } else {   // the odd K of the image layer: the second k slot is the product 0 * 0
        b0 = half ? 0.f : trow[k_offset(2 * kk)];
        b1 = half ? 0.f : trow[k_offset(2 * kk) + HALO_W];
      }
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1, acc1, 0, 0, 0);
    }
    __syncthreads();
  }
  const int x = tx0 + col, y0 = ty0 + r0;
  if (x >= a.sink.w) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = m0 + mb + (r & 3) + 8 * (r >> 2) + 4 * half;
    if (m >= a.sink.m) continue;
    if (y0 < a.sink.h) *sink_at(a.sink, b, m, y0, x) = sink_value(a.sink, m, acc0[r]);
    if (y0 + 1 < a.sink.h) *sink_at(a.sink, b, m, y0 + 1, x) = sink_value(a.sink, m, acc1[r]);
  }
}

#ifdef LPIPS_POOL_KERNEL
// A/B build only (tools/lpips_bench.py with MPMHIP_LIB): the 2 x 2 maximum written by a kernel of its own
// instead of being folded into the next layer's tile load.  planes = images * channels; src [planes, sh, sw] -> dst [planes, h, w]
__global__ void __launch_bounds__(TPB) k_lpips_pool(const float *src, float *dst, int64_t planes, int h, int w, int sh, int sw) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= planes * h * w) return;
  const int x = (int)(i % w), y = (int)((i / w) % h);
  const float *o = src + ((i / ((int64_t)h * w)) * sh + 2 * y) * sw + 2 * x;
  dst[i] = max4(o[0], o[1], o[sw], o[sw + 1]);
}
#endif

struct FlipArgs {
  const float *w[LAYERS];
  float *wb[LAYERS];
  int64_t first[LAYERS + 1];   // the elements first[L] .. first[L + 1] - 1 of the launch are layer L's
};

__global__ void __launch_bounds__(TPB) k_lpips_flip(FlipArgs a) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= a.first[LAYERS]) return;
  int L = 0;
  while (i >= a.first[L + 1]) ++L;
  const int64_t e = i - a.first[L];
  a.wb[L][e] = a.w[L][flipped_source(layer_cin(L), layer_cout(L), e)];
}

// the sum of one double per lane over the workgroup in a fixed tree; the result is in every lane's return
__device__ double block_sum(double v, double *red) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int s = TPB / 2; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  const double total = red[0];
  __syncthreads();
  return total;
}

// lanes over the pixels of image blockIdx.y, channels walked inside: reads of a channel plane are coalesced
__global__ void __launch_bounds__(TPB) k_lpips_head(const float *fx, const float *fy, const float *w, int c_count, int hw, double *part) {
  __shared__ double red[TPB];
  const int n = blockIdx.y, p = blockIdx.x * TPB + threadIdx.x;
  float s = 0.f;
  if (p < hw) {
    const int64_t at = (int64_t)n * c_count * hw + p;
    s = head_pixel(fx + at, fy + at, w, c_count, hw);
  }
  const double total = block_sum((double)s, red);
  if (threadIdx.x == 0) part[(int64_t)n * gridDim.x + blockIdx.x] = total;
}

struct SumArgs {
  const double *part[TAPS];
  int32_t count[TAPS], hw[TAPS];
};

// one workgroup: per tap the slots in ascending order per lane, the tree, the division by the tap's pixels; taps in order
__global__ void __launch_bounds__(TPB) k_lpips_sum(SumArgs a, float *out) {
  __shared__ double red[TPB];
  double total = 0.0;
  for (int k = 0; k < TAPS; ++k) {
    double v = 0.0;
    for (int i = threadIdx.x; i < a.count[k]; i += TPB) v += a.part[k][i];
    total += block_sum(v, red) / (double)a.hw[k];
  }
  if (threadIdx.x == 0) out[0] = (float)total;
}

__global__ void __launch_bounds__(TPB) k_lpips_head_backward(const float *fx, const float *fy, const float *w, int c_count, int hw,
                                                            const float *g_out, float *dfx) {
  const int n = blockIdx.y, p = blockIdx.x * TPB + threadIdx.x;
  if (p >= hw) return;
  const int64_t at = (int64_t)n * c_count * hw + p;
  head_pixel_backward(fx + at, fy + at, w, c_count, hw, g_out[0] / (float)hw, dfx + at);
}

// ---- the host side -----------------------------------------------------------------------------------------------------------------------

int check_sizes(const mpmhip_lpips_desc *d) {
  if (!d) return MPMHIP_ERR_INVALID;
  if (d->n < 0 || d->n > MAX_BATCH || d->h < MIN_SIZE || d->w < MIN_SIZE || d->h > MAX_SIZE || d->w > MAX_SIZE) return MPMHIP_ERR_INVALID;
  return MPMHIP_OK;
}

int check_desc(const mpmhip_lpips_desc *d, const void *workspace, int64_t workspace_bytes, int keep) {
  if (int rc = check_sizes(d)) return rc;
  if (keep != 0 && keep != 1) return MPMHIP_ERR_INVALID;
  for (int L = 0; L < LAYERS; ++L)
    if (!d->weight[L] || !d->bias[L] || (keep && !d->weight_bwd[L])) return MPMHIP_ERR_INVALID;
  for (int t = 0; t < TAPS; ++t)
    if (!d->tap_weight[t]) return MPMHIP_ERR_INVALID;
  for (int c = 0; c < 3; ++c)
    if (!std::isfinite(d->mean[c]) || !std::isfinite(d->std[c]) || d->std[c] == 0.f) return MPMHIP_ERR_INVALID;
  if (!workspace || workspace_bytes < 4 * workspace_layout(d->n, d->h, d->w, keep).words) return MPMHIP_ERR_INVALID;
  return MPMHIP_OK;
}

int launch_conv(hipStream_t st, const ConvArgs &a, int images) {
  const dim3 grid(tiles_x(a.sink.w), tiles_y(a.sink.h), images * a.m_tiles);
  if (a.src.c == 3) hipLaunchKernelGGL(k_lpips_conv<3>, grid, TPB, 0, st, a);
  else hipLaunchKernelGGL(k_lpips_conv<CHUNK_C>, grid, TPB, 0, st, a);
  return check(hipGetLastError());
}

}  // namespace

extern "C" {

int mpmhip_lpips_prepare_weights(int32_t device, void *stream, const mpmhip_lpips_desc *desc) {
  if (!desc) return MPMHIP_ERR_INVALID;
  for (int L = 0; L < LAYERS; ++L)
    if (!desc->weight[L] || !desc->weight_bwd[L]) return MPMHIP_ERR_INVALID;
  if (int rc = device_in_range(device)) return rc;
  ENTRY_CHECK(hipSetDevice(device));
  FlipArgs a;
  a.first[0] = 0;
  for (int L = 0; L < LAYERS; ++L) {
    a.w[L] = desc->weight[L];
    a.wb[L] = desc->weight_bwd[L];
    a.first[L + 1] = a.first[L] + layer_weights(L);
  }
  hipLaunchKernelGGL(k_lpips_flip, blocks(a.first[LAYERS], TPB), TPB, 0, (hipStream_t)stream, a);
  return check(hipGetLastError());
}

int mpmhip_lpips_workspace_bytes(int32_t device, void *stream, const mpmhip_lpips_desc *desc, int32_t keep, int64_t *out_workspace_bytes) {
  (void)stream;
  if (int rc = check_sizes(desc)) return rc;
  if (!out_workspace_bytes || (keep != 0 && keep != 1)) return MPMHIP_ERR_INVALID;
  *out_workspace_bytes = 4 * workspace_layout(desc->n, desc->h, desc->w, keep).words;   // host arithmetic, whatever the device
  return device_in_range(device);
}

int mpmhip_lpips_forward(int32_t device, void *stream, const mpmhip_lpips_desc *desc, const float *x, const float *y, int32_t keep,
                         void *workspace, int64_t workspace_bytes, float *out) {
  if (int rc = check_desc(desc, workspace, workspace_bytes, keep)) return rc;
  if (!x || !y || !out) return MPMHIP_ERR_INVALID;
  if (int rc = device_in_range(device)) return rc;
  ENTRY_CHECK(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  const int N = desc->n, H = desc->h, W = desc->w;
  if (N == 0) return check(hipMemsetAsync(out, 0, sizeof(float), st));
  const Workspace ws = workspace_layout(N, H, W, keep);
  float *base = (float *)workspace;
  for (int L = 0; L < LAYERS; ++L) {
    const int level = layer_level(L), h = level_size(H, level), w = level_size(W, level);
    ConvArgs a;
    std::memset(&a, 0, sizeof(a));
    a.src.mode = L == 0 ? SRC_IMAGE : pool_in_front(L) ? SRC_POOLED : SRC_PLAIN;
    a.src.n_first = N; a.src.c = layer_cin(L); a.src.h = h; a.src.w = w;
    a.src.sh = pool_in_front(L) ? level_size(H, level - 1) : h;
    a.src.sw = pool_in_front(L) ? level_size(W, level - 1) : w;
    a.src.p0 = L == 0 ? x : base + ws.x[L - 1];
    a.src.p1 = L == 0 ? y : base + ws.y[L - 1];
    for (int c = 0; c < 3; ++c) { a.src.mean[c] = desc->mean[c]; a.src.std[c] = desc->std[c]; }
#ifdef LPIPS_POOL_KERNEL
    if (pool_in_front(L)) {
      for (int side = 0; side < 2; ++side) {
        const int64_t planes = (int64_t)N * a.src.c;
        hipLaunchKernelGGL(k_lpips_pool, blocks(planes * h * w, TPB), TPB, 0, st, side ? a.src.p1 : a.src.p0, base + ws.dgrad[side], planes, h,
                           w, a.src.sh, a.src.sw);
        ENTRY_CHECK(hipGetLastError());
      }
      a.src.mode = SRC_PLAIN; a.src.p0 = base + ws.dgrad[0]; a.src.p1 = base + ws.dgrad[1]; a.src.sh = h; a.src.sw = w;
    }
#endif
    a.sink.mode = SINK_RELU; a.sink.n_first = N; a.sink.m = layer_cout(L); a.sink.h = h; a.sink.w = w;
    a.sink.o0 = base + ws.x[L]; a.sink.o1 = base + ws.y[L]; a.sink.bias = desc->bias[L];
    a.w = desc->weight[L]; a.k_total = 9 * a.src.c; a.m_tiles = (a.sink.m + TILE_M - 1) / TILE_M;
    if (int rc = launch_conv(st, a, 2 * N)) return rc;
  }
  SumArgs sum;
  for (int t = 0; t < TAPS; ++t) {
    const int L = tap_layer(t), hw = level_size(H, t) * level_size(W, t), groups = head_groups(H, W, t);
    double *part = (double *)(base + ws.part[t]);
    hipLaunchKernelGGL(k_lpips_head, dim3(groups, N), TPB, 0, st, base + ws.x[L], base + ws.y[L], desc->tap_weight[t], layer_cout(L), hw, part);
    ENTRY_CHECK(hipGetLastError());
    sum.part[t] = part; sum.count[t] = N * groups; sum.hw[t] = hw;
  }
  hipLaunchKernelGGL(k_lpips_sum, 1, TPB, 0, st, sum, out);
  return check(hipGetLastError());
}

int mpmhip_lpips_backward(int32_t device, void *stream, const mpmhip_lpips_desc *desc, const float *g_out, void *workspace,
                          int64_t workspace_bytes, float *dx) {
  if (int rc = check_desc(desc, workspace, workspace_bytes, 1)) return rc;
  if (!g_out || !dx) return MPMHIP_ERR_INVALID;
  if (int rc = device_in_range(device)) return rc;
  if (desc->n == 0) return MPMHIP_OK;
  ENTRY_CHECK(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  const int N = desc->n, H = desc->h, W = desc->w;
  const Workspace ws = workspace_layout(N, H, W, 1);
  float *base = (float *)workspace;
  for (int t = 0; t < TAPS; ++t) {
    const int L = tap_layer(t), hw = level_size(H, t) * level_size(W, t);
    hipLaunchKernelGGL(k_lpips_head_backward, dim3(head_groups(H, W, t), N), TPB, 0, st, base + ws.x[L], base + ws.y[L],
                       desc->tap_weight[t], layer_cout(L), hw, g_out, base + ws.dtap[t]);
    ENTRY_CHECK(hipGetLastError());
  }
  for (int L = LAYERS - 1; L >= 0; --L) {
    const int level = layer_level(L), h = level_size(H, level), w = level_size(W, level);
    const bool pooled = L + 1 < LAYERS && pool_in_front(L + 1);
    ConvArgs a;
    std::memset(&a, 0, sizeof(a));
    a.src.mode = SRC_GRAD; a.src.n_first = N; a.src.c = layer_cout(L); a.src.h = h; a.src.w = w;
    a.src.pooled = pooled;
    a.src.sh = pooled ? level_size(H, level + 1) : h;
    a.src.sw = pooled ? level_size(W, level + 1) : w;
    a.src.p0 = base + ws.x[L];
    a.src.p1 = tap_of(L) >= 0 ? base + ws.dtap[tap_of(L)] : nullptr;
    a.src.p2 = L + 1 < LAYERS ? base + ws.dgrad[(L + 1) & 1] : nullptr;
    a.sink.mode = L == 0 ? SINK_IMAGE : SINK_PLAIN; a.sink.n_first = N; a.sink.m = layer_cin(L); a.sink.h = h; a.sink.w = w;
    a.sink.o0 = L == 0 ? dx : base + ws.dgrad[L & 1];
    for (int c = 0; c < 3; ++c) a.sink.std[c] = desc->std[c];
    a.w = desc->weight_bwd[L]; a.k_total = 9 * a.src.c; a.m_tiles = (a.sink.m + TILE_M - 1) / TILE_M;
    if (int rc = launch_conv(st, a, N)) return rc;
  }
  return MPMHIP_OK;
}

}  // extern "C"
