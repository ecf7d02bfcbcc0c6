// raster_state.hpp -- what raster.hip (forward) and raster_backward.hip (backward) share: the handle, the layout of a saved
// frame, and the small host helpers of both.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "entry.hpp"
#include "raster_grad_math.hpp"

struct mpmhip_raster {
  int device = 0;
  hipStream_t stream = nullptr;
  // per Gaussian (capacity cap_n)
  int cap_n = 0;
  float4 *rec0 = nullptr, *rec1 = nullptr;  // (px, py, opacity, depth), (A, B, C, 0)
  float *colour = nullptr;                  // [n*3]
  int4 *rect = nullptr;                     // x0 y0 x1 y1
  uint32_t *touched = nullptr;              // [n + 1], the last one 0
  uint64_t *offsets = nullptr;              // [n + 1] exclusive scan; offsets[n] = number of entries
  void *scan_tmp = nullptr;
  size_t scan_tmp_bytes = 0;
  // per (tile, Gaussian) entry (capacity cap_e)
  size_t cap_e = 0;
  uint64_t *keys[2] = {nullptr, nullptr};
  uint32_t *vals[2] = {nullptr, nullptr};
  void *sort_tmp = nullptr;
  size_t sort_tmp_bytes = 0;
  // per tile (capacity cap_tiles)
  int cap_tiles = 0;
  uint2 *ranges = nullptr;
  // small
  uint64_t *h_total = nullptr;  // pinned
  int32_t *d_counts = nullptr;  // [2]: longest tile list, Gaussians with radius > 0 (mpmhip_raster_stats)
  // the last frame, for mpmhip_raster_stats
  int64_t last_entries = 0;
  int last_n = 0, last_tiles = 0;
  // Training flavour (mpmhip_raster_forward_grad / _save / _backward); nothing here is allocated before the first such call.
  size_t cap_pix = 0;
  float *pix_T = nullptr;        // per pixel: the final T itself (1 - alpha_out has lost the bits)
  uint32_t *pix_stop = nullptr;  // per pixel: the entry that finished it, or the end of its tile's range
  size_t cap_inv = 0;
  uint32_t *inv = nullptr;       // entry position before the sort (offsets[g] + place in g's rectangle) -> sorted position
  bool grad_frame = false;       // the newest frame recorded its per-pixel state: _save may copy it
  int grad_n = 0, grad_tiles = 0;
  size_t grad_pixels = 0;
  int64_t grad_entries = 0;
  size_t cap_rows = 0;
  float *rows = nullptr;         // the backward pass's own temporary: [entries][N_PARTIALS]
  // Extra attribute channels (raster_extra.hip); nothing here is allocated before the first backward pass with extras.
  int grad_w = 0, grad_h = 0;    // image size of the newest forward_grad frame: mpmhip_raster_extra_forward asks for the same
  size_t cap_xrows = 0;
  float *xrows = nullptr;        // the attribute partials of that backward pass: [entries][E]
  // mpmhip_raster_profile: events between the stages of a frame (off by default: no events, no extra synchronisation)
  bool profile = false;
  hipEvent_t ev[MPMHIP_RASTER_STAGES + 1] = {};
  double stage_ms[MPMHIP_RASTER_STAGES] = {};
  int64_t profiled_frames = 0;
};

namespace raster_host {

using namespace entry;
constexpr int TPB = 256;
constexpr int TILE = rast::TILE;
static_assert(TILE * TILE == TPB, "one lane per pixel of a tile");

struct Camera {  // the scalar half of mpmhip_raster_settings plus its three device pointers
  int W, H, gx, gy;
  float tanfovx, tanfovy, scale_modifier;
  int sh_degree;
  const float *view, *proj, *campos;
};

// A saved frame (mpmhip_raster_save): everything the backward pass reads of the forward one, copied out of the handle's
// scratch, which the next forward overwrites.  Offsets in bytes, every section 16-byte aligned but the last two.
struct SavedLayout {
  size_t rec0, rec1, rect, offsets, ranges, colour, pix_T, pix_stop, vals, inv, bytes;
};
inline SavedLayout saved_layout(size_t n, size_t tiles, size_t pixels, size_t entries) {
  auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
  SavedLayout l;
  size_t at = 0;
  l.rec0 = at; at += n * sizeof(float4);
  l.rec1 = at; at += n * sizeof(float4);
  l.rect = at; at += n * sizeof(int4);
  l.offsets = at; at = up(at + (n + 1) * sizeof(uint64_t));
  l.ranges = at; at = up(at + tiles * sizeof(uint2));
  l.colour = at; at = up(at + n * 3 * sizeof(float));
  l.pix_T = at; at = up(at + pixels * sizeof(float));
  l.pix_stop = at; at = up(at + pixels * sizeof(uint32_t));
  l.vals = at; at += entries * sizeof(uint32_t);
  l.inv = at; at += entries * sizeof(uint32_t);
  l.bytes = at;
  return l;
}

struct Inputs {  // of the forward call; exactly one of each alternative is non-NULL
  const float *means, *shs, *colors, *opac, *scales, *rots, *cov;
  int n_sh;
};

// What mpmhip_raster_forward* and mpmhip_raster_backward ask of a frame alike: handle, settings and the input alternatives
// (MPMHIP_ERR_INVALID), then the tile grid (MPMHIP_ERR_LIMIT).  The caller checks its own outputs BEFORE this, so that a
// missing output stays MPMHIP_ERR_INVALID on a frame that is also too large.
inline int validate_frame(const mpmhip_raster *r, const mpmhip_raster_settings *s, int32_t n, const Inputs &in, int *gx, int *gy) {
  if (!r || !s || n < 0 || s->image_height <= 0 || s->image_width <= 0) return MPMHIP_ERR_INVALID;
  if (!s->viewmatrix || !s->projmatrix || !s->campos) return MPMHIP_ERR_INVALID;
  if (n > 0) {
    if (!in.means || !in.opac) return MPMHIP_ERR_INVALID;
    if ((in.shs != nullptr) == (in.colors != nullptr)) return MPMHIP_ERR_INVALID;
    const bool sr = in.scales && in.rots;
    if ((in.scales != nullptr) != (in.rots != nullptr) || sr == (in.cov != nullptr)) return MPMHIP_ERR_INVALID;
    if (in.shs && (s->sh_degree < 0 || s->sh_degree > 3 || in.n_sh < (s->sh_degree + 1) * (s->sh_degree + 1))) return MPMHIP_ERR_INVALID;
  }
  *gx = (s->image_width + TILE - 1) / TILE;
  *gy = (s->image_height + TILE - 1) / TILE;
  if ((int64_t)*gx * *gy > INT32_MAX || *gy > 65535) return MPMHIP_ERR_LIMIT;
  return MPMHIP_OK;
}

struct Grads {  // the outputs of the backward call; the alternatives that the frame does not use are NULL
  float *means, *means2d, *shs, *colors, *opac, *scales, *rots, *cov;
};

// mpmhip_raster_backward in its stages (raster_backward.hip), so that mpmhip_raster_backward_extra (raster_extra.hip) runs the
// very same ones with its own tile pass in between:
//   backward_check      every condition of the call (MPMHIP_ERR_INVALID / _LIMIT); launches nothing.  *frame = the image
//                       size, the tile grid and the layout of `saved`
//   backward_tiles      the row buffer of the frame's entries and k_raster_backward_tiles over it (n_entries > 0)
//   backward_gaussians  k_raster_backward_gaussians over the rows (n > 0)
struct BackwardFrame {
  int W, H, gx, gy;
  SavedLayout l;
};
int backward_check(const mpmhip_raster *r, const mpmhip_raster_settings *s, int32_t n, const Inputs &in, const void *saved,
                   int64_t saved_bytes, int64_t n_entries, const Grads &out, BackwardFrame *frame);
int backward_tiles(mpmhip_raster *r, const mpmhip_raster_settings *s, int32_t n, const BackwardFrame &f, const void *saved,
                   int64_t n_entries, const float *dL_dimage, const float *dL_dalpha);
int backward_gaussians(mpmhip_raster *r, const mpmhip_raster_settings *s, int32_t n, const Inputs &in, const BackwardFrame &f,
                       const void *saved, int64_t n_entries, const Grads &out);

template <class T>
inline int regrow(T *&p, size_t count) {
  if (p) ENTRY_CHECK(hipFree(p));
  p = nullptr;
  return check(hipMalloc((void **)&p, count * sizeof(T)));
}

// capacity that holds `need`: at least twice the old one, so that a slowly growing scene reallocates O(log) times
template <class I>
inline I grown(I cap, I need) { return need > 2 * cap ? need : 2 * cap; }

// temporary storage of a rocPRIM call: asked for with the call's own arguments every frame (a host-side computation)
inline int reserve_tmp(mpmhip_raster *r, void *&p, size_t &have, size_t need) {
  if (need <= have) return MPMHIP_OK;
  ENTRY_CHECK(hipStreamSynchronize(r->stream));
  const size_t cap = grown(have, need);
  char *tmp = (char *)p;
  p = nullptr;
  have = 0;
  if (int rc = regrow(tmp, cap)) return rc;
  p = tmp;
  have = cap;
  return MPMHIP_OK;
}

inline int reserve_gaussians(mpmhip_raster *r, int n) {
  if (n <= r->cap_n) return MPMHIP_OK;
  ENTRY_CHECK(hipStreamSynchronize(r->stream));  // nothing in flight may still read what is freed
  const int cap = grown(r->cap_n, n);
  r->cap_n = 0;
  if (int rc = regrow(r->rec0, (size_t)cap)) return rc;
  if (int rc = regrow(r->rec1, (size_t)cap)) return rc;
  if (int rc = regrow(r->colour, (size_t)cap * 3)) return rc;
  if (int rc = regrow(r->rect, (size_t)cap)) return rc;
  if (int rc = regrow(r->touched, (size_t)cap + 1)) return rc;
  if (int rc = regrow(r->offsets, (size_t)cap + 1)) return rc;
  r->cap_n = cap;
  return MPMHIP_OK;
}

inline int reserve_entries(mpmhip_raster *r, size_t total) {
  if (total <= r->cap_e) return MPMHIP_OK;
  ENTRY_CHECK(hipStreamSynchronize(r->stream));
  const size_t cap = grown(r->cap_e, total);
  r->cap_e = 0;
  for (int k = 0; k < 2; ++k) {
    if (int rc = regrow(r->keys[k], cap)) return rc;
    if (int rc = regrow(r->vals[k], cap)) return rc;
  }
  r->cap_e = cap;
  return MPMHIP_OK;
}

inline int reserve_tiles(mpmhip_raster *r, int tiles) {
  if (tiles <= r->cap_tiles) return MPMHIP_OK;
  ENTRY_CHECK(hipStreamSynchronize(r->stream));
  const int cap = grown(r->cap_tiles, tiles);
  r->cap_tiles = 0;
  if (int rc = regrow(r->ranges, (size_t)cap)) return rc;
  r->cap_tiles = cap;
  return MPMHIP_OK;
}

}  // namespace raster_host
