// ao_math.hpp -- the ambient-occlusion bake of the evaluation and demo loops (blender/bake.py, driven from
// train_material_params.py:819-881): for every texel of the UV map that a face covers, the fraction of a cosine-weighted
// hemisphere around the face normal that the mesh itself leaves open.  What is taken from bake.py: the resolution (--ao_res), the
// margin (ao_res // 256), the bake type AO, the black background, the row order of the PNG.  What is NOT known: Cycles' sampling
// pattern, its ray offset and the transfer curve of its 8-bit file; Blender cannot run where this code runs, so the sampling here
// is a definition of this project, not a copy: a fixed Hammersley table of cosine-weighted directions,
// rotated per texel about the normal by a hashed angle, any-hit Moeller-Trumbore against every other face of the mesh.
//
// Plain C++ for the device (ao.hip) and the host (tests/hostao/) alike: one function per work item, so the kernels and the host
// loops are the same statements.  Rounding is pinned: every fused operation is an explicit __builtin_fmaf, everything else is
// compiled with contraction off (AO_STRICT), division and square root are the correctly rounded ones, so both builds give the
// same bits.  Coverage and barycentrics are float64 and rounded once to fp32; everything per frame is fp32.
//
// The acceleration structure is a uniform grid over the mesh's bounding box.  Its two pure functions are here: face_cells (the
// cells a face is inserted into: those its bounding box, inflated by INFLATE of a cell, overlaps) and walk (the cells a ray
// visits, in order, each handed to a visitor).  The walk never accumulates: the parameter of the next cell wall is recomputed from
// the integer cell index at every step, so its error is a few ulp of the coordinates (about 1e-5 of a cell at 128 cells per axis),
// two orders below the inflation.  A hit that the fp32 walk would step past, because the ray clips a corner of a cell for less
// than that, lies that close to a wall, so the face is also listed in the neighbouring cell the walk does visit.
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#define AO_STRICT _Pragma("clang fp contract(off)")

namespace ao {

constexpr float INFLATE = 1e-3f;     // of a cell: what a face's box grows by before it is binned, and the slack of the box clip
constexpr int MAX_DIM = 1024;        // cells per axis at the most
constexpr int MAX_SAMPLES = 4096;

struct V3 { float x, y, z; };

__host__ __device__ __forceinline__ V3 sub(V3 a, V3 b) { AO_STRICT return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__host__ __device__ __forceinline__ float dot(V3 a, V3 b) { return __builtin_fmaf(a.z, b.z, __builtin_fmaf(a.y, b.y, a.x * b.x)); }
__host__ __device__ __forceinline__ V3 cross(V3 a, V3 b) {
  AO_STRICT
  return V3{__builtin_fmaf(a.y, b.z, -(a.z * b.y)), __builtin_fmaf(a.z, b.x, -(a.x * b.z)), __builtin_fmaf(a.x, b.y, -(a.y * b.x))};
}
// a + s b
__host__ __device__ __forceinline__ V3 axpy(float s, V3 b, V3 a) {
  return V3{__builtin_fmaf(s, b.x, a.x), __builtin_fmaf(s, b.y, a.y), __builtin_fmaf(s, b.z, a.z)};
}
__host__ __device__ __forceinline__ V3 scale(float s, V3 a) { AO_STRICT return V3{s * a.x, s * a.y, s * a.z}; }
__host__ __device__ __forceinline__ V3 load3(const float *p, int64_t i) { return V3{p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }
__host__ __device__ __forceinline__ void store3(float *p, int64_t i, V3 v) { p[3 * i] = v.x; p[3 * i + 1] = v.y; p[3 * i + 2] = v.z; }

// ---- coverage (once per mesh, float64) ------------------------------------------------------------------------------------

__host__ __device__ __forceinline__ double edge(double ax, double ay, double bx, double by, double px, double py) {
  AO_STRICT
  return (bx - ax) * (py - ay) - (by - ay) * (px - ax);
}

// centre of texel (row y, column x): row 0 is the top of the image, v = 1 at the top (mesh_gaussian_model.py:110)
__host__ __device__ __forceinline__ void texel_centre(int x, int y, int H, int W, double *u, double *v) {
  AO_STRICT
  *u = ((double)x + 0.5) / (double)W;
  *v = 1.0 - ((double)y + 0.5) / (double)H;
}

// Is (pu, pv) inside the UV triangle a b c, either winding, edges inclusive; a triangle without area contains nothing.
// b1, b2: the weights of b and c, so that p = a + b1 (b - a) + b2 (c - a).
__host__ __device__ __forceinline__ bool uv_contains(const float *a, const float *b, const float *c, double pu, double pv, double *b1, double *b2) {
  AO_STRICT
  const double ax = a[0], ay = a[1], bx = b[0], by = b[1], cx = c[0], cy = c[1];
  const double area = edge(ax, ay, bx, by, cx, cy);
  if (!(area != 0.0)) return false;  // NaN as well
  const double w0 = edge(bx, by, cx, cy, pu, pv), w1 = edge(cx, cy, ax, ay, pu, pv), w2 = edge(ax, ay, bx, by, pu, pv);
  const bool pos = w0 >= 0.0 && w1 >= 0.0 && w2 >= 0.0, neg = w0 <= 0.0 && w1 <= 0.0 && w2 <= 0.0;
  if (!(pos || neg)) return false;
  *b1 = w1 / area;
  *b2 = w2 / area;
  return true;
}

// A face that names a vertex twice has no area in any frame: it covers nothing.  (A face that merely collapses in one frame
// keeps its texels; they bake to 0 in that frame, texel_frame's ok = false.)
__host__ __device__ __forceinline__ bool face_has_area(const int32_t *faces, int64_t f) {
  const int32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
  return a != b && b != c && a != c;
}

// claim(texel) for every texel whose centre face f's UV triangle contains.  The candidates are the texels of the triangle's
// bounding box, rounded outwards.
template <class Claim>
__host__ __device__ __forceinline__ void face_texels(int64_t f, const int32_t *faces, const int32_t *ft, const float *vt, int H, int W, Claim &&claim) {
  AO_STRICT
  if (!face_has_area(faces, f)) return;
  const float *a = vt + 2 * (int64_t)ft[3 * f], *b = vt + 2 * (int64_t)ft[3 * f + 1], *c = vt + 2 * (int64_t)ft[3 * f + 2];
  const double umin = fmin(fmin((double)a[0], (double)b[0]), (double)c[0]), umax = fmax(fmax((double)a[0], (double)b[0]), (double)c[0]);
  const double vmin = fmin(fmin((double)a[1], (double)b[1]), (double)c[1]), vmax = fmax(fmax((double)a[1], (double)b[1]), (double)c[1]);
  // decided on the doubles: a triangle far outside the map never becomes an integer
  const double fx0 = fmax(floor(umin * W - 0.5), 0.0), fx1 = fmin(ceil(umax * W - 0.5), (double)(W - 1));
  const double fy0 = fmax(floor((1.0 - vmax) * H - 0.5), 0.0), fy1 = fmin(ceil((1.0 - vmin) * H - 0.5), (double)(H - 1));
  if (!(fx0 <= fx1 && fy0 <= fy1)) return;
  const int x0 = (int)fx0, x1 = (int)fx1, y0 = (int)fy0, y1 = (int)fy1;
  for (int y = y0; y <= y1; ++y)
    for (int x = x0; x <= x1; ++x) {
      double pu, pv, b1, b2;
      texel_centre(x, y, H, W, &pu, &pv);
      if (uv_contains(a, b, c, pu, pv, &b1, &b2)) claim(y * W + x);
    }
}

// the two barycentrics of a texel inside face f, rounded once to fp32
__host__ __device__ __forceinline__ void texel_bary(int texel, int64_t f, const int32_t *ft, const float *vt, int H, int W, float *bary) {
  double pu, pv, b1 = 0.0, b2 = 0.0;
  texel_centre(texel % W, texel / W, H, W, &pu, &pv);
  uv_contains(vt + 2 * (int64_t)ft[3 * f], vt + 2 * (int64_t)ft[3 * f + 1], vt + 2 * (int64_t)ft[3 * f + 2], pu, pv, &b1, &b2);
  bary[0] = (float)b1;
  bary[1] = (float)b2;
}

// ---- the texel frame (per frame, fp32) ------------------------------------------------------------------------------------

struct Frame {
  V3 p, n, t, b;
  bool ok;  // false: the face has no area in this frame; everything is zero
};

__host__ __device__ __forceinline__ V3 normalized(V3 a, float *len) {
  AO_STRICT
  *len = sqrtf(dot(a, a));
  return V3{a.x / *len, a.y / *len, a.z / *len};
}

// origin p = v0 + b1 e1 + b2 e2; n the geometric normal (an OBJ without vn lines is flat shaded); t the unit projection onto the
// tangent plane of the coordinate axis least aligned with n (the lowest axis on a tie), turned about n by the angle of (c, s);
// b = n x t.
__host__ __device__ __forceinline__ Frame texel_frame(V3 v0, V3 v1, V3 v2, float b1, float b2, float c, float s) {
  AO_STRICT
  Frame fr{V3{0.f, 0.f, 0.f}, V3{0.f, 0.f, 0.f}, V3{0.f, 0.f, 0.f}, V3{0.f, 0.f, 0.f}, false};
  const V3 e1 = sub(v1, v0), e2 = sub(v2, v0);
  float len;
  const V3 n = normalized(cross(e1, e2), &len);
  if (!(len > 0.f) || !(len < INFINITY)) return fr;
  const float ax = fabsf(n.x), ay = fabsf(n.y), az = fabsf(n.z);
  const int k = (ax <= ay && ax <= az) ? 0 : (ay <= az ? 1 : 2);
  const float nk = k == 0 ? n.x : k == 1 ? n.y : n.z;
  float tlen;
  const V3 t0 = normalized(axpy(-nk, n, V3{k == 0 ? 1.f : 0.f, k == 1 ? 1.f : 0.f, k == 2 ? 1.f : 0.f}), &tlen);
  const V3 b0 = cross(n, t0);
  fr.p = axpy(b2, e2, axpy(b1, e1, v0));
  fr.n = n;
  fr.t = axpy(s, b0, scale(c, t0));
  fr.b = cross(n, fr.t);
  fr.ok = true;
  return fr;
}

// ray i of a texel: table direction (dx, dy, dz) in the frame
__host__ __device__ __forceinline__ V3 ray_dir(const Frame &fr, const float *dirs, int i) {
  return axpy(dirs[3 * i + 2], fr.n, axpy(dirs[3 * i + 1], fr.b, scale(dirs[3 * i], fr.t)));
}

// ---- occlusion ------------------------------------------------------------------------------------------------------------

// One triangle as the trace reads it: 48 bytes, three 16-byte loads.
struct alignas(16) Tri {
  float v0x, v0y, v0z, e1x, e1y, e1z, e2x, e2y, e2z, pad0, pad1, pad2;
};
static_assert(sizeof(Tri) == 48, "a triangle record is three 16-byte loads");

__host__ __device__ __forceinline__ Tri make_tri(V3 v0, V3 v1, V3 v2) {
  const V3 e1 = sub(v1, v0), e2 = sub(v2, v0);
  return Tri{v0.x, v0.y, v0.z, e1.x, e1.y, e1.z, e2.x, e2.y, e2.z, 0.f, 0.f, 0.f};
}

// Moeller-Trumbore: does the ray o + t d meet the triangle with bias < t <= tmax.  Both sides count; a triangle seen edge-on
// (det == 0) or without area never does; any NaN gives false.
__host__ __device__ __forceinline__ bool ray_hits(V3 o, V3 d, const Tri &tr, float bias, float tmax) {
  AO_STRICT
  const V3 v0{tr.v0x, tr.v0y, tr.v0z}, e1{tr.e1x, tr.e1y, tr.e1z}, e2{tr.e2x, tr.e2y, tr.e2z};
  const V3 pvec = cross(d, e2);
  const float det = dot(e1, pvec);
  if (!(det != 0.f)) return false;
  const float inv = 1.f / det;
  const V3 tvec = sub(o, v0);
  const float u = dot(tvec, pvec) * inv;
  if (!(u >= 0.f)) return false;
  const V3 qvec = cross(tvec, e1);
  const float v = dot(d, qvec) * inv;
  if (!(v >= 0.f) || !(u + v <= 1.f)) return false;
  const float t = dot(e2, qvec) * inv;
  return t > bias && t <= tmax;
}

// ---- the uniform grid -----------------------------------------------------------------------------------------------------

struct Grid {
  float lo[3];
  float cs, inv_cs;  // cell edge and its reciprocal
  int32_t dim[3];
  int32_t n_cells;
  int32_t pad_[7];
};
static_assert(sizeof(Grid) == 64, "Grid is one 64-byte record in the scratch");

// The grid over the box [lo, hi] of the mesh: cubic cells of about twice the mean edge length, grown until there are at most
// cap_cells of them.  Every axis gets floor(extent / cell) + 1 cells centred on the box, so a flat sheet (extent 0) gets one
// cell that pads it by half a cell on either side, and the mesh never touches the outer walls.
__host__ __device__ __forceinline__ Grid grid_setup(const float *lo, const float *hi, float mean_edge, int32_t cap_cells) {
  AO_STRICT
  Grid g{};
  float ext[3], longest = 0.f;
  for (int k = 0; k < 3; ++k) {
    ext[k] = hi[k] - lo[k];
    if (!(ext[k] >= 0.f) || !(ext[k] < INFINITY)) ext[k] = 0.f;  // no faces, or a NaN vertex: a grid of one cell
    longest = fmaxf(longest, ext[k]);
  }
  float cs = 2.f * mean_edge;
  if (!(cs > 0.f) || !(cs < INFINITY)) cs = longest > 0.f ? longest : 1.f;
  cs = fmaxf(cs, longest / (float)(MAX_DIM - 1));
  for (int it = 0; it < 256; ++it) {
    int64_t cells = 1;
    for (int k = 0; k < 3; ++k) {
      g.dim[k] = (int32_t)fminf(floorf(ext[k] / cs), (float)(MAX_DIM - 1)) + 1;
      cells *= g.dim[k];
    }
    if (cells <= cap_cells || (g.dim[0] == 1 && g.dim[1] == 1 && g.dim[2] == 1)) break;
    cs = cs * 1.25f;
  }
  g.cs = cs;
  g.inv_cs = 1.f / cs;
  g.n_cells = g.dim[0] * g.dim[1] * g.dim[2];
  for (int k = 0; k < 3; ++k) {
    const float l = (ext[k] > 0.f || (lo[k] == lo[k] && fabsf(lo[k]) < INFINITY)) ? lo[k] : 0.f;
    g.lo[k] = l + 0.5f * (ext[k] - (float)g.dim[k] * cs);
  }
  return g;
}

__host__ __device__ __forceinline__ int32_t cell_of(const Grid &g, int k, float x, float shift) {
  AO_STRICT
  const float c = floorf((x - g.lo[k]) * g.inv_cs + shift);
  return (int32_t)fminf(fmaxf(c, 0.f), (float)(g.dim[k] - 1));  // on the floats; fmaxf drops a NaN
}

// The cells face (v0, v1, v2) is inserted into: every cell its bounding box, grown by INFLATE of a cell, overlaps.
__host__ __device__ __forceinline__ void face_cells(const Grid &g, V3 v0, V3 v1, V3 v2, int32_t *c_lo, int32_t *c_hi) {
  const float mn[3] = {fminf(fminf(v0.x, v1.x), v2.x), fminf(fminf(v0.y, v1.y), v2.y), fminf(fminf(v0.z, v1.z), v2.z)};
  const float mx[3] = {fmaxf(fmaxf(v0.x, v1.x), v2.x), fmaxf(fmaxf(v0.y, v1.y), v2.y), fmaxf(fmaxf(v0.z, v1.z), v2.z)};
  for (int k = 0; k < 3; ++k) {
    c_lo[k] = cell_of(g, k, mn[k], -INFLATE);
    c_hi[k] = cell_of(g, k, mx[k], INFLATE);
  }
}

template <class Each>
__host__ __device__ __forceinline__ void for_face_cells(const Grid &g, const float *verts, const int32_t *faces, int64_t f, Each &&each) {
  int32_t a[3], b[3];
  face_cells(g, load3(verts, faces[3 * f]), load3(verts, faces[3 * f + 1]), load3(verts, faces[3 * f + 2]), a, b);
  for (int32_t z = a[2]; z <= b[2]; ++z)
    for (int32_t y = a[1]; y <= b[1]; ++y)
      for (int32_t x = a[0]; x <= b[0]; ++x) each((z * g.dim[1] + y) * g.dim[0] + x);
}

// The cells ray o + t d, 0 <= t <= tmax, passes through, in the order it meets them: visit(cell) for each, until visit returns
// true or the ray leaves the grid.  A 3-D DDA; see the head of the file for why it is conservative together with face_cells.
template <class Visit>
__host__ __device__ __forceinline__ void walk(const Grid &g, V3 o, V3 d, float tmax, Visit &&visit) {
  AO_STRICT
  const float oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z};
  const float slack = INFLATE * g.cs;
  float t0 = 0.f, t1 = tmax, inv[3];
  for (int k = 0; k < 3; ++k) {  // clip to the box of the grid, grown by the slack
    const float lo = g.lo[k] - slack, hi = g.lo[k] + (float)g.dim[k] * g.cs + slack;
    if (dd[k] != 0.f) {
      inv[k] = 1.f / dd[k];
      const float ta = (lo - oo[k]) * inv[k], tb = (hi - oo[k]) * inv[k];
      t0 = fmaxf(t0, fminf(ta, tb));
      t1 = fminf(t1, fmaxf(ta, tb));
    } else {
      inv[k] = 0.f;
      if (!(oo[k] >= lo && oo[k] <= hi)) return;
    }
  }
  if (!(t0 <= t1)) return;
  int32_t c[3], step[3];
  float tnext[3];
  auto wall = [&](int k) {  // parameter at which the ray leaves cell c[k] along axis k, from the integer index every time
    const float w = __builtin_fmaf((float)(c[k] + (step[k] > 0 ? 1 : 0)), g.cs, g.lo[k]);
    return (w - oo[k]) * inv[k];
  };
  for (int k = 0; k < 3; ++k) {
    c[k] = cell_of(g, k, __builtin_fmaf(t0, dd[k], oo[k]), 0.f);
    step[k] = dd[k] > 0.f ? 1 : -1;
    tnext[k] = dd[k] != 0.f ? wall(k) : INFINITY;
  }
  const int max_steps = g.dim[0] + g.dim[1] + g.dim[2];
  for (int it = 0; it <= max_steps; ++it) {
    if (visit((c[2] * g.dim[1] + c[1]) * g.dim[0] + c[0])) return;
    const int k = (tnext[0] <= tnext[1] && tnext[0] <= tnext[2]) ? 0 : (tnext[1] <= tnext[2] ? 1 : 2);
    if (!(tnext[k] <= t1)) return;
    c[k] += step[k];
    if (c[k] < 0 || c[k] >= g.dim[k]) return;
    tnext[k] = wall(k);
  }
}

// Is ray (o, d) occluded by any face but `own`.  cell_start [n_cells + 1], items: the faces of each cell, in no particular order;
// the answer is an any-hit boolean, so the order does not matter.
__host__ __device__ __forceinline__ bool ray_occluded(const Grid &g, const uint32_t *cell_start, const int32_t *items, const Tri *tri, int32_t own,
                                                      V3 o, V3 d, float bias, float tmax) {
  bool hit = false;
  walk(g, o, d, tmax, [&](int32_t cell) {
    for (uint32_t j = cell_start[cell]; j < cell_start[cell + 1]; ++j) {
      const int32_t f = items[j];
      if (f != own && ray_hits(o, d, tri[f], bias, tmax)) { hit = true; return true; }
    }
    return false;
  });
  return hit;
}

__host__ __device__ __forceinline__ float ao_value(int occluded, int S) { AO_STRICT return 1.f - (float)occluded / (float)S; }

// ---- the margin -----------------------------------------------------------------------------------------------------------

// One margin pixel for texel t: a covered texel keeps its value; an uncovered one with covered texels among its 8 neighbours
// takes their mean, summed in row-major order, and counts as covered for the next pass.
__host__ __device__ __forceinline__ void margin_texel(int t, int H, int W, const float *in_val, const uint8_t *in_mask, float *out_val, uint8_t *out_mask) {
  AO_STRICT
  if (in_mask[t]) { out_val[t] = in_val[t]; out_mask[t] = 1; return; }
  const int y = t / W, x = t % W;
  float sum = 0.f;
  int cnt = 0;
  for (int dy = -1; dy <= 1; ++dy)
    for (int dx = -1; dx <= 1; ++dx) {
      const int yy = y + dy, xx = x + dx;
      if ((dy == 0 && dx == 0) || yy < 0 || yy >= H || xx < 0 || xx >= W || !in_mask[yy * W + xx]) continue;
      sum = sum + in_val[yy * W + xx];
      ++cnt;
    }
  out_val[t] = cnt ? sum / (float)cnt : 0.f;
  out_mask[t] = cnt ? 1 : 0;
}

}  // namespace ao
