// densify_math.hpp -- densification of the bound Gaussians (scene/gaussian_model.py:378-526, train_appearance.py:245-257), per
// work item: the statistics of every iteration, the decisions of densify_and_prune and the arithmetic of a split child.
//   stats     for rows with radii > 0:  accum += sqrt(gx^2 + gy^2), denom += 1, max_radii2D = max(max_radii2D, radii)
//   g_i       accum / denom, NaN -> 0;  gs_i = exp(_scaling[i]) * face_scaling[binding[i]], the world scale
//   clone     g_i >= max_grad and max(gs_i) <= dense         (dense = percent_dense * extent)
//   split     g_i >= max_grad and max(gs_i) >  dense: two children, the source leaves
//             child c:  xyz = R(q / |q|) (gs_i * noise[i, c]) + _xyz[i],  _scaling = log((gs_i / face_scaling) / 1.6)
//   prune     over the enlarged set: sigmoid(_opacity) < min_opacity, or (with a screen size given) max(world scale) > world
//             (world = 0.1 * extent); a face all of whose Gaussians are flagged keeps them all (prune_points :379-385)
// One pass over the originals decides everything, because an original yields at most itself, one clone (its copy, so flagged
// exactly when the original is) and two children (equal to each other in opacity and scale, so flagged together): classify() gives
// the bits of row i, a face then counts its rows and its flagged rows with integer adds, and keeps() turns bits and the face's two
// counts into what row i leaves behind.  The split's own prune_points never meets the face rule: a face that loses s sources has
// just gained 2 s children.
// Plain C++ for the device (densify.hip) and the host (tests/hostdensify/) alike.  All arithmetic is fp32 and every comparison is an
// fp32 comparison against a threshold rounded to fp32, as torch takes them.
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

namespace densify {

constexpr uint8_t CLONE = 1, SPLIT = 2, FLAG_SELF = 4, FLAG_CHILD = 8, BAD = 16;   // the bits of classify()
constexpr int32_t KEPT = 0, CLONED = 1, CHILD = 2;                                 // `kind` of an output row
constexpr uint8_t KEEP_SELF = 1, KEEP_CLONE = 2, KEEP_CHILDREN = 4;                // the bits of keeps()
// modes of a row-aligned tensor in the gather: copied for every row; copied for kept rows and zero for new ones (Adam moments);
// _xyz and _scaling, which a split child computes
constexpr int32_t MODE_COPY = 0, MODE_MOMENT = 1, MODE_XYZ = 2, MODE_SCALING = 3;
// out_counts of the plan
constexpr int N_OUT = 0, N_CLONED = 1, N_SPLIT = 2, N_PRUNED = 3, ERROR = 4, AT_CLONES = 5, AT_FIRST = 6, AT_SECOND = 7, N_COUNTS = 8;

struct Limits {
  float max_grad, dense, min_opacity, world;
  int32_t prune_big;  // a screen size was given: the world-size test is on (the reference's screen-size test itself is dead)
};

__host__ __device__ __forceinline__ float sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

__host__ __device__ __forceinline__ float max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

// train_appearance.py:248 and add_densification_stats; exactly one of radii / mask is given, a set byte of mask counts as radius 1
__host__ __device__ __forceinline__ void stats_add(int64_t i, const float *grad, const int32_t *radii, const uint8_t *mask, float *accum,
                                                   float *denom, float *max_radii) {
#pragma clang fp contract(off)
  const int32_t r = radii ? radii[i] : (int32_t)(mask[i] != 0);
  if (r <= 0) return;
  const float gx = grad[3 * i], gy = grad[3 * i + 1];
  accum[i] += sqrtf(gx * gx + gy * gy);
  denom[i] += 1.f;
  max_radii[i] = fmaxf(max_radii[i], (float)r);
}

struct World {
  float x, y, z;
};

__host__ __device__ __forceinline__ World world_scale(const float *scaling, int64_t i, float fs) {
#pragma clang fp contract(off)
  return World{expf(scaling[3 * i]) * fs, expf(scaling[3 * i + 1]) * fs, expf(scaling[3 * i + 2]) * fs};
}

// log((gs / face_scaling) / (0.8 N)), N = 2
__host__ __device__ __forceinline__ float child_scaling(float gs, float fs) {
#pragma clang fp contract(off)
  return logf((gs / fs) / 1.6f);
}

// the bits of row i; BAD alone for a binding outside [0, n_faces), which reads nothing
__host__ __device__ __forceinline__ uint8_t classify(int64_t i, int32_t n_faces, const float *scaling, const float *opacity,
                                                     const int32_t *binding, const float *face_scaling, const float *accum,
                                                     const float *denom, const Limits &l) {
#pragma clang fp contract(off)
  const int32_t f = binding[i];
  if (f < 0 || f >= n_faces) return BAD;
  const float fs = face_scaling[f];
  float g = accum[i] / denom[i];
  if (g != g) g = 0.f;
  const World gs = world_scale(scaling, i, fs);
  const float m = max3(gs.x, gs.y, gs.z);
  uint8_t bits = 0;
  if (g >= l.max_grad) bits |= m > l.dense ? SPLIT : CLONE;
  const bool faint = sigmoid(opacity[i]) < l.min_opacity;
  if (faint || (l.prune_big && m > l.world)) bits |= FLAG_SELF;
  if (bits & SPLIT) {
    const float mc = max3(expf(child_scaling(gs.x, fs)) * fs, expf(child_scaling(gs.y, fs)) * fs, expf(child_scaling(gs.z, fs)) * fs);
    if (faint || (l.prune_big && mc > l.world)) bits |= FLAG_CHILD;
  }
  return bits;
}

// what row i adds to its face's count of rows and of flagged rows in the enlarged set
__host__ __device__ __forceinline__ void face_votes(uint8_t bits, int32_t *rows, int32_t *flagged) {
  const int self = (bits & SPLIT) ? 0 : 1, clone = (bits & CLONE) ? 1 : 0, children = (bits & SPLIT) ? 2 : 0;
  *rows = self + clone + children;
  *flagged = ((bits & FLAG_SELF) ? self + clone : 0) + ((bits & FLAG_CHILD) ? children : 0);
}

// the face rule: flagged rows leave only if the face keeps at least one row
__host__ __device__ __forceinline__ uint8_t keeps(uint8_t bits, int32_t face_rows, int32_t face_flagged) {
  if (bits & BAD) return 0;
  const bool prune = face_rows - face_flagged > 0;
  const bool self_goes = (bits & FLAG_SELF) && prune, children_go = (bits & FLAG_CHILD) && prune;
  uint8_t k = 0;
  if (!(bits & SPLIT) && !self_goes) k |= KEEP_SELF;
  if ((bits & CLONE) && !self_goes) k |= KEEP_CLONE;
  if ((bits & SPLIT) && !children_go) k |= KEEP_CHILDREN;
  return k;
}

struct Child {
  float xyz[3], scaling[3];
};

// child c of source i (densify_and_split :462-470, build_rotation of utils/general_utils.py:116-137); noise [n, 2, 3].  The sample
// gs * noise is in world scale and is added to the local _xyz: the reference's mix, kept as it stands.
__host__ __device__ __forceinline__ Child child(int64_t i, int c, const float *xyz, const float *scaling, const float *rotation,
                                                const int32_t *binding, const float *face_scaling, const float *noise) {
#pragma clang fp contract(off)
  const float fs = face_scaling[binding[i]];
  const World gs = world_scale(scaling, i, fs);
  const float *z = noise + (2 * i + c) * 3;
  const float s0 = gs.x * z[0], s1 = gs.y * z[1], s2 = gs.z * z[2];
  const float *q = rotation + 4 * i;
  const float norm = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const float r = q[0] / norm, x = q[1] / norm, y = q[2] / norm, w = q[3] / norm;
  Child o;
  o.xyz[0] = ((1.f - 2.f * (y * y + w * w)) * s0 + (2.f * (x * y - r * w)) * s1 + (2.f * (x * w + r * y)) * s2) + xyz[3 * i];
  o.xyz[1] = ((2.f * (x * y + r * w)) * s0 + (1.f - 2.f * (x * x + w * w)) * s1 + (2.f * (y * w - r * x)) * s2) + xyz[3 * i + 1];
  o.xyz[2] = ((2.f * (x * w - r * y)) * s0 + (2.f * (y * w + r * x)) * s1 + (1.f - 2.f * (x * x + y * y)) * s2) + xyz[3 * i + 2];
  o.scaling[0] = child_scaling(gs.x, fs);
  o.scaling[1] = child_scaling(gs.y, fs);
  o.scaling[2] = child_scaling(gs.z, fs);
  return o;
}

// element `col` of output row `row` of a tensor of the given mode and width, whose source row is i; second: the row is a second child
__host__ __device__ __forceinline__ float gathered(int32_t mode, int32_t width, int64_t i, int32_t col, int32_t kind, bool second,
                                                   const float *in, const float *xyz, const float *scaling, const float *rotation,
                                                   const int32_t *binding, const float *face_scaling, const float *noise) {
  if (kind == CHILD && (mode == MODE_XYZ || mode == MODE_SCALING)) {
    const Child ch = child(i, second ? 1 : 0, xyz, scaling, rotation, binding, face_scaling, noise);
    return mode == MODE_XYZ ? ch.xyz[col] : ch.scaling[col];
  }
  if (mode == MODE_MOMENT && kind != KEPT) return 0.f;
  return in[i * width + col];
}

// reset_opacity (:284-287): inverse_sigmoid(min(sigmoid(x), 0.01))
__host__ __device__ __forceinline__ float reset_opacity(float x) {
#pragma clang fp contract(off)
  const float s = fminf(sigmoid(x), 0.01f);
  return logf(s / (1.f - s));
}

}  // namespace densify
