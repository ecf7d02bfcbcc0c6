// geo_math.hpp -- the three pieces of the geometry evaluation (/root/reference/metric.py) whose numerics the tests pin.
// Plain C++ for the device and the host alike: tests/hostgeo/ compiles it with g++ over the stand-in for
// <hip/hip_runtime.h>, the way tests/hostmath/ compiles mpm_math.hpp.
//
// What is pinned against what: pair_d2 and the two finalisers against the reference's own functions (SciPy's cKDTree and
// metric.py:31-41, tests/golden/geo_metrics.npz).  sample_point restates trimesh.sample.sample_surface, which metric.py:5
// calls; trimesh is not installed where the fixtures are made, so NOTHING here is pinned against trimesh itself -- only
// against a float64 restatement of the same construction.
#pragma once
#include <hip/hip_runtime.h>

namespace geo {

struct P3 {
  float x, y, z;
};

// |a - b|^2 in the direct form: three differences, then dx*dx + dy*dy + dz*dz with the two sums contracted into FMAs
// (written out, so that every caller -- the packed inner loop of k_nn_d2, its index search, the host build -- rounds
// alike).  At most 8 roundings of 2^-24 relative, none of them absolute in |a|^2: the expanded form
// |a|^2 + |b|^2 - 2 a.b loses ~3e-4 relative at d2 ~ 1e-3 on unit-sized meshes, enough to move points across the
// F-score threshold, which is why the dot products do not go through MFMA.
__host__ __device__ __forceinline__ float pair_d2(P3 a, P3 b) {
  float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
  return __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
}

// trimesh's uniform point on a triangle: (u1, u2) in the unit square, the half beyond the diagonal folded back
// (both become |u - 1|), point = v0 + u1 (v1 - v0) + u2 (v2 - v0).  The fold is decided on the exact sum (two floats
// add exactly in double), as trimesh decides it in float64.
__host__ __device__ __forceinline__ P3 sample_point(P3 v0, P3 v1, P3 v2, float u1, float u2) {
  if ((double)u1 + (double)u2 > 1.0) {
    u1 = __builtin_fabsf(u1 - 1.0f);
    u2 = __builtin_fabsf(u2 - 1.0f);
  }
  P3 e1{v1.x - v0.x, v1.y - v0.y, v1.z - v0.z}, e2{v2.x - v0.x, v2.y - v0.y, v2.z - v0.z};
  return P3{v0.x + u1 * e1.x + u2 * e2.x, v0.y + u1 * e1.y + u2 * e2.y, v0.z + u1 * e1.z + u2 * e2.z};
}

// 0.5 |e1 x e2|
__host__ __device__ __forceinline__ float face_area(P3 v0, P3 v1, P3 v2) {
  P3 a{v1.x - v0.x, v1.y - v0.y, v1.z - v0.z}, b{v2.x - v0.x, v2.y - v0.y, v2.z - v0.z};
  float cx = a.y * b.z - a.z * b.y, cy = a.z * b.x - a.x * b.z, cz = a.x * b.y - a.y * b.x;
  return 0.5f * __builtin_sqrtf(cx * cx + cy * cy + cz * cz);
}

// metric.py:34-35, the reference's quirk kept: percent_below compares the SQUARED distance with the threshold
// (dists**2 <= thresh), so tau = 1e-3 is a distance of 0.0316, not 0.001.
__host__ __device__ __forceinline__ bool below(float d2, double tau) { return (double)d2 <= tau; }

struct FScore {
  double fscore, precision, recall;
};
// metric.py:34-41: precision / recall = count / n * 100, F = 2 P R / (P + R + 1e-9)
__host__ __device__ __forceinline__ FScore fscore_from_counts(double count12, double n1, double count21, double n2) {
  double p = count12 / n1 * 100.0, r = count21 / n2 * 100.0;
  return FScore{2.0 * p * r / (p + r + 1e-9), p, r};
}

// metric.py:31: 1000 (mean d12^2 + mean d21^2)
__host__ __device__ __forceinline__ double chamfer_from_sums(double sum12, double n1, double sum21, double n2) {
  return 1000.0 * (sum12 / n1 + sum21 / n2);
}

}  // namespace geo
