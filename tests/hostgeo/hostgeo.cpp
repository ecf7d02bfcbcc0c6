// The geometry-evaluation math of the product (mpmavatar_amd/csrc/geo_math.hpp) compiled for the host
// (tests/test_geo_metrics.py; the stand-in for <hip/hip_runtime.h> is tests/hostmath/stub).  The nearest-neighbour loop is
// the serial statement of what k_nn_d2 computes: the minimum of pair_d2 over all targets, lowest index on ties.
#include "geo_math.hpp"
#include <cstdint>
using namespace geo;

static P3 ld3(const float *p, int64_t i) { return P3{p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }

extern "C" void hg_nn(const float *src, int n_src, const float *dst, int n_dst, float *dist2, int32_t *index) {
  for (int i = 0; i < n_src; ++i) {
    P3 q = ld3(src, i);
    float best = pair_d2(q, ld3(dst, 0));
    int32_t arg = 0;
    for (int j = 1; j < n_dst; ++j) {
      float d = pair_d2(q, ld3(dst, j));
      if (d < best) { best = d; arg = j; }
    }
    dist2[i] = best;
    index[i] = arg;
  }
}

extern "C" void hg_sample_point(const float *v0, const float *v1, const float *v2, const float *u1, const float *u2, int n,
                                float *out) {
  for (int i = 0; i < n; ++i) {
    P3 p = sample_point(ld3(v0, i), ld3(v1, i), ld3(v2, i), u1[i], u2[i]);
    out[3 * i] = p.x; out[3 * i + 1] = p.y; out[3 * i + 2] = p.z;
  }
}

// out = fscore, chamfer, precision, recall, count12, count21 (what k_geo_partial + k_geo_final compute, serially)
extern "C" void hg_metrics(const float *d12, int n1, const float *d21, int n2, double tau, double *out) {
  double sum[2] = {0, 0}, cnt[2] = {0, 0};
  for (int i = 0; i < n1; ++i) { sum[0] += (double)d12[i]; cnt[0] += below(d12[i], tau) ? 1.0 : 0.0; }
  for (int i = 0; i < n2; ++i) { sum[1] += (double)d21[i]; cnt[1] += below(d21[i], tau) ? 1.0 : 0.0; }
  FScore f = fscore_from_counts(cnt[0], n1, cnt[1], n2);
  out[0] = f.fscore; out[1] = chamfer_from_sums(sum[0], n1, sum[1], n2); out[2] = f.precision; out[3] = f.recall;
  out[4] = cnt[0]; out[5] = cnt[1];
}
