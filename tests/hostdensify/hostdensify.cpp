// Densification (mpmavatar_amd/csrc/densify_math.hpp) compiled for the host (tests/test_densify_host.py; the stand-in for
// <hip/hip_runtime.h> is tests/hostmath/stub): serial loops over the per-item functions, one loop per kernel of densify.hip, with
// the same indexing; the atomics are plain adds and the scan is a running sum.
// With -DHOSTDENSIFY_MAIN the file is a stand-alone program for a sanitizer build: synthetic Gaussians on a few faces, every array
// exactly sized, every loop run, also with zero-width rows left out of the table and with n = 0.
#include "densify_math.hpp"

#include <cstdint>

extern "C" void hd_stats_add(int n, const float *grad, const int32_t *radii, const uint8_t *mask, float *accum, float *denom, float *max_radii) {
  for (int i = 0; i < n; ++i) densify::stats_add(i, grad, radii, mask, accum, denom, max_radii);
}

// keep, at [3 n + 1]; counts [8]
extern "C" void hd_plan(int n, int n_faces, const float *scaling, const float *opacity, const int32_t *binding, const float *face_scaling,
                        const float *accum, const float *denom, float max_grad, float dense, float min_opacity, float world, int prune_big,
                        uint32_t *keep, uint32_t *at, int32_t *counts) {
  const densify::Limits lim{max_grad, dense, min_opacity, world, prune_big};
  uint8_t *bits = new uint8_t[n];
  int32_t *face_rows = new int32_t[n_faces](), *face_flagged = new int32_t[n_faces]();
  for (int k = 0; k < densify::N_COUNTS; ++k) counts[k] = 0;
  for (int i = 0; i < n; ++i) {  // k_classify
    const uint8_t b = bits[i] = densify::classify(i, n_faces, scaling, opacity, binding, face_scaling, accum, denom, lim);
    if (b & densify::BAD) { counts[densify::ERROR] |= 1; continue; }
    int32_t rows, flagged;
    densify::face_votes(b, &rows, &flagged);
    face_rows[binding[i]] += rows;
    face_flagged[binding[i]] += flagged;
    counts[densify::N_CLONED] += (b & densify::CLONE) ? 1 : 0;
    counts[densify::N_SPLIT] += (b & densify::SPLIT) ? 1 : 0;
  }
  keep[3 * (int64_t)n] = 0u;
  for (int i = 0; i < n; ++i) {  // k_resolve
    const uint8_t b = bits[i];
    const uint8_t k = (b & densify::BAD) ? 0 : densify::keeps(b, face_rows[binding[i]], face_flagged[binding[i]]);
    keep[i] = (k & densify::KEEP_SELF) ? 1u : 0u;
    keep[(int64_t)n + i] = (k & densify::KEEP_CLONE) ? 1u : 0u;
    keep[2 * (int64_t)n + i] = (k & densify::KEEP_CHILDREN) ? 1u : 0u;
  }
  uint32_t run = 0;
  for (int64_t j = 0; j <= 3 * (int64_t)n; ++j) { at[j] = run; run += keep[j]; }  // the exclusive scan
  const int32_t first = (int32_t)at[2 * (int64_t)n], second = (int32_t)at[3 * (int64_t)n];  // k_counts
  counts[densify::AT_CLONES] = (int32_t)at[n];
  counts[densify::AT_FIRST] = first;
  counts[densify::AT_SECOND] = second;
  counts[densify::N_OUT] = second + (second - first);
  counts[densify::N_PRUNED] = n + counts[densify::N_CLONED] + counts[densify::N_SPLIT] - counts[densify::N_OUT];
  delete[] bits;
  delete[] face_rows;
  delete[] face_flagged;
}

extern "C" void hd_emit(int n, int n_faces, int n_out, const float *xyz, const float *scaling, const float *rotation, const int32_t *binding,
                        const float *face_scaling, const float *noise, const uint32_t *keep, const uint32_t *at, int n_tensors,
                        const float *const *in, float *const *out, const int32_t *widths, const int32_t *modes, int32_t *src, int32_t *kind,
                        int32_t *out_binding, int32_t *counter) {
  for (int f = 0; f < n_faces; ++f) counter[f] = 0;
  const int64_t pairs = (int64_t)at[3 * (int64_t)n] - (int64_t)at[2 * (int64_t)n];
  for (int i = 0; i < n; ++i) {  // k_emit
    const int64_t rows[4] = {keep[i] ? (int64_t)at[i] : -1, keep[(int64_t)n + i] ? (int64_t)at[(int64_t)n + i] : -1,
                             keep[2 * (int64_t)n + i] ? (int64_t)at[2 * (int64_t)n + i] : -1,
                             keep[2 * (int64_t)n + i] ? (int64_t)at[2 * (int64_t)n + i] + pairs : -1};
    const int32_t kinds[4] = {densify::KEPT, densify::CLONED, densify::CHILD, densify::CHILD};
    for (int k = 0; k < 4; ++k) {
      if (rows[k] < 0 || rows[k] >= n_out) continue;
      src[rows[k]] = i;
      kind[rows[k]] = kinds[k];
      out_binding[rows[k]] = binding[i];
      ++counter[binding[i]];
    }
  }
  for (int t = 0; t < n_tensors; ++t)  // k_gather: blockIdx.y = t, a thread per element
    for (int64_t e = 0; e < (int64_t)n_out * widths[t]; ++e) {
      const int64_t row = e / widths[t];
      const int32_t col = (int32_t)(e - row * widths[t]);
      const bool second = row >= (int64_t)at[3 * (int64_t)n];
      out[t][e] = densify::gathered(modes[t], widths[t], src[row], col, kind[row], second, in[t], xyz, scaling, rotation, binding, face_scaling,
                                    noise);
    }
}

extern "C" void hd_reset_opacity(int n, const float *opacity, float *out) {
  for (int i = 0; i < n; ++i) out[i] = densify::reset_opacity(opacity[i]);
}

#ifdef HOSTDENSIFY_MAIN
#include <cmath>
#include <cstdio>
#include <vector>

namespace {

float synth(int i) { return 0.25f + 0.5f * std::sin(0.37f * (float)i + 0.1f); }  // in (-0.25, 0.75)

// n Gaussians on n_faces faces with rows of `rest` floats of _features_rest (0: left out of the table) -> 0, and *n_out
int run(int n, int n_faces, int rest, int prune_big, int *n_out_) {
  std::vector<float> xyz(3 * (size_t)n), scl(3 * (size_t)n), rot(4 * (size_t)n), opa(n), accum(n), denom(n), maxr(n), fs(n_faces), noise(6 * (size_t)n),
      grad(3 * (size_t)n), feat((size_t)rest * n), mom((size_t)rest * n);
  std::vector<int32_t> binding(n), radii(n);
  std::vector<uint8_t> mask(n);
  for (int f = 0; f < n_faces; ++f) fs[f] = 0.03f + 0.04f * synth(f);
  for (int i = 0; i < n; ++i) {
    binding[i] = (i * 7) % n_faces;
    opa[i] = i % 5 == 0 ? -7.f : 6.f * synth(i);
    radii[i] = i % 3;
    mask[i] = radii[i] > 0;
    denom[i] = (float)(i % 4);
    accum[i] = denom[i] * 3e-4f * (0.5f + synth(i + 5));
  }
  for (size_t i = 0; i < xyz.size(); ++i) { xyz[i] = synth((int)i + 3); scl[i] = 3.f * synth((int)i + 9) - 1.5f; grad[i] = 1e-3f * synth((int)i); }
  for (size_t i = 0; i < rot.size(); ++i) rot[i] = synth((int)i + 1) + 0.3f;
  for (size_t i = 0; i < noise.size(); ++i) noise[i] = 2.f * synth((int)i + 2) - 0.5f;
  for (size_t i = 0; i < feat.size(); ++i) { feat[i] = synth((int)i); mom[i] = 1.f + synth((int)i); }
  hd_stats_add(n, grad.data(), radii.data(), nullptr, accum.data(), denom.data(), maxr.data());
  hd_stats_add(n, grad.data(), nullptr, mask.data(), accum.data(), denom.data(), maxr.data());
  std::vector<uint32_t> keep(3 * (size_t)n + 1), at(3 * (size_t)n + 1);
  int32_t counts[densify::N_COUNTS];
  hd_plan(n, n_faces, scl.data(), opa.data(), binding.data(), fs.data(), accum.data(), denom.data(), 2.5e-4f, 0.02f, 0.005f, 0.2f, prune_big,
          keep.data(), at.data(), counts);
  if (counts[densify::ERROR]) return 2;
  const int n_out = *n_out_ = counts[densify::N_OUT];
  if (n_out != n + counts[densify::N_CLONED] + counts[densify::N_SPLIT] - counts[densify::N_PRUNED]) return 3;
  std::vector<float> o_xyz(3 * (size_t)n_out), o_scl(3 * (size_t)n_out), o_rot(4 * (size_t)n_out), o_opa(n_out), o_feat((size_t)rest * n_out),
      o_mom((size_t)rest * n_out);
  std::vector<int32_t> src(n_out), kind(n_out), o_bind(n_out), counter(n_faces);
  std::vector<const float *> in = {xyz.data(), scl.data(), rot.data(), opa.data()};
  std::vector<float *> out = {o_xyz.data(), o_scl.data(), o_rot.data(), o_opa.data()};
  std::vector<int32_t> widths = {3, 3, 4, 1}, modes = {densify::MODE_XYZ, densify::MODE_SCALING, densify::MODE_COPY, densify::MODE_COPY};
  if (rest > 0) {
    in.push_back(feat.data()); out.push_back(o_feat.data()); widths.push_back(rest); modes.push_back(densify::MODE_COPY);
    in.push_back(mom.data()); out.push_back(o_mom.data()); widths.push_back(rest); modes.push_back(densify::MODE_MOMENT);
  }
  hd_emit(n, n_faces, n_out, xyz.data(), scl.data(), rot.data(), binding.data(), fs.data(), noise.data(), keep.data(), at.data(), (int)in.size(),
          in.data(), out.data(), widths.data(), modes.data(), src.data(), kind.data(), o_bind.data(), counter.data());
  int64_t total = 0;
  for (int f = 0; f < n_faces; ++f) {
    total += counter[f];
    bool bound = false;
    for (int i = 0; i < n; ++i) bound = bound || binding[i] == f;
    if (bound && counter[f] < 1) return 4;  // a face never loses its last Gaussian
  }
  if (total != n_out) return 5;
  for (int r = 0; r < n_out; ++r) {
    if (src[r] < 0 || src[r] >= n || o_bind[r] != binding[src[r]]) return 6;
    for (int k = 0; k < 3; ++k) if (!std::isfinite(o_xyz[3 * (size_t)r + k]) || !std::isfinite(o_scl[3 * (size_t)r + k])) return 7;
    for (int k = 0; k < rest; ++k) if (o_mom[(size_t)rest * r + k] != (kind[r] == densify::KEPT ? mom[(size_t)rest * src[r] + k] : 0.f)) return 8;
  }
  std::vector<float> reset(n);
  hd_reset_opacity(n, opa.data(), reset.data());
  for (float v : reset) if (!(v <= -4.59f)) return 9;  // log(0.01 / 0.99) = -4.595
  return 0;
}

}  // namespace

int main() {
  int a = 0, b = 0, c = 0;
  int rc = run(301, 17, 45, 1, &a);
  if (rc) { std::printf("FAILED %d\n", rc); return rc; }
  rc = run(301, 17, 0, 0, &b);
  if (rc) { std::printf("FAILED (R = 0) %d\n", rc); return rc; }
  rc = run(0, 4, 3, 1, &c);
  if (rc || c != 0) { std::printf("FAILED (n = 0) %d\n", rc); return rc ? rc : 20; }
  std::printf("ok: 301 Gaussians on 17 faces -> %d rows; R = 0 -> %d rows; n = 0\n", a, b);
  return 0;
}
#endif
