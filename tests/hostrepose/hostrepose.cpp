// Re-posing (mpmavatar_amd/csrc/repose_math.hpp) compiled for the host (tests/test_repose_host.py; the stand-in for
// <hip/hip_runtime.h> is tests/hostmath/stub): serial loops that mirror the kernels of knn_device.hpp and repose.hip.
//   hr_knn      per slice of knn::plan and per query the register list of k_knn_slices (targets in ascending order, a float compare
//               guarding the insertion), the keys written per (slice, query) as the kernel lays them out, then the merge of k_knn_merge
//   hr_shepard  one (point, joint) at a time, as k_shepard
//   hr_skin     one (frame, point) at a time over rp::blend and rp::to_pose / rp::to_tpose, as k_skin
// With -DHOSTREPOSE_MAIN the file is a stand-alone program for a sanitizer build: synthetic values on exactly sized arrays through
// every loop, N = 0 and P = 0 included.
#include "repose_math.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace {

template <int D, int KP>
void knn_dk(int n, int m, int k, const knn::Plan &p, const float *q, const float *t, float *dists, int32_t *idx) {
  std::vector<uint64_t> keys((size_t)p.slices * n * k);
  for (int s = 0; s < p.slices; ++s) {
    const int j0 = (int)std::min((int64_t)s * p.slice_len, (int64_t)m), j1 = (int)std::min((int64_t)j0 + p.slice_len, (int64_t)m);
    for (int i = 0; i < n; ++i) {
      knn::Nearest<KP> best;
      best.fill(INFINITY, j0 < m ? j0 : 0);
      for (int j = j0; j < j1; ++j) {
        const float d2 = knn::dist2<D>(q + (size_t)i * D, t + (size_t)j * D);
        if (d2 < best.worst()) best.insert(d2, j);
      }
      for (int c = 0; c < k; ++c) keys[((size_t)s * n + i) * k + c] = knn::key(best.d[c], best.j[c]);
    }
  }
  for (int i = 0; i < n; ++i) {
    knn::List<uint64_t, KP> best;
    best.fill(~0ull);
    for (int s = 0; s < p.slices; ++s)
      for (int c = 0; c < k; ++c) {
        const uint64_t x = keys[((size_t)s * n + i) * k + c];
        if (x < best.worst()) best.insert(x);
      }
    for (int c = 0; c < k; ++c) {
      dists[(size_t)i * k + c] = knn::key_dist(best.v[c]);
      idx[(size_t)i * k + c] = knn::key_index(best.v[c]);
    }
  }
}

}  // namespace

// -> 0, or -1 for the arguments mpmhip_knn refuses; *out_slices (may be NULL) = the number of slices used
extern "C" int hr_knn(int n, int m, int dim, int k, int slices, const float *q, const float *t, float *dists, int32_t *idx, int32_t *out_slices) {
  if (n < 0 || m < 1 || (dim != 3 && dim != 6) || k < 1 || k > knn::MAX_K || k > m || slices < 0) return -1;
  const knn::Plan p = knn::plan(n, m, slices);
  if (out_slices) *out_slices = p.slices;
  if (n == 0) return 0;
  const int kp = knn::padded_k(k);
  if (dim == 3) {
    if (kp == 4) knn_dk<3, 4>(n, m, k, p, q, t, dists, idx);
    else if (kp == 8) knn_dk<3, 8>(n, m, k, p, q, t, dists, idx);
    else knn_dk<3, 16>(n, m, k, p, q, t, dists, idx);
  } else {
    if (kp == 4) knn_dk<6, 4>(n, m, k, p, q, t, dists, idx);
    else if (kp == 8) knn_dk<6, 8>(n, m, k, p, q, t, dists, idx);
    else knn_dk<6, 16>(n, m, k, p, q, t, dists, idx);
  }
  return 0;
}

// lbs == NULL: out [n * k] = the weights themselves
extern "C" void hr_shepard(int n, int k, int power, const float *d2, const int32_t *idx, const float *lbs, int n_verts, int n_joints, float *out) {
  const int cols = lbs ? n_joints : k;
  for (int p = 0; p < n; ++p)
    for (int j = 0; j < cols; ++j) {
      float w[knn::MAX_K];
      rp::shepard_weights(d2 + (size_t)p * k, k, power, w);
      out[(size_t)p * cols + j] = lbs ? rp::shepard_entry(w, idx + (size_t)p * k, k, lbs, n_verts, n_joints, j) : w[j];
    }
}

extern "C" void hr_skin(int inverse, int n_frames, int n_points, int n_joints, const float *verts, int vb, const float *W, int wb, const float *A,
                        const float *transl, const float *scale, int sb, float *out, float *out_T) {
  for (int b = 0; b < n_frames; ++b)
    for (int p = 0; p < n_points; ++p) {
      float T[16], Ti[16], o[3];
      rp::blend(W + ((size_t)(wb ? b : 0) * n_points + p) * n_joints, n_joints, A + (size_t)b * n_joints * 16, T);
      const float *v = verts + ((size_t)(vb ? b : 0) * n_points + p) * 3;
      const float *tr = transl ? transl + 3 * (size_t)b : nullptr;
      const float *sc = scale ? scale + (sb ? b : 0) : nullptr;
      const size_t row = (size_t)b * n_points + p;
      if (inverse) rp::to_tpose(T, v, tr, sc, Ti, o);
      else rp::to_pose(T, v, tr, sc, o);
      if (out_T)
        for (int e = 0; e < 16; ++e) out_T[row * 16 + e] = inverse ? Ti[e] : T[e];
      for (int c = 0; c < 3; ++c) out[row * 3 + c] = o[c];
    }
}

#ifdef HOSTREPOSE_MAIN
#include <cstdio>

namespace {

float synth(int i) { return 0.25f + 0.5f * std::sin(0.37f * (float)i + 0.1f); }

int run_knn(int n, int m, int dim, int k, int slices) {
  std::vector<float> q((size_t)n * dim), t((size_t)m * dim), dists((size_t)n * k);
  std::vector<int32_t> idx((size_t)n * k);
  for (size_t i = 0; i < q.size(); ++i) q[i] = synth((int)i + 3);
  for (size_t i = 0; i < t.size(); ++i) t[i] = synth(5 * (int)i + 1);
  int32_t used = 0;
  if (hr_knn(n, m, dim, k, slices, q.data(), t.data(), dists.data(), idx.data(), &used)) return 1;
  if (used < 1 || used > m) return 2;
  for (int i = 0; i < n; ++i)
    for (int c = 0; c < k; ++c) {
      const int32_t j = idx[(size_t)i * k + c];
      if (j < 0 || j >= m) return 3;
      if (c > 0 && !(dists[(size_t)i * k + c - 1] <= dists[(size_t)i * k + c])) return 4;
    }
  return 0;
}

int run_skin(int B, int P, int J, int K, int V) {
  std::vector<float> lbs((size_t)V * J), d2((size_t)P * K), W((size_t)P * J), Wb((size_t)B * P * J), A((size_t)B * J * 16), verts((size_t)B * P * 3),
      transl((size_t)B * 3), scale(B), out((size_t)B * P * 3), T((size_t)B * P * 16), wk((size_t)P * K);
  std::vector<int32_t> idx((size_t)P * K);
  for (size_t i = 0; i < lbs.size(); ++i) lbs[i] = synth((int)i) / (float)J;
  for (size_t i = 0; i < d2.size(); ++i) { d2[i] = 0.01f * synth((int)i) * (float)(i % K); idx[i] = (int32_t)((7 * i) % V); }
  for (size_t i = 0; i < A.size(); ++i) A[i] = (i % 16) % 5 == 0 ? 1.f + 0.1f * synth((int)i) : 0.2f * synth((int)i) - 0.1f;  // near the identity
  for (size_t i = 0; i < verts.size(); ++i) verts[i] = synth((int)i + 11);
  for (size_t i = 0; i < transl.size(); ++i) transl[i] = synth((int)i + 2);
  for (int b = 0; b < B; ++b) scale[b] = 1.f + 0.1f * (float)b;
  hr_shepard(P, K, 2, d2.data(), idx.data(), lbs.data(), V, J, W.data());
  hr_shepard(P, K, 1, d2.data(), nullptr, nullptr, 0, 0, wk.data());
  for (int b = 0; b < B; ++b)
    for (size_t i = 0; i < W.size(); ++i) Wb[(size_t)b * W.size() + i] = W[i];
  for (int inverse = 0; inverse < 2; ++inverse) {
    hr_skin(inverse, B, P, J, verts.data(), 1, W.data(), 0, A.data(), transl.data(), scale.data(), 1, out.data(), T.data());
    for (float v : out) if (!std::isfinite(v)) return 5;
    for (float v : T) if (!std::isfinite(v)) return 6;
    hr_skin(inverse, B, P, J, verts.data(), 0, Wb.data(), 1, A.data(), nullptr, scale.data(), 0, out.data(), nullptr);
    hr_skin(inverse, B, P, J, verts.data(), 0, Wb.data(), 1, A.data(), nullptr, nullptr, 0, out.data(), nullptr);
    for (float v : out) if (!std::isfinite(v)) return 7;
  }
  for (int p = 0; p < P; ++p) {
    float s = 0.f;
    for (int c = 0; c < K; ++c) s += wk[(size_t)p * K + c];
    if (std::fabs(s - 1.f) > 1e-5f) return 8;
  }
  return 0;
}

}  // namespace

int main() {
  const int knn_runs[][5] = {{301, 777, 3, 10, 0}, {301, 777, 6, 10, 4}, {77, 2100, 6, 16, 1}, {5, 16, 3, 16, 0}, {3, 31, 3, 1, 31},
                             {9, 31, 6, 5, 0},     {0, 31, 3, 4, 0},     {1, 1, 3, 1, 0}};
  for (const auto &r : knn_runs)
    if (int rc = run_knn(r[0], r[1], r[2], r[3], r[4])) { std::printf("FAILED (knn %d x %d) %d\n", r[0], r[1], rc); return rc; }
  float one = 0.f;
  int32_t j = 0;
  if (hr_knn(1, 3, 3, 4, 0, &one, &one, &one, &j, nullptr) != -1 || hr_knn(1, 3, 4, 1, 0, &one, &one, &one, &j, nullptr) != -1) {
    std::printf("FAILED (bad arguments accepted)\n");
    return 9;
  }
  const int skin_runs[][5] = {{5, 257, 55, 10, 300}, {1, 1, 3, 1, 2}, {3, 0, 55, 10, 300}, {0, 17, 3, 4, 9}};
  for (const auto &r : skin_runs)
    if (int rc = run_skin(r[0], r[1], r[2], r[3], r[4])) { std::printf("FAILED (skin B = %d, P = %d) %d\n", r[0], r[1], rc); return rc; }
  std::printf("ok: 8 searches (N = 0 included), 4 skinning runs (P = 0 and B = 0 included)\n");
  return 0;
}
#endif
