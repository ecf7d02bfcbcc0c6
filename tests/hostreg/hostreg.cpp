// The regularisation terms (mpmavatar_amd/csrc/reg_math.hpp) compiled for the host (tests/test_reg_host.py; the stand-in for
// <hip/hip_runtime.h> is tests/hostmath/stub): serial loops over the per-item functions, one loop per kernel of reg.hip, with the
// same stencil indexing; the sums are plain double sums in index order.
// With -DHOSTREG_MAIN the file is a stand-alone program for a sanitizer build: it reads a mesh's index structure (faces, neighbours)
// from a file, builds the stencil table, fills in synthetic values and runs every loop, and also F = 0 and n = 0.
#include "reg_math.hpp"

#include <cstdint>

extern "C" void hr_mesh_forward(int n_f, int n_v, const float *verts, const int32_t *faces, const int32_t *nb, const float *nd, const float *nw,
                                float *terms, float *stats, float *sq_dist) {
  if (n_f == 0) return;
  double s[3] = {0.0, 0.0, 0.0};
  float *area = new float[n_f];
  for (int f = 0; f < n_f; ++f) {
    const reg::FaceTerms t = reg::face_forward(f, n_f, n_v, verts, faces, nb, nd, nw, sq_dist);
    area[f] = t.area;
    s[0] += (double)t.normal; s[1] += (double)t.iso; s[2] += (double)t.area;
  }
  const float mean = (float)(s[2] / (double)n_f);
  double w[2] = {0.0, 0.0};
  for (int f = 0; f < n_f; ++f) {
    const float d = area[f] - mean;
    w[0] += (double)fabsf(d);
    w[1] += (double)reg::sign(d);
  }
  delete[] area;
  terms[0] = (float)(s[0] / (double)n_f);
  terms[1] = (float)(s[1] / ((double)n_f * reg::K));
  terms[2] = (float)(w[0] / (double)n_f);
  stats[0] = mean;
  stats[1] = (float)(w[1] / (double)n_f);
}

extern "C" void hr_mesh_backward(int n_f, int n_v, const float *verts, const int32_t *faces, const int32_t *nb, const float *nd, const float *nw,
                                 const float *stats, const float *g, const int32_t *vert_start, const int32_t *vert_items, float *d_stencil,
                                 float *d_verts) {
  if (!d_verts) return;
  for (int f = 0; f < n_f; ++f) reg::face_backward(f, n_f, n_v, verts, faces, nb, nd, nw, stats, g, d_stencil);
  for (int v = 0; v < n_v; ++v) fgrad::vertex_gather(v, vert_start, vert_items, d_stencil, d_verts);
}

extern "C" void hr_gauss_forward(int n, const float *opacity, const float *xyz, const float *scaling, const int32_t *radii, const uint8_t *mask,
                                 float t_xyz, float t_scale, float *terms, int32_t *n_visible) {
  if (n == 0) return;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = 0; i < n; ++i) {
    const reg::GaussTerms t = reg::gauss_forward(i, opacity, xyz, scaling, radii, mask, t_xyz, t_scale);
    s[0] += (double)t.opacity; s[1] += (double)t.xyz; s[2] += (double)t.scale; s[3] += t.visible ? 1.0 : 0.0;
  }
  terms[0] = (float)(s[0] / (double)n);
  terms[1] = (float)(s[1] / s[3]);
  terms[2] = (float)(s[2] / s[3]);
  n_visible[0] = (int32_t)s[3];
}

extern "C" void hr_gauss_backward(int n, const float *opacity, const float *xyz, const float *scaling, const int32_t *radii, const uint8_t *mask,
                                  float t_xyz, float t_scale, const int32_t *n_visible, const float *g, float *d_opacity, float *d_xyz,
                                  float *d_scaling) {
  for (int i = 0; i < n; ++i)
    reg::gauss_backward(i, n, opacity, xyz, scaling, radii, mask, t_xyz, t_scale, n_visible, g, d_opacity, d_xyz, d_scaling);
}

#ifdef HOSTREG_MAIN
#include <cmath>
#include <cstdio>
#include <vector>

namespace {

float synth(int i) { return 0.25f + 0.5f * std::sin(0.37f * (float)i + 0.1f); }

int run_mesh(int n_v, const std::vector<int32_t> &faces, const std::vector<int32_t> &nb, int *self_slots) {
  const int n_f = (int)faces.size() / 3;
  // the stencil table: S[f, s, c] = faces[nbx[f, s], c], a stable counting sort by vertex
  std::vector<int32_t> key((size_t)n_f * reg::STENCIL * 3), start((size_t)n_v + 1, 0), items(key.size());
  *self_slots = 0;
  for (int f = 0; f < n_f; ++f)
    for (int s = 0; s < reg::STENCIL; ++s) {
      const int32_t j = s == 0 ? f : nb[(size_t)reg::K * f + s - 1];
      *self_slots += s > 0 && j == f;
      for (int c = 0; c < 3; ++c) key[((size_t)f * reg::STENCIL + s) * 3 + c] = faces[3 * (size_t)j + c];
    }
  for (int32_t k : key) ++start[k + 1];
  for (int v = 0; v < n_v; ++v) start[v + 1] += start[v];
  std::vector<int32_t> at(start.begin(), start.end() - 1);
  for (size_t i = 0; i < key.size(); ++i) items[at[key[i]]++] = (int32_t)i;
  // exactly sized arrays: an access past a row is the sanitizer's to report
  std::vector<float> verts(3 * (size_t)n_v), nd((size_t)n_f * reg::K), nw(nd.size()), sq(nd.size()), d_stencil((size_t)n_f * reg::ROW),
      d_verts(3 * (size_t)n_v);
  for (size_t i = 0; i < verts.size(); ++i) verts[i] = 0.3f * synth((int)i) + 0.05f * (float)(i % 7);
  float terms[3] = {0.f, 0.f, 0.f}, stats[2] = {0.f, 0.f};
  const float g[3] = {0.1f, 20.f, 1000.f};
  hr_mesh_forward(n_f, n_v, verts.data(), faces.data(), nb.data(), nd.data(), nw.data(), terms, stats, sq.data());
  for (size_t i = 0; i < sq.size(); ++i) { nd[i] = std::sqrt(sq[i]) * (0.8f + 0.4f * synth((int)i)); nw[i] = std::exp(-2.f * sq[i]); }
  hr_mesh_forward(n_f, n_v, verts.data(), faces.data(), nb.data(), nd.data(), nw.data(), terms, stats, nullptr);
  hr_mesh_backward(n_f, n_v, verts.data(), faces.data(), nb.data(), nd.data(), nw.data(), stats, g, start.data(), items.data(), d_stencil.data(),
                   d_verts.data());
  if (n_f == 0) {
    for (float v : d_verts) if (v != 0.f) return 2;
    return 0;
  }
  for (int k = 0; k < 3; ++k) if (!std::isfinite(terms[k])) return 3;
  for (float v : d_verts) if (!std::isfinite(v)) return 4;
  for (int f = 0; f < n_f; ++f)
    for (int k = 0; k < reg::K; ++k)
      if (nb[(size_t)reg::K * f + k] == f)
        for (int i = 0; i < 9; ++i) if (d_stencil[(size_t)reg::ROW * f + 9 * (1 + k) + i] != 0.f) return 5;
  return 0;
}

int run_gauss(int n) {
  std::vector<float> opa(n), xyz(3 * (size_t)n), scl(3 * (size_t)n), d_opa(n), d_xyz(xyz.size()), d_scl(scl.size());
  std::vector<int32_t> radii(n);
  std::vector<uint8_t> mask(n);
  for (int i = 0; i < n; ++i) { opa[i] = 4.f * synth(i) - 2.f; radii[i] = i % 4; mask[i] = radii[i] > 0; }
  for (size_t i = 0; i < xyz.size(); ++i) { xyz[i] = 3.f * synth((int)i + 3) - 1.5f; scl[i] = 2.f * synth((int)i + 9) - 1.9f; }
  float terms[3] = {0.f, 0.f, 0.f}, again[3] = {0.f, 0.f, 0.f};
  int32_t n_vis = -1, n_vis2 = -1;
  const float g[3] = {0.05f, 1.f, 1.f};
  hr_gauss_forward(n, opa.data(), xyz.data(), scl.data(), radii.data(), nullptr, 1.0f, 0.6f, terms, &n_vis);
  hr_gauss_forward(n, opa.data(), xyz.data(), scl.data(), nullptr, mask.data(), 1.0f, 0.6f, again, &n_vis2);
  if (n == 0) return 0;
  if (n_vis != n_vis2 || terms[1] != again[1] || terms[2] != again[2]) return 6;
  hr_gauss_backward(n, opa.data(), xyz.data(), scl.data(), radii.data(), nullptr, 1.0f, 0.6f, &n_vis, g, d_opa.data(), d_xyz.data(), d_scl.data());
  hr_gauss_backward(n, opa.data(), xyz.data(), scl.data(), nullptr, mask.data(), 1.0f, 0.6f, &n_vis, g, nullptr, d_xyz.data(), nullptr);
  for (int i = 0; i < n; ++i)
    if (radii[i] == 0)
      for (int c = 0; c < 3; ++c) if (d_xyz[3 * (size_t)i + c] != 0.f || d_scl[3 * (size_t)i + c] != 0.f) return 7;
  for (float v : d_opa) if (!std::isfinite(v) || v == 0.f) return 8;
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  int n_v = 4;
  std::vector<int32_t> faces = {0, 1, 2, 0, 2, 3}, nb = {1, 0, 0, 0, 1, 1};  // two triangles sharing an edge
  if (argc > 1) {  // int32: n_v, n_f; then int32 faces [3 n_f]; then int32 neighbours [3 n_f]
    FILE *fp = std::fopen(argv[1], "rb");
    if (!fp) return 10;
    int32_t hdr[2];
    if (std::fread(hdr, 4, 2, fp) != 2) return 11;
    n_v = hdr[0];
    faces.resize(3 * (size_t)hdr[1]);
    nb.resize(3 * (size_t)hdr[1]);
    if (std::fread(faces.data(), 4, faces.size(), fp) != faces.size()) return 12;
    if (std::fread(nb.data(), 4, nb.size(), fp) != nb.size()) return 13;
    std::fclose(fp);
  }
  int self_slots = 0, none = 0;
  int rc = run_mesh(n_v, faces, nb, &self_slots);
  if (rc) { std::printf("FAILED %d\n", rc); return rc; }
  rc = run_mesh(n_v, std::vector<int32_t>(), std::vector<int32_t>(), &none);  // F = 0
  if (rc) { std::printf("FAILED (F = 0) %d\n", rc); return rc; }
  rc = run_gauss(301);
  if (rc) { std::printf("FAILED (Gaussians) %d\n", rc); return rc; }
  rc = run_gauss(0);
  if (rc) { std::printf("FAILED (n = 0) %d\n", rc); return rc; }
  std::printf("ok: %d faces, %d vertices, %d self slots; F = 0; 301 Gaussians; n = 0\n", (int)faces.size() / 3, n_v, self_slots);
  return 0;
}
#endif
