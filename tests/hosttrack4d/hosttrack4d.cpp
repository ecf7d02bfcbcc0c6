// The Laplacian and scale-ratio terms (mpmavatar_amd/csrc/track4d_math.hpp) compiled for the host (tests/test_track4d_host.py; the
// stand-in for <hip/hip_runtime.h> is tests/hostmath/stub): serial loops over the per-item functions, one loop per kernel of
// track4d.hip; the sums are plain double sums in index order, the variance from the sums of q and q^2 as k_scale_finish takes it.
// With -DHOSTTRACK4D_MAIN the file is a stand-alone program for a sanitizer build: it reads a mesh's faces from a file, builds the
// adjacency and the corner table, fills in synthetic values and runs every loop.
#include "track4d_math.hpp"

#include <cstdint>

extern "C" void h4_laplacian_forward(int n_v, const float *verts, const int32_t *start, const int32_t *nbr, float *lv, float *value) {
  double s = 0.0;
  for (int i = 0; i < n_v; ++i) {
    float norm;
    const trk::V3 l = trk4::laplacian_row(i, n_v, verts, start, nbr, norm);
    if (lv) trk::st3(lv, i, l);
    s += (double)norm;
  }
  if (value) value[0] = (float)(s / (double)n_v);
}

extern "C" void h4_laplacian_backward(int n_v, const float *lv, const int32_t *start, const int32_t *nbr, const float *g, float *d_verts) {
  for (int j = 0; j < n_v; ++j) trk4::laplacian_backward(j, n_v, lv, start, nbr, g, d_verts);
}

extern "C" void h4_scale_forward(int n_f, int n_v, const float *verts, const int32_t *faces, const float *scales, float th_ratio, float th_edge,
                                 float *terms) {
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int f = 0; f < n_f; ++f) {
    const trk4::ScaleTerms t = trk4::scale_terms_forward(f, n_v, verts, faces, scales, th_ratio, th_edge);
    s[0] += (double)t.ratio; s[1] += (double)t.edge; s[2] += (double)t.q; s[3] += (double)t.q * (double)t.q;
  }
  const double n = (double)n_f;
  terms[0] = (float)(s[0] / n);
  terms[1] = (float)(s[1] / n);
  terms[2] = (float)((s[3] - s[2] * s[2] / n) / (n - 1.0));
  terms[3] = (float)(s[2] / n);
}

extern "C" void h4_scale_backward(int n_f, int n_v, const float *verts, const int32_t *faces, const float *scales, float th_ratio, float th_edge,
                                  const float *terms, const float *g, const int32_t *start, const int32_t *items, float *d_stencil,
                                  float *d_verts, float *d_scales) {
  if (!d_verts && !d_scales) return;
  for (int f = 0; f < n_f; ++f)
    trk4::scale_terms_backward(f, n_f, n_v, verts, faces, scales, th_ratio, th_edge, terms[3], g, d_verts ? d_stencil : nullptr, d_scales);
  if (d_verts)
    for (int v = 0; v < n_v; ++v) fgrad::vertex_gather(v, start, items, d_stencil, d_verts);
}

#ifdef HOSTTRACK4D_MAIN
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <utility>
#include <vector>

namespace {

float synth(int i) { return 0.25f + 0.5f * std::sin(0.37f * (float)i + 0.1f); }

int run(int n_v, const std::vector<int32_t> &faces) {
  const int n_f = (int)faces.size() / 3;
  // the adjacency: every edge in both directions, sorted, each once
  std::vector<std::pair<int32_t, int32_t>> edges;
  for (int f = 0; f < n_f; ++f)
    for (int k = 0; k < 3; ++k) {
      const int32_t a = faces[3 * f + k], b = faces[3 * f + (k + 1) % 3];
      edges.emplace_back(a, b);
      edges.emplace_back(b, a);
    }
  std::sort(edges.begin(), edges.end());
  edges.erase(std::unique(edges.begin(), edges.end()), edges.end());
  std::vector<int32_t> nstart((size_t)n_v + 1, 0), nbr(edges.size());
  for (size_t i = 0; i < edges.size(); ++i) { ++nstart[edges[i].first + 1]; nbr[i] = edges[i].second; }
  for (int v = 0; v < n_v; ++v) nstart[v + 1] += nstart[v];
  // the corner table: a stable counting sort of the corners by vertex
  std::vector<int32_t> start((size_t)n_v + 1, 0), items(faces.size());
  for (int32_t k : faces) ++start[k + 1];
  for (int v = 0; v < n_v; ++v) start[v + 1] += start[v];
  std::vector<int32_t> at(start.begin(), start.end() - 1);
  for (size_t i = 0; i < faces.size(); ++i) items[at[faces[i]]++] = (int32_t)i;
  // exactly sized arrays: an access past a row is the sanitizer's to report
  std::vector<float> verts(3 * (size_t)n_v), lv(3 * (size_t)n_v), d_verts(3 * (size_t)n_v), scales(3 * (size_t)n_f), d_scales(3 * (size_t)n_f),
      stencil(9 * (size_t)n_f);
  for (size_t i = 0; i < verts.size(); ++i) verts[i] = 0.3f * synth((int)i) + 0.05f * (float)(i % 7);
  for (size_t i = 0; i < scales.size(); ++i) scales[i] = i % 3 == 2 ? 0.f : 0.02f + 0.2f * synth((int)i) * synth((int)i);
  float value = -1.f, terms[4] = {0.f, 0.f, 0.f, 0.f};
  const float one = 1.f, g[3] = {10.f, 1000.f, 10.f};
  h4_laplacian_forward(n_v, verts.data(), nstart.data(), nbr.data(), lv.data(), &value);
  h4_laplacian_forward(n_v, verts.data(), nstart.data(), nbr.data(), nullptr, &value);
  h4_laplacian_backward(n_v, lv.data(), nstart.data(), nbr.data(), &one, d_verts.data());
  if (!(value > 0.f)) return 2;
  for (float v : d_verts) if (!std::isfinite(v)) return 3;
  if (n_f == 0) return 0;
  h4_scale_forward(n_f, n_v, verts.data(), faces.data(), scales.data(), 5.f, 1.f, terms);
  h4_scale_backward(n_f, n_v, verts.data(), faces.data(), scales.data(), 5.f, 1.f, terms, g, start.data(), items.data(), stencil.data(),
                    d_verts.data(), d_scales.data());
  h4_scale_backward(n_f, n_v, verts.data(), faces.data(), scales.data(), 5.f, 1.f, terms, g, nullptr, nullptr, nullptr, nullptr, d_scales.data());
  for (int k = 0; k < 4; ++k) if (!std::isfinite(terms[k])) return 4;
  for (float v : d_verts) if (!std::isfinite(v)) return 5;
  for (size_t i = 0; i < d_scales.size(); ++i) if (!std::isfinite(d_scales[i]) || (i % 3 == 2 && d_scales[i] != 0.f)) return 6;
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  int n_v = 4;
  std::vector<int32_t> faces = {0, 1, 2, 0, 2, 3};  // two triangles sharing an edge
  if (argc > 1) {  // int32: n_v, n_f; then int32 faces [3 n_f]
    FILE *fp = std::fopen(argv[1], "rb");
    if (!fp) return 20;
    int32_t hdr[2];
    if (std::fread(hdr, 4, 2, fp) != 2) return 21;
    n_v = hdr[0];
    faces.resize(3 * (size_t)hdr[1]);
    if (std::fread(faces.data(), 4, faces.size(), fp) != faces.size()) return 22;
    std::fclose(fp);
  }
  int rc = run(n_v, faces);
  if (rc) { std::printf("FAILED %d\n", rc); return rc; }
  rc = run(n_v + 2, faces);  // two vertices in no face
  if (rc) { std::printf("FAILED (isolated) %d\n", rc); return rc; }
  rc = run(n_v, std::vector<int32_t>());  // no face at all: every row is -v
  if (rc) { std::printf("FAILED (F = 0) %d\n", rc); return rc; }
  std::printf("ok: %d faces, %d vertices; two isolated vertices; F = 0\n", (int)faces.size() / 3, n_v);
  return 0;
}
#endif
