// The mesh tracking step (mpmavatar_amd/csrc/track_math.hpp) compiled for the host (tests/test_track_host.py; the stand-in for
// <hip/hip_runtime.h> is tests/hostmath/stub): serial loops over the per-item functions, one loop per kernel of track.hip, with the
// same corner indexing; the sums are plain double sums in index order, and the nearest body vertex is the first strict minimum of
// geo::pair_d2 in ascending order -- the lowest index of the exact minimum, which is what k_nn_d2 returns.
// With -DHOSTTRACK_MAIN the file is a stand-alone program for a sanitizer build: it reads a mesh's faces from a file, builds the
// corner table, fills in synthetic values and runs every loop, and also F = 0 and n = 0.
#include "geo_math.hpp"
#include "track_math.hpp"

#include <cstdint>

extern "C" void ht_render_vars(int n_f, int n_v, const float *verts, const int32_t *faces, const float *ls, const float *lo, float *means,
                               float *rot, float *scales, float *opac) {
  for (int f = 0; f < n_f; ++f) trk::render_vars_forward(f, n_v, verts, faces, ls, lo, means, rot, scales, opac);
}

extern "C" void ht_render_vars_backward(int n_f, int n_v, const float *verts, const int32_t *faces, const float *ls, const float *lo,
                                        const float *g_means, const float *g_rot, const float *g_scales, const float *g_opac,
                                        const int32_t *start, const int32_t *items, float *d_stencil, float *d_verts, float *d_ls, float *d_lo) {
  if (!d_verts && !d_ls && !d_lo) return;
  for (int f = 0; f < n_f; ++f)
    trk::render_vars_backward(f, n_v, verts, faces, ls, lo, g_means, g_rot, g_scales, g_opac, d_verts ? d_stencil : nullptr, d_ls, d_lo);
  if (d_verts)
    for (int v = 0; v < n_v; ++v) fgrad::vertex_gather(v, start, items, d_stencil, d_verts);
}

extern "C" void ht_face_geometry(int n_f, int n_v, const float *verts, const int32_t *faces, float *normals, float *areas) {
  for (int f = 0; f < n_f; ++f) trk::face_geometry(f, n_v, verts, faces, normals, areas);
}

extern "C" void ht_terms_forward(int n_f, int n_v, const float *verts, const int32_t *faces, const float *ls, const float *lo, float *terms) {
  if (n_f == 0) return;
  double s[3] = {0.0, 0.0, 0.0};
  for (int f = 0; f < n_f; ++f) {
    const trk::Terms t = trk::terms_forward(f, n_v, verts, faces, ls, lo);
    s[0] += (double)t.area; s[1] += (double)t.scale; s[2] += (double)t.opacity;
  }
  for (int k = 0; k < 3; ++k) terms[k] = (float)(s[k] / (double)n_f);
}

extern "C" void ht_terms_backward(int n_f, int n_v, const float *verts, const int32_t *faces, const float *ls, const float *lo, const float *g,
                                  const int32_t *start, const int32_t *items, float *d_stencil, float *d_verts, float *d_ls, float *d_lo) {
  if (!d_verts && !d_ls && !d_lo) return;
  for (int f = 0; f < n_f; ++f) trk::terms_backward(f, n_f, n_v, verts, faces, ls, lo, g, d_verts ? d_stencil : nullptr, d_ls, d_lo);
  if (d_verts)
    for (int v = 0; v < n_v; ++v) fgrad::vertex_gather(v, start, items, d_stencil, d_verts);
}

extern "C" void ht_vertex_normals(int n_f, int n_v, const float *verts, const int32_t *faces, const int32_t *start, const int32_t *items,
                                  float *normals) {
  (void)n_f;
  for (int v = 0; v < n_v; ++v) trk::vertex_normal(v, n_v, verts, faces, start, items, normals);
}

extern "C" void ht_collision_forward(int n, const float *va, const float *vb, const float *nb, int n_body, float eps, int mode, int32_t *index,
                                     float *dist, float *value) {
  double s = 0.0;
  for (int i = 0; i < n; ++i) {
    const geo::P3 q{va[3 * i], va[3 * i + 1], va[3 * i + 2]};
    int best = 0;
    float d2 = INFINITY;
    for (int j = 0; j < n_body; ++j) {
      const float d = geo::pair_d2(q, geo::P3{vb[3 * j], vb[3 * j + 1], vb[3 * j + 2]});
      if (d < d2) { d2 = d; best = j; }
    }
    index[i] = best;
    if (!nb) continue;
    dist[i] = trk::signed_distance(i, va, vb, nb, best);
    s += (double)trk::penalty(dist[i], eps, mode);
  }
  if (nb && mode != trk::MODE_DISTANCE && n > 0) value[0] = (float)(mode == trk::MODE_AVERAGE ? s / (double)n : s);
}

extern "C" void ht_collision_backward(int n, const float *nb, int n_body, const int32_t *index, const float *dist, float eps, int mode,
                                      const float *g, float *d_va) {
  for (int i = 0; i < n; ++i) trk::collision_backward(i, n, nb, n_body, index, dist, eps, mode, g, d_va);
}

#ifdef HOSTTRACK_MAIN
#include <cmath>
#include <cstdio>
#include <vector>

namespace {

float synth(int i) { return 0.25f + 0.5f * std::sin(0.37f * (float)i + 0.1f); }

int run_mesh(int n_v, const std::vector<int32_t> &faces) {
  const int n_f = (int)faces.size() / 3;
  // the corner table: a stable counting sort of the corners by vertex
  std::vector<int32_t> start((size_t)n_v + 1, 0), items(faces.size());
  for (int32_t k : faces) ++start[k + 1];
  for (int v = 0; v < n_v; ++v) start[v + 1] += start[v];
  std::vector<int32_t> at(start.begin(), start.end() - 1);
  for (size_t i = 0; i < faces.size(); ++i) items[at[faces[i]]++] = (int32_t)i;
  // exactly sized arrays: an access past a row is the sanitizer's to report
  std::vector<float> verts(3 * (size_t)n_v), ls(3 * (size_t)n_f), lo(n_f), means(3 * (size_t)n_f), rot(4 * (size_t)n_f), scales(3 * (size_t)n_f),
      opac(n_f), normals(3 * (size_t)n_f), areas(n_f), vnormals(3 * (size_t)n_v), stencil(9 * (size_t)n_f), d_verts(3 * (size_t)n_v),
      d_ls(3 * (size_t)n_f), d_lo(n_f);
  for (size_t i = 0; i < verts.size(); ++i) verts[i] = 0.3f * synth((int)i) + 0.05f * (float)(i % 7);
  for (size_t i = 0; i < ls.size(); ++i) ls[i] = i % 3 == 2 ? -100.f : -3.f + synth((int)i);
  for (int f = 0; f < n_f; ++f) lo[f] = 4.f * synth(f) - 2.f;
  float terms[3] = {0.f, 0.f, 0.f};
  const float g[3] = {500.f, 1.f, 0.05f};
  ht_render_vars(n_f, n_v, verts.data(), faces.data(), ls.data(), lo.data(), means.data(), rot.data(), scales.data(), opac.data());
  ht_face_geometry(n_f, n_v, verts.data(), faces.data(), normals.data(), areas.data());
  ht_vertex_normals(n_f, n_v, verts.data(), faces.data(), start.data(), items.data(), vnormals.data());
  ht_terms_forward(n_f, n_v, verts.data(), faces.data(), ls.data(), lo.data(), terms);
  // the forward's own outputs as upstream gradients: every row is read
  ht_render_vars_backward(n_f, n_v, verts.data(), faces.data(), ls.data(), lo.data(), means.data(), rot.data(), scales.data(), opac.data(),
                          start.data(), items.data(), stencil.data(), d_verts.data(), d_ls.data(), d_lo.data());
  ht_render_vars_backward(n_f, n_v, verts.data(), faces.data(), ls.data(), lo.data(), nullptr, rot.data(), nullptr, nullptr, start.data(),
                          items.data(), stencil.data(), d_verts.data(), nullptr, nullptr);
  for (float v : d_verts) if (!std::isfinite(v)) return 2;
  ht_terms_backward(n_f, n_v, verts.data(), faces.data(), ls.data(), lo.data(), g, start.data(), items.data(), stencil.data(), d_verts.data(),
                    d_ls.data(), d_lo.data());
  if (n_f == 0) {
    for (float v : d_verts) if (v != 0.f) return 3;
    return 0;
  }
  for (int k = 0; k < 3; ++k) if (!std::isfinite(terms[k])) return 4;
  for (float v : d_verts) if (!std::isfinite(v)) return 5;
  for (float v : d_ls) if (!std::isfinite(v)) return 6;
  for (int f = 0; f < n_f; ++f) {
    const float *q = &rot[4 * (size_t)f];
    if (!(q[0] >= 0.f) || std::fabs(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] - 1.f) > 1e-5f) return 7;
  }
  return 0;
}

int run_collision(int n, int m) {
  std::vector<float> va(3 * (size_t)n), vb(3 * (size_t)m), nb(3 * (size_t)m), dist(n), d_va(3 * (size_t)n), g(n > 0 ? n : 1, 0.5f);
  std::vector<int32_t> index(n);
  for (size_t i = 0; i < va.size(); ++i) va[i] = synth((int)i + 5);
  for (size_t i = 0; i < vb.size(); ++i) { vb[i] = synth(3 * (int)i + 1); nb[i] = synth(7 * (int)i) - 0.5f; }
  for (int mode = 0; mode < 3; ++mode) {
    float value = -1.f;
    ht_collision_forward(n, va.data(), vb.data(), nb.data(), m, 1e-3f, mode, index.data(), dist.data(), &value);
    ht_collision_backward(n, nb.data(), m, index.data(), dist.data(), 1e-3f, mode, g.data(), d_va.data());
    for (int32_t j : index) if (j < 0 || j >= m) return 8;
    for (float v : d_va) if (!std::isfinite(v)) return 9;
    if (n > 0 && mode != 0 && !(value >= 0.f)) return 10;
  }
  ht_collision_forward(n, va.data(), vb.data(), nullptr, m, 0.f, 0, index.data(), nullptr, nullptr);  // the index alone
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
  int rc = run_mesh(n_v, faces);
  if (rc) { std::printf("FAILED %d\n", rc); return rc; }
  rc = run_mesh(n_v, std::vector<int32_t>());  // F = 0
  if (rc) { std::printf("FAILED (F = 0) %d\n", rc); return rc; }
  rc = run_collision(301, 77);
  if (rc) { std::printf("FAILED (collision) %d\n", rc); return rc; }
  rc = run_collision(0, 77);
  if (rc) { std::printf("FAILED (n = 0) %d\n", rc); return rc; }
  std::printf("ok: %d faces, %d vertices; F = 0; 301 x 77 points; n = 0\n", (int)faces.size() / 3, n_v);
  return 0;
}
#endif
