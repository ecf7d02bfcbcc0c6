// The AO bake (mpmavatar_amd/csrc/ao_math.hpp) compiled for the host (tests/test_ao_host.py, tests/test_gpu_ao_bake.py; the stand-in
// for <hip/hip_runtime.h> is tests/hostmath/stub): serial loops over the per-item functions, one loop per kernel of ao.hip, plus
// what only a test wants: the brute-force trace over all faces, and the set of faces a single ray hits either way.
// With -DHOSTAO_MAIN the file is a stand-alone program for a sanitizer build: a small closed scene through every loop.
#include "ao_math.hpp"

#include <cstdint>
#include <vector>

namespace {

struct HostGrid {
  ao::Grid g;
  std::vector<uint32_t> start;
  std::vector<int32_t> items;
  std::vector<ao::Tri> tri;
};

// k_ao_prepare + k_ao_grid_setup + count / scan / fill, serially (faces ascending inside a cell)
void build(int n_f, const float *verts, const int32_t *faces, int32_t cap_cells, HostGrid &h) {
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY}, edges = 0.f;
  h.tri.resize(n_f);
  for (int f = 0; f < n_f; ++f) {
    const ao::V3 v[3] = {ao::load3(verts, faces[3 * f]), ao::load3(verts, faces[3 * f + 1]), ao::load3(verts, faces[3 * f + 2])};
    h.tri[f] = ao::make_tri(v[0], v[1], v[2]);
    for (int k = 0; k < 3; ++k) {
      mn[0] = fminf(mn[0], v[k].x); mn[1] = fminf(mn[1], v[k].y); mn[2] = fminf(mn[2], v[k].z);
      mx[0] = fmaxf(mx[0], v[k].x); mx[1] = fmaxf(mx[1], v[k].y); mx[2] = fmaxf(mx[2], v[k].z);
      const ao::V3 e = ao::sub(v[(k + 1) % 3], v[k]);
      edges += sqrtf(ao::dot(e, e));
    }
  }
  h.g = ao::grid_setup(mn, mx, n_f > 0 ? edges / (3.f * (float)n_f) : 0.f, cap_cells);
  h.start.assign((size_t)h.g.n_cells + 1, 0);
  for (int f = 0; f < n_f; ++f) ao::for_face_cells(h.g, verts, faces, f, [&](int32_t c) { ++h.start[c + 1]; });
  for (int c = 0; c < h.g.n_cells; ++c) h.start[c + 1] += h.start[c];
  std::vector<uint32_t> at(h.start.begin(), h.start.end() - 1);
  h.items.assign(h.start[h.g.n_cells], 0);
  for (int f = 0; f < n_f; ++f) ao::for_face_cells(h.g, verts, faces, f, [&](int32_t c) { h.items[at[c]++] = f; });
}

bool brute_occluded(const HostGrid &h, int32_t own, ao::V3 o, ao::V3 d, float bias, float tmax) {
  for (int32_t f = 0; f < (int32_t)h.tri.size(); ++f)
    if (f != own && ao::ray_hits(o, d, h.tri[f], bias, tmax)) return true;
  return false;
}

}  // namespace

extern "C" void ha_coverage(int n_f, const int32_t *faces, const int32_t *ft, const float *vt, int H, int W, int32_t *cov_face, float *cov_bary) {
  for (int t = 0; t < H * W; ++t) cov_face[t] = INT32_MAX;
  for (int f = 0; f < n_f; ++f)
    ao::face_texels(f, faces, ft, vt, H, W, [&](int texel) { if (f < cov_face[texel]) cov_face[texel] = f; });
  for (int t = 0; t < H * W; ++t) {
    if (cov_face[t] == INT32_MAX) { cov_face[t] = -1; cov_bary[2 * t] = cov_bary[2 * t + 1] = 0.f; }
    else ao::texel_bary(t, cov_face[t], ft, vt, H, W, cov_bary + 2 * t);
  }
}

// origin, normal, tangent, bitangent [H*W*3] each (bitangent may be NULL)
extern "C" void ha_frames(const float *verts, const int32_t *faces, int H, int W, const int32_t *cov_face, const float *cov_bary, const float *rot,
                          float *origin, float *normal, float *tangent, float *bitangent) {
  for (int t = 0; t < H * W; ++t) {
    ao::Frame fr{};
    const int32_t f = cov_face[t];
    if (f >= 0)
      fr = ao::texel_frame(ao::load3(verts, faces[3 * f]), ao::load3(verts, faces[3 * f + 1]), ao::load3(verts, faces[3 * f + 2]), cov_bary[2 * t],
                           cov_bary[2 * t + 1], rot[2 * t], rot[2 * t + 1]);
    ao::store3(origin, t, fr.p);
    ao::store3(normal, t, fr.n);
    ao::store3(tangent, t, fr.t);
    if (bitangent) ao::store3(bitangent, t, fr.b);
  }
}

// occluded [H*W] (0 on uncovered texels) from GIVEN frames (origin, normal, tangent; b = n x t as texel_frame forms it), by the grid
// walk (brute = 0) or over all faces (brute = 1).  A texel whose normal is all zero is skipped.
extern "C" void ha_count(int n_f, const float *verts, const int32_t *faces, int32_t cap_cells, int H, int W, const int32_t *cov_face, const float *origin,
                         const float *normal, const float *tangent, int S, const float *dirs, float bias, float tmax, int brute, int32_t *occluded) {
  HostGrid h;
  build(n_f, verts, faces, cap_cells, h);
  for (int t = 0; t < H * W; ++t) {
    occluded[t] = 0;
    if (cov_face[t] < 0) continue;
    ao::Frame fr{ao::load3(origin, t), ao::load3(normal, t), ao::load3(tangent, t), ao::V3{0.f, 0.f, 0.f}, true};
    if (fr.n.x == 0.f && fr.n.y == 0.f && fr.n.z == 0.f) continue;
    fr.b = ao::cross(fr.n, fr.t);
    for (int i = 0; i < S; ++i) {
      const ao::V3 d = ao::ray_dir(fr, dirs, i);
      occluded[t] += brute ? brute_occluded(h, cov_face[t], fr.p, d, bias, tmax)
                           : ao::ray_occluded(h.g, h.start.data(), h.items.data(), h.tri.data(), cov_face[t], fr.p, d, bias, tmax);
    }
  }
}

// the whole bake before the margin: ao [H*W] (0 on uncovered texels) and the counts
extern "C" void ha_bake(int n_f, const float *verts, const int32_t *faces, int32_t cap_cells, int H, int W, const int32_t *cov_face, const float *cov_bary,
                        const float *rot, int S, const float *dirs, float bias, float tmax, int brute, float *ao_out, int32_t *occluded) {
  std::vector<float> o(3 * (size_t)H * W), n(o.size()), t(o.size());
  ha_frames(verts, faces, H, W, cov_face, cov_bary, rot, o.data(), n.data(), t.data(), nullptr);
  ha_count(n_f, verts, faces, cap_cells, H, W, cov_face, o.data(), n.data(), t.data(), S, dirs, bias, tmax, brute, occluded);
  for (int i = 0; i < H * W; ++i) {
    const bool live = cov_face[i] >= 0 && !(n[3 * i] == 0.f && n[3 * i + 1] == 0.f && n[3 * i + 2] == 0.f);
    ao_out[i] = live ? ao::ao_value(occluded[i], S) : 0.f;
  }
}

// hits [n_rays * n_f]: 1 where ray r meets face f, found by walking the grid without an early exit (brute = 0) or by trying every
// face (brute = 1).  dims [4]: the grid's cells per axis and the number of (cell, face) entries.
extern "C" void ha_ray_faces(int n_f, const float *verts, const int32_t *faces, int32_t cap_cells, int n_rays, const float *o, const float *d, float bias,
                             float tmax, int brute, uint8_t *hits, int64_t *dims) {
  HostGrid h;
  build(n_f, verts, faces, cap_cells, h);
  if (dims) { dims[0] = h.g.dim[0]; dims[1] = h.g.dim[1]; dims[2] = h.g.dim[2]; dims[3] = (int64_t)h.items.size(); }
  for (int r = 0; r < n_rays; ++r) {
    uint8_t *row = hits + (size_t)r * n_f;
    for (int f = 0; f < n_f; ++f) row[f] = 0;
    const ao::V3 ro = ao::load3(o, r), rd = ao::load3(d, r);
    if (brute) {
      for (int f = 0; f < n_f; ++f) row[f] = ao::ray_hits(ro, rd, h.tri[f], bias, tmax);
    } else {
      ao::walk(h.g, ro, rd, tmax, [&](int32_t cell) {
        for (uint32_t j = h.start[cell]; j < h.start[cell + 1]; ++j)
          if (ao::ray_hits(ro, rd, h.tri[h.items[j]], bias, tmax)) row[h.items[j]] = 1;
        return false;
      });
    }
  }
}

extern "C" void ha_margin(int H, int W, const float *in_val, const uint8_t *in_mask, float *out_val, uint8_t *out_mask) {
  for (int t = 0; t < H * W; ++t) ao::margin_texel(t, H, W, in_val, in_mask, out_val, out_mask);
}

#ifdef HOSTAO_MAIN
#include <cstdio>

// A unit quad (two faces) under a tilted roof (two faces) with a per-face atlas, through every loop, grid against brute force.
int main() {
  const std::vector<float> verts = {0, 0, 0, 1, 0, 0, 1, 0, 1, 0, 0, 1, -1, 0.2f, -1, 2, 0.3f, -1, 2, 0.6f, 2, -1, 0.4f, 2, 9, 9, 9};
  const std::vector<int32_t> faces = {0, 2, 1, 0, 3, 2, 4, 5, 6, 4, 6, 7, 8, 8, 8}, ft = {0, 1, 2, 0, 2, 3, 4, 5, 6, 4, 6, 7, 0, 0, 0};
  const std::vector<float> vt = {0.05f, 0.05f, 0.45f, 0.05f, 0.45f, 0.45f, 0.05f, 0.45f, 0.55f, 0.55f, 0.95f, 0.55f, 0.95f, 0.95f, 0.55f, 0.95f};
  const int n_f = (int)faces.size() / 3, H = 9, W = 7, S = 5;
  std::vector<int32_t> cov((size_t)H * W), occ_g(cov.size()), occ_b(cov.size());
  std::vector<float> bary(2 * cov.size()), rot(2 * cov.size()), dirs(3 * (size_t)S), ao_g(cov.size()), ao_b(cov.size()), out(cov.size());
  for (size_t t = 0; t < cov.size(); ++t) { rot[2 * t] = cosf(0.7f * (float)t); rot[2 * t + 1] = sinf(0.7f * (float)t); }
  for (int i = 0; i < S; ++i) {
    const float u = ((float)i + 0.5f) / (float)S, r = sqrtf(u), phi = 2.4f * (float)i;
    dirs[3 * i] = r * cosf(phi); dirs[3 * i + 1] = r * sinf(phi); dirs[3 * i + 2] = sqrtf(1.f - u);
  }
  ha_coverage(n_f, faces.data(), ft.data(), vt.data(), H, W, cov.data(), bary.data());
  int covered = 0, shaded = 0;
  for (int32_t f : cov) covered += f >= 0;
  for (int32_t cap : {1, 7, 4096}) {
    ha_bake(n_f, verts.data(), faces.data(), cap, H, W, cov.data(), bary.data(), rot.data(), S, dirs.data(), 1e-4f, 10.f, 0, ao_g.data(), occ_g.data());
    ha_bake(n_f, verts.data(), faces.data(), cap, H, W, cov.data(), bary.data(), rot.data(), S, dirs.data(), 1e-4f, 10.f, 1, ao_b.data(), occ_b.data());
    for (size_t t = 0; t < cov.size(); ++t) {
      if (occ_g[t] != occ_b[t]) { std::printf("FAILED: texel %zu grid %d brute %d (cap %d)\n", t, occ_g[t], occ_b[t], cap); return 2; }
      shaded += occ_g[t] > 0;
    }
  }
  std::vector<uint8_t> m0(cov.size()), m1(cov.size());
  for (size_t t = 0; t < cov.size(); ++t) m0[t] = cov[t] >= 0;
  ha_margin(H, W, ao_g.data(), m0.data(), out.data(), m1.data());
  std::vector<uint8_t> hits((size_t)n_f);
  const float o[3] = {5.f, 5.f, 5.f}, d[3] = {0.f, 0.f, 0.f};  // a ray that starts outside the grid and goes nowhere
  ha_ray_faces(n_f, verts.data(), faces.data(), 64, 1, o, d, 1e-4f, 10.f, 0, hits.data(), nullptr);
  ha_ray_faces(0, verts.data(), faces.data(), 64, 1, o, d, 1e-4f, 10.f, 0, hits.data(), nullptr);  // no faces
  if (!covered || !shaded) { std::printf("FAILED: %d covered, %d shaded\n", covered, shaded); return 3; }
  std::printf("ok: %d faces, %d x %d map, %d texels covered, %d texel bakes with an occluded ray\n", n_f, H, W, covered, shaded);
  return 0;
}
#endif
