// The backward math of the mesh binding (mpmavatar_amd/csrc/frames_grad_math.hpp) compiled for the host
// (tests/test_binding_grad_host.py; the stand-in for <hip/hip_runtime.h> is tests/hostmath/stub): serial loops over the four per-item
// functions, one loop per kernel of frames_backward.hip, with the same CSR indexing and the same order of the sums.
// With -DHOSTFRAMES_GRAD_MAIN the file is a stand-alone program for a sanitizer build: it reads an index structure (faces, binding)
// from a file, fills in synthetic parameters, runs the per-face forward (frm::face_frame_row, the loop of tests/hostframes/) into
// exactly sized outputs and every backward loop on what it saved, also with n = 0.
#include "frames_grad_math.hpp"

#include <cstdint>

extern "C" void hf_render_inputs_backward(int n, int n_f, const int32_t *binding, const float *xyz_local, const float *rot_raw,
                                          const float *scaling_raw, const float *opacity_raw, const float *mat, const float *quat,
                                          const float *fscale, const float *g_mean, const float *g_opac, const float *g_scale,
                                          const float *g_rot, float *d_xyz, float *d_rot, float *d_scaling, float *d_opacity,
                                          const int32_t *face_start, const int32_t *face_items, float *d_center, float *d_mat, float *d_quat,
                                          float *d_fscale) {
  if (d_xyz || d_rot || d_scaling || d_opacity)
    for (int g = 0; g < n; ++g)
      fgrad::gaussian_backward(g, binding, rot_raw, scaling_raw, opacity_raw, mat, quat, fscale, g_mean, g_rot, g_scale, g_opac, d_xyz, d_rot,
                               d_scaling, d_opacity);
  if (d_center)
    for (int f = 0; f < n_f; ++f)
      fgrad::face_accumulate(f, face_start, face_items, xyz_local, rot_raw, scaling_raw, mat, quat, fscale, g_mean, g_rot, g_scale, d_center,
                             d_mat, d_quat, d_fscale);
}

extern "C" void hf_face_frames_backward(const float *verts, const int32_t *faces, int n_f, int n_v, const float *mat, const float *quat,
                                        const float *g_center, const float *g_mat, const float *g_quat, const float *g_fscale,
                                        const int32_t *vert_start, const int32_t *vert_corners, float *d_corners, float *d_verts) {
  for (int f = 0; f < n_f; ++f) fgrad::face_frames_backward(f, verts, faces, mat, quat, g_center, g_mat, g_quat, g_fscale, d_corners);
  for (int v = 0; v < n_v; ++v) fgrad::vertex_gather(v, vert_start, vert_corners, d_corners, d_verts);
}

#ifdef HOSTFRAMES_GRAD_MAIN
#include <cmath>
#include <cstdio>
#include <vector>

namespace {

// key -> items table: start [n_keys + 1], items in ascending item index within a key (a stable counting sort)
void csr(const std::vector<int32_t> &key, int n_keys, std::vector<int32_t> &start, std::vector<int32_t> &items) {
  start.assign(n_keys + 1, 0);
  for (int32_t k : key) ++start[k + 1];
  for (int k = 0; k < n_keys; ++k) start[k + 1] += start[k];
  std::vector<int32_t> at(start.begin(), start.end() - 1);
  items.assign(key.size(), 0);
  for (size_t i = 0; i < key.size(); ++i) items[at[key[i]]++] = (int32_t)i;
}

float synth(int i) { return 0.25f + 0.5f * std::sin(0.37f * (float)i + 0.1f); }

int run(int n_v, const std::vector<int32_t> &faces, const std::vector<int32_t> &binding) {
  const int n_f = (int)faces.size() / 3, n = (int)binding.size();
  std::vector<float> verts(3 * (size_t)n_v);
  for (int v = 0; v < n_v; ++v) {  // points spread in space: no two vertices of a face coincide
    verts[3 * v] = std::cos(0.7f * v) + 0.01f * v;
    verts[3 * v + 1] = std::sin(1.3f * v);
    verts[3 * v + 2] = std::cos(2.1f * v + 1.f);
  }
  // the real forward into exactly sized outputs: a write past a row is the sanitizer's to report
  std::vector<float> center(3 * (size_t)n_f), mat(9 * (size_t)n_f), quat(4 * (size_t)n_f), fscale(n_f);
  for (int f = 0; f < n_f; ++f) frm::face_frame_row(f, verts.data(), faces.data(), center.data(), mat.data(), quat.data(), fscale.data());
  std::vector<float> xyz(3 * (size_t)n), rot(4 * (size_t)n), scl(3 * (size_t)n), opa(n), gm(3 * (size_t)n), gr(4 * (size_t)n), gs(3 * (size_t)n), go(n);
  for (int i = 0; i < 3 * n; ++i) { xyz[i] = synth(i); scl[i] = -1.f + synth(i + 5); gm[i] = synth(i + 11); gs[i] = synth(i + 13); }
  for (int i = 0; i < 4 * n; ++i) { rot[i] = synth(i + 3); gr[i] = synth(i + 17); }
  for (int i = 0; i < n; ++i) { opa[i] = synth(i + 7); go[i] = synth(i + 19); }
  std::vector<int32_t> fstart, fitems, vstart, vcorners;
  csr(binding, n_f, fstart, fitems);
  csr(faces, n_v, vstart, vcorners);
  // exactly sized outputs: a write past a row is the sanitizer's to report
  std::vector<float> d_xyz(3 * (size_t)n), d_rot(4 * (size_t)n), d_scl(3 * (size_t)n), d_opa(n), d_c(3 * (size_t)n_f), d_m(9 * (size_t)n_f), d_q(4 * (size_t)n_f),
      d_s(n_f), d_corner(9 * (size_t)n_f), d_verts(3 * (size_t)n_v);
  hf_render_inputs_backward(n, n_f, binding.data(), xyz.data(), rot.data(), scl.data(), opa.data(), mat.data(), quat.data(), fscale.data(),
                            gm.data(), go.data(), gs.data(), gr.data(), d_xyz.data(), d_rot.data(), d_scl.data(), d_opa.data(), fstart.data(),
                            fitems.data(), d_c.data(), d_m.data(), d_q.data(), d_s.data());
  hf_face_frames_backward(verts.data(), faces.data(), n_f, n_v, mat.data(), quat.data(), d_c.data(), d_m.data(), d_q.data(), d_s.data(),
                          vstart.data(), vcorners.data(), d_corner.data(), d_verts.data());
  // the null forms: no upstream at all, no parameter gradient wanted
  hf_render_inputs_backward(n, n_f, binding.data(), nullptr, nullptr, nullptr, nullptr, mat.data(), quat.data(), fscale.data(), nullptr,
                            nullptr, nullptr, nullptr, d_xyz.data(), nullptr, nullptr, nullptr, fstart.data(), fitems.data(), d_c.data(),
                            d_m.data(), d_q.data(), d_s.data());
  for (float v : d_xyz) if (v != 0.f) return 2;
  for (float v : d_m) if (v != 0.f) return 3;
  hf_render_inputs_backward(n, n_f, binding.data(), xyz.data(), rot.data(), scl.data(), opa.data(), mat.data(), quat.data(), fscale.data(),
                            gm.data(), go.data(), gs.data(), gr.data(), d_xyz.data(), d_rot.data(), d_scl.data(), d_opa.data(), fstart.data(),
                            fitems.data(), d_c.data(), d_m.data(), d_q.data(), d_s.data());
  int bad = 0;
  for (int f = 0; f < n_f; ++f) {
    bool empty = fstart[f] == fstart[f + 1];
    for (int k = 0; k < 9; ++k) {
      if (!std::isfinite(d_m[9 * f + k])) bad = 4;
      if (empty && d_m[9 * f + k] != 0.f) bad = 5;
    }
    if (empty && (d_s[f] != 0.f || d_c[3 * f] != 0.f || d_q[4 * f] != 0.f)) bad = 6;
  }
  for (int v = 0; v < n_v; ++v)
    for (int k = 0; k < 3; ++k) {
      if (!std::isfinite(d_verts[3 * v + k])) bad = 7;
      if (vstart[v] == vstart[v + 1] && d_verts[3 * v + k] != 0.f) bad = 8;
    }
  return bad;
}

}  // namespace

int main(int argc, char **argv) {
  std::vector<int32_t> faces, binding;
  int n_v = 0;
  if (argc > 1) {  // int32: n_v, n_f, n, then faces [3 n_f], binding [n]
    FILE *fp = std::fopen(argv[1], "rb");
    if (!fp) return 10;
    int32_t hdr[3];
    if (std::fread(hdr, 4, 3, fp) != 3) return 11;
    n_v = hdr[0];
    faces.resize(3 * (size_t)hdr[1]);
    binding.resize(hdr[2]);
    if (std::fread(faces.data(), 4, faces.size(), fp) != faces.size()) return 12;
    if (std::fread(binding.data(), 4, binding.size(), fp) != binding.size()) return 13;
    std::fclose(fp);
  } else {  // a fan of four triangles around vertex 0, vertex 6 in no face, face 3 without Gaussians
    n_v = 7;
    faces = {0, 1, 2, 0, 2, 3, 0, 3, 4, 0, 4, 5};
    binding = {2, 0, 0, 1, 0, 2};
  }
  int empty_faces = 0, lone_verts = 0;
  {
    std::vector<int32_t> s, it;
    csr(binding, (int)faces.size() / 3, s, it);
    for (size_t f = 0; f + 1 < s.size(); ++f) empty_faces += s[f] == s[f + 1];
    csr(faces, n_v, s, it);
    for (size_t v = 0; v + 1 < s.size(); ++v) lone_verts += s[v] == s[v + 1];
  }
  int rc = run(n_v, faces, binding);
  if (rc) { std::printf("FAILED %d\n", rc); return rc; }
  rc = run(n_v, faces, std::vector<int32_t>());  // n = 0
  if (rc) { std::printf("FAILED (n = 0) %d\n", rc); return rc; }
  std::printf("ok: %d vertices (%d in no face), %d faces (%d without Gaussians), %d Gaussians\n", n_v, lone_verts, (int)faces.size() / 3,
              empty_faces, (int)binding.size());
  return 0;
}
#endif
