// The colour path (mpmavatar_amd/csrc/shade_math.hpp) compiled for the host (tests/test_shade_host.py; the stand-in for
// <hip/hip_runtime.h> is tests/hostmath/stub): serial loops over the per-item functions, one loop per kernel of shade.hip, with the
// same CSR indexing and the same order of the sums.
// With -DHOSTSHADE_MAIN the file is a stand-alone program for a sanitizer build: it reads an index structure (map size, uv, binding)
// from a file, fills in synthetic values and runs every loop at every degree, in both NULL forms, and with n = 0.
#include "shade_math.hpp"

#include <cstdint>

extern "C" void hs_forward(int n, int n_f, const int32_t *binding, const float *means3D, const float *campos, int deg, int n_coeffs,
                           const float *dc, const float *rest, const float *map, int H, int W, const float *face_uv, float *colors) {
  for (int i = 0; i < n; ++i) shade::forward(i, n_f, binding, means3D, campos, deg, n_coeffs, dc, rest, map, H, W, face_uv, colors);
}

extern "C" void hs_backward(int n, int n_f, const int32_t *binding, const float *means3D, const float *campos, int deg, int n_coeffs,
                            const float *dc, const float *rest, const float *map, int H, int W, const float *face_uv,
                            const float *g_colors, float *d_dc, float *d_rest, float *d_means3D, const int32_t *face_start,
                            const int32_t *face_items, const int32_t *texel_start, const int32_t *texel_items, float *d_map,
                            float *scratch) {
  float *ds = d_map ? scratch : nullptr, *dS = d_map ? scratch + n : nullptr;
  if (d_dc || d_rest || d_means3D || d_map)
    for (int i = 0; i < n; ++i)
      shade::backward_gaussian(i, n_f, binding, means3D, campos, deg, n_coeffs, dc, rest, map, H, W, face_uv, g_colors, d_dc, d_rest,
                               d_means3D, ds);
  if (d_map) {
    for (int f = 0; f < n_f; ++f) shade::face_sum(f, face_start, face_items, ds, dS);
    for (int t = 0; t < H * W; ++t) shade::texel_sum(t, texel_start, texel_items, H, W, face_uv, dS, d_map);
  }
}

extern "C" void hs_taps(int n_f, const float *face_uv, int H, int W, int32_t *idx, float *w) {
  for (int f = 0; f < n_f; ++f) shade::shadow_taps(face_uv[2 * f], face_uv[2 * f + 1], H, W, idx + 4 * f, w + 4 * f);
}

#ifdef HOSTSHADE_MAIN
#include <cmath>
#include <cstdio>
#include <vector>

namespace {

// key -> items table: start [n_keys + 1], items in ascending item index within a key (a stable counting sort); key < 0 is dropped
void csr(const std::vector<int32_t> &key, int n_keys, std::vector<int32_t> &start, std::vector<int32_t> &items) {
  start.assign(n_keys + 1, 0);
  size_t kept = 0;
  for (int32_t k : key)
    if (k >= 0) { ++start[k + 1]; ++kept; }
  for (int k = 0; k < n_keys; ++k) start[k + 1] += start[k];
  std::vector<int32_t> at(start.begin(), start.end() - 1);
  items.assign(kept, 0);
  for (size_t i = 0; i < key.size(); ++i)
    if (key[i] >= 0) items[at[key[i]]++] = (int32_t)i;
}

float synth(int i) { return 0.25f + 0.5f * std::sin(0.37f * (float)i + 0.1f); }

int run(int H, int W, const std::vector<float> &uv, const std::vector<int32_t> &binding, int n_coeffs) {
  const int n_f = (int)uv.size() / 2, n = (int)binding.size();
  std::vector<int32_t> tap_texel(4 * (size_t)n_f);
  std::vector<float> tap_w(4 * (size_t)n_f);
  hs_taps(n_f, uv.data(), H, W, tap_texel.data(), tap_w.data());
  std::vector<int32_t> fstart, fitems, tstart, titems;
  csr(binding, n_f, fstart, fitems);
  csr(tap_texel, H * W, tstart, titems);
  // exactly sized inputs and outputs: an access past a row is the sanitizer's to report
  std::vector<float> means(3 * (size_t)n), dc(3 * (size_t)n), rest(3 * (size_t)n * (n_coeffs - 1)), map((size_t)H * W), g(3 * (size_t)n);
  for (size_t i = 0; i < means.size(); ++i) { means[i] = 2.f * synth((int)i); dc[i] = synth((int)i + 3) - 0.4f; g[i] = synth((int)i + 7); }
  for (size_t i = 0; i < rest.size(); ++i) rest[i] = 0.6f * (synth((int)i + 5) - 0.25f);
  for (size_t i = 0; i < map.size(); ++i) map[i] = 0.5f + synth((int)i + 11);
  const float campos[3] = {0.3f, -0.2f, 4.f};
  std::vector<float> colors(3 * (size_t)n), d_dc(3 * (size_t)n), d_rest(rest.size()), d_means(3 * (size_t)n), d_map((size_t)H * W),
      scratch((size_t)n + n_f);
  const int max_deg = n_coeffs >= 16 ? 3 : n_coeffs >= 9 ? 2 : n_coeffs >= 4 ? 1 : 0;
  for (int deg = 0; deg <= max_deg; ++deg) {
    hs_forward(n, n_f, binding.data(), means.data(), campos, deg, n_coeffs, dc.data(), rest.data(), map.data(), H, W, uv.data(),
               colors.data());
    hs_backward(n, n_f, binding.data(), means.data(), campos, deg, n_coeffs, dc.data(), rest.data(), map.data(), H, W, uv.data(), g.data(),
                d_dc.data(), d_rest.data(), d_means.data(), fstart.data(), fitems.data(), tstart.data(), titems.data(), d_map.data(),
                scratch.data());
    for (float v : colors) if (!std::isfinite(v)) return 2;
    for (float v : d_map) if (!std::isfinite(v)) return 3;
    for (int t = 0; t < H * W; ++t) if (tstart[t] == tstart[t + 1] && d_map[t] != 0.f) return 4;
    const int used = (deg + 1) * (deg + 1);
    for (int i = 0; i < n; ++i)
      for (int k = used; k < n_coeffs; ++k)
        for (int c = 0; c < 3; ++c) if (d_rest[(size_t)3 * (i * (size_t)(n_coeffs - 1) + k - 1) + c] != 0.f) return 5;
    if (deg == 0) for (float v : d_means) if (v != 0.f) return 6;
  }
  // the NULL forms: no shadow map (and no binding, uv or tables); no features; no upstream
  hs_forward(n, 0, nullptr, means.data(), campos, max_deg, n_coeffs, dc.data(), rest.data(), nullptr, 0, 0, nullptr, colors.data());
  hs_backward(n, 0, nullptr, means.data(), campos, max_deg, n_coeffs, dc.data(), rest.data(), nullptr, 0, 0, nullptr, g.data(), d_dc.data(),
              d_rest.data(), d_means.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  hs_forward(n, n_f, binding.data(), nullptr, nullptr, 0, 0, nullptr, nullptr, map.data(), H, W, uv.data(), colors.data());
  hs_backward(n, n_f, binding.data(), nullptr, nullptr, 0, 0, nullptr, nullptr, map.data(), H, W, uv.data(), g.data(), nullptr, nullptr,
              nullptr, fstart.data(), fitems.data(), tstart.data(), titems.data(), d_map.data(), scratch.data());
  for (float v : d_map) if (!std::isfinite(v)) return 7;
  hs_backward(n, n_f, binding.data(), means.data(), campos, max_deg, n_coeffs, dc.data(), rest.data(), map.data(), H, W, uv.data(), nullptr,
              d_dc.data(), d_rest.data(), d_means.data(), fstart.data(), fitems.data(), tstart.data(), titems.data(), d_map.data(),
              scratch.data());
  for (float v : d_map) if (v != 0.f) return 8;
  for (float v : d_dc) if (v != 0.f) return 9;
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  int H = 2, W = 3, n_coeffs = 16;
  std::vector<float> uv;
  std::vector<int32_t> binding;
  if (argc > 1) {  // int32: H, W, n_f, n, n_coeffs; then float uv [2 n_f]; then int32 binding [n]
    FILE *fp = std::fopen(argv[1], "rb");
    if (!fp) return 10;
    int32_t hdr[5];
    if (std::fread(hdr, 4, 5, fp) != 5) return 11;
    H = hdr[0]; W = hdr[1]; n_coeffs = hdr[4];
    uv.resize(2 * (size_t)hdr[2]);
    binding.resize(hdr[3]);
    if (std::fread(uv.data(), 4, uv.size(), fp) != uv.size()) return 12;
    if (std::fread(binding.data(), 4, binding.size(), fp) != binding.size()) return 13;
    std::fclose(fp);
  } else {  // four faces: one on a corner of the map, one outside it, face 3 without Gaussians
    uv = {-1.f, -1.f, 0.2f, 0.4f, 3.f, -2.f, 1.f, 1.f};
    binding = {2, 0, 0, 1, 0, 2};
  }
  const int n_f = (int)uv.size() / 2;
  std::vector<int32_t> s, it, tt(4 * (size_t)n_f);
  std::vector<float> tw(4 * (size_t)n_f);
  csr(binding, n_f, s, it);
  int empty_faces = 0, outside = 0, untapped = 0;
  for (int f = 0; f < n_f; ++f) empty_faces += s[f] == s[f + 1];
  hs_taps(n_f, uv.data(), H, W, tt.data(), tw.data());
  for (int f = 0; f < n_f; ++f) outside += tt[4 * f] < 0 && tt[4 * f + 1] < 0 && tt[4 * f + 2] < 0 && tt[4 * f + 3] < 0;
  csr(tt, H * W, s, it);
  for (int t = 0; t < H * W; ++t) untapped += s[t] == s[t + 1];
  int rc = run(H, W, uv, binding, n_coeffs);
  if (rc) { std::printf("FAILED %d\n", rc); return rc; }
  rc = run(H, W, uv, std::vector<int32_t>(), n_coeffs);  // n = 0
  if (rc) { std::printf("FAILED (n = 0) %d\n", rc); return rc; }
  std::printf("ok: %d x %d map (%d texels without a tap), %d faces (%d without Gaussians, %d outside the map), %d Gaussians\n", H, W,
              untapped, n_f, empty_faces, outside, (int)binding.size());
  return 0;
}
#endif
