// The image head (mpmavatar_amd/csrc/image_head_math.hpp) compiled for the host (tests/test_image_head_host.py; the stand-in for
// <hip/hip_runtime.h> is tests/hostmath/stub): serial loops over the per-pixel functions, one loop per kernel of image_head.hip, with
// the same deal of pixel quads to workgroups and lanes and the same two-stage order of the six sums (per-workgroup partials in the
// caller's scratch, then one fold that writes both [n_cam, 3] outputs in full).
// With -DHOSTIMAGEHEAD_MAIN the file is a stand-alone program for a sanitizer build: it reads cases from files, runs every loop over
// exactly sized buffers in every NULL form, and ends with a zero-pixel call.
#include "image_head_math.hpp"

#include <cmath>
#include <cstdint>

using imghead::QUAD;
using imghead::SUMS;
using imghead::TPB;

extern "C" int32_t ih_workgroups(int64_t n_pixels) { return imghead::workgroups(n_pixels); }

namespace {

void camera_row(const float *cam_m, const float *cam_c, int cam, float a[3], float c[3]) {
  for (int ch = 0; ch < 3; ++ch) {
    a[ch] = cam_m ? expf(cam_m[3 * (size_t)cam + ch]) : 1.0f;
    c[ch] = cam_m ? cam_c[3 * (size_t)cam + ch] : 0.0f;
  }
}

}  // namespace

extern "C" void ih_forward(const float *render, const float *mask, const float *cam_m, const float *cam_c, int n_cam, int cam, int H, int W,
                           float *image) {
  (void)n_cam;
  const int64_t hw = (int64_t)H * W;
  float a[3], c[3];
  camera_row(cam_m, cam_c, cam, a, c);
  for (int ch = 0; ch < 3; ++ch)
    for (int64_t p = 0; p < hw; ++p) image[ch * hw + p] = imghead::clip01(imghead::value(render[ch * hw + p], a[ch], c[ch], mask[p]));
}

extern "C" void ih_backward(const float *render, const float *mask, const float *cam_m, const float *cam_c, int n_cam, int cam, int H, int W,
                            const float *g_image, double *scratch, float *d_render, float *d_mask, float *d_cam_m, float *d_cam_c) {
  const int64_t hw = (int64_t)H * W, n_quads = (hw + QUAD - 1) / QUAD;
  const int n_wg = imghead::workgroups(hw);
  float a[3], c[3];
  camera_row(cam_m, cam_c, cam, a, c);
  const bool sums = d_cam_m || d_cam_c;
  // the map: workgroup b, lane t, quads b TPB + t, (b + n_wg) TPB + t, ...
  for (int b = 0; b < n_wg; ++b) {
    double part[SUMS] = {0, 0, 0, 0, 0, 0};
    for (int t = 0; t < TPB; ++t) {
      double lane[SUMS] = {0, 0, 0, 0, 0, 0};
      for (int64_t q = (int64_t)b * TPB + t; q < n_quads; q += (int64_t)n_wg * TPB)
        for (int k = 0; k < QUAD; ++k) {
          const int64_t p = q * QUAD + k;
          if (p >= hw) break;
          float share[3];
          for (int ch = 0; ch < 3; ++ch) {
            const imghead::PixelGrad pg = imghead::pixel_grad(render[ch * hw + p], a[ch], c[ch], mask[p], g_image ? g_image[ch * hw + p] : 0.0f);
            if (d_render) d_render[ch * hw + p] = pg.d_render;
            share[ch] = pg.d_mask;
            lane[ch] += (double)pg.s_c;
            lane[3 + ch] += (double)pg.s_m;
          }
          if (d_mask) d_mask[p] = imghead::mask_grad(share[0], share[1], share[2]);
        }
      for (int k = 0; k < SUMS; ++k) part[k] += lane[k];
    }
    if (sums)
      for (int k = 0; k < SUMS; ++k) scratch[(size_t)b * SUMS + k] = part[k];
  }
  if (!sums) return;
  // the fold: lane t adds the partials t, t + TPB, ..., then the lanes in index order
  double s[SUMS] = {0, 0, 0, 0, 0, 0};
  for (int t = 0; t < TPB; ++t) {
    double lane[SUMS] = {0, 0, 0, 0, 0, 0};
    for (int w = t; w < n_wg; w += TPB)
      for (int k = 0; k < SUMS; ++k) lane[k] += scratch[(size_t)w * SUMS + k];
    for (int k = 0; k < SUMS; ++k) s[k] += lane[k];
  }
  for (int i = 0; i < 3 * n_cam; ++i) {
    const int r = i / 3, ch = i - 3 * r;
    if (d_cam_c) d_cam_c[i] = r == cam ? (float)s[ch] : 0.0f;
    if (d_cam_m) d_cam_m[i] = r == cam ? (float)((double)a[ch] * s[3 + ch]) : 0.0f;
  }
}

extern "C" void ih_bytes(const float *render, const float *mask, const float *cam_m, const float *cam_c, int n_cam, int cam, int white, int H,
                         int W, uint8_t *out_u8) {
  (void)n_cam;
  const int64_t hw = (int64_t)H * W;
  float a[3], c[3];
  camera_row(cam_m, cam_c, cam, a, c);
  for (int64_t p = 0; p < hw; ++p)
    for (int ch = 0; ch < 3; ++ch) out_u8[3 * p + ch] = imghead::frame_byte(render[ch * hw + p], a[ch], c[ch], mask[p], white != 0);
}

extern "C" void ih_compose(const float *rgb, const float *msk, int white, int H, int W, float *out) {
  const int64_t hw = (int64_t)H * W;
  for (int ch = 0; ch < 3; ++ch)
    for (int64_t p = 0; p < hw; ++p) out[ch * hw + p] = imghead::compose(rgb[ch * hw + p], msk[p], white != 0);
}

extern "C" void ih_eval_pair(const uint8_t *pred_u8, const uint8_t *gt_u8, const float *mask, int remove_white, int H, int W, float *out_pred,
                             float *out_gt) {
  const int64_t hw = (int64_t)H * W;
  for (int img = 0; img < 2; ++img) {
    const uint8_t *in = img ? gt_u8 : pred_u8;
    float *out = img ? out_gt : out_pred;
    for (int64_t p = 0; p < hw; ++p) {
      float f[3];
      imghead::eval_pixel(in + 3 * p, mask[p], remove_white != 0, f);
      for (int ch = 0; ch < 3; ++ch) out[ch * hw + p] = f[ch];
    }
  }
}

#ifdef HOSTIMAGEHEAD_MAIN
#include <cstdio>
#include <vector>

namespace {

// every loop over exactly sized buffers: an access past a plane, a row of cam_m or the scratch is the sanitizer's to report
int run(int H, int W, int n_cam, int cam, const std::vector<float> &render, const std::vector<float> &mask, const std::vector<float> &cam_m,
        const std::vector<float> &cam_c, const std::vector<float> &g) {
  const size_t hw = (size_t)H * W;
  std::vector<float> image(3 * hw), d_render(3 * hw), d_mask(hw), d_cam_m(3 * (size_t)n_cam), d_cam_c(3 * (size_t)n_cam), out(3 * hw), out2(3 * hw);
  std::vector<double> scratch((size_t)imghead::workgroups((int64_t)hw) * SUMS);
  std::vector<uint8_t> u8(3 * hw), u8b(3 * hw);
  ih_forward(render.data(), mask.data(), cam_m.data(), cam_c.data(), n_cam, cam, H, W, image.data());
  for (float v : image) if (!(v >= 0.f && v <= 1.f)) return 2;
  ih_backward(render.data(), mask.data(), cam_m.data(), cam_c.data(), n_cam, cam, H, W, g.data(), scratch.data(), d_render.data(), d_mask.data(),
              d_cam_m.data(), d_cam_c.data());
  for (float v : d_render) if (!std::isfinite(v)) return 3;
  for (float v : d_mask) if (!std::isfinite(v)) return 4;
  for (int i = 0; i < 3 * n_cam; ++i)
    if (i / 3 != cam && (d_cam_m[i] != 0.f || d_cam_c[i] != 0.f)) return 5;
  // each output alone, the others NULL; without cam gradients no scratch either
  ih_backward(render.data(), mask.data(), cam_m.data(), cam_c.data(), n_cam, cam, H, W, g.data(), nullptr, d_render.data(), nullptr, nullptr, nullptr);
  ih_backward(render.data(), mask.data(), cam_m.data(), cam_c.data(), n_cam, cam, H, W, g.data(), nullptr, nullptr, d_mask.data(), nullptr, nullptr);
  ih_backward(render.data(), mask.data(), cam_m.data(), cam_c.data(), n_cam, cam, H, W, g.data(), scratch.data(), nullptr, nullptr, d_cam_m.data(), nullptr);
  ih_backward(render.data(), mask.data(), cam_m.data(), cam_c.data(), n_cam, cam, H, W, g.data(), scratch.data(), nullptr, nullptr, nullptr, d_cam_c.data());
  // no upstream gradient: zeros everywhere
  ih_backward(render.data(), mask.data(), cam_m.data(), cam_c.data(), n_cam, cam, H, W, nullptr, scratch.data(), d_render.data(), d_mask.data(),
              d_cam_m.data(), d_cam_c.data());
  for (float v : d_render) if (v != 0.f) return 6;
  for (float v : d_mask) if (v != 0.f) return 7;
  for (float v : d_cam_m) if (v != 0.f) return 8;
  for (float v : d_cam_c) if (v != 0.f) return 9;
  // the evaluation side, with and without the affine
  for (int white = 0; white < 2; ++white) {
    ih_bytes(render.data(), mask.data(), cam_m.data(), cam_c.data(), n_cam, cam, white, H, W, u8.data());
    ih_bytes(render.data(), mask.data(), nullptr, nullptr, 0, 0, white, H, W, u8b.data());
    ih_compose(render.data(), mask.data(), white, H, W, out.data());
    ih_eval_pair(u8.data(), u8b.data(), mask.data(), white, H, W, out.data(), out2.data());
    for (float v : out) if (!(v >= 0.f && v <= 1.f)) return 10;
  }
  return 0;
}

bool read_floats(FILE *fp, std::vector<float> &v, size_t n) {
  v.resize(n);
  return std::fread(v.data(), 4, n, fp) == n;
}

}  // namespace

// each argument: a file of int32 H, W, n_cam, cam, then float render [3 H W], mask [H W], cam_m [n_cam 3], cam_c [n_cam 3], g [3 H W]
int main(int argc, char **argv) {
  long pixels = 0;
  for (int i = 1; i < argc; ++i) {
    FILE *fp = std::fopen(argv[i], "rb");
    if (!fp) return 20;
    int32_t hdr[4];
    if (std::fread(hdr, 4, 4, fp) != 4) return 21;
    const size_t hw = (size_t)hdr[0] * hdr[1];
    std::vector<float> render, mask, cam_m, cam_c, g;
    if (!read_floats(fp, render, 3 * hw) || !read_floats(fp, mask, hw) || !read_floats(fp, cam_m, 3 * (size_t)hdr[2]) ||
        !read_floats(fp, cam_c, 3 * (size_t)hdr[2]) || !read_floats(fp, g, 3 * hw))
      return 22;
    std::fclose(fp);
    if (int rc = run(hdr[0], hdr[1], hdr[2], hdr[3], render, mask, cam_m, cam_c, g)) { std::printf("FAILED %d in %s\n", rc, argv[i]); return rc; }
    pixels += (long)hw;
  }
  // no pixel at all: nothing is read or written but the two [n_cam, 3] outputs, which are zero
  const std::vector<float> none, cam_m = {0.1f, -0.2f, 0.3f, 0.f, 0.f, 0.f}, cam_c = {0.01f, 0.02f, 0.03f, 0.f, 0.f, 0.f};
  if (int rc = run(0, 7, 2, 0, none, none, cam_m, cam_c, none)) { std::printf("FAILED %d with no pixel\n", rc); return rc; }
  std::printf("ok: %d cases, %ld pixels, and a call without a pixel\n", argc - 1, pixels);
  return 0;
}
#endif
