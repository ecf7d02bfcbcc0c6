"""The forward rasteriser without a GPU: mpmavatar_amd/csrc/raster_math.hpp compiled with g++ (tests/hostraster/hostraster.cpp, the
way tests/test_geo_metrics.py compiles geo_math.hpp) against the float64 twin (tests/raster_twin.py) and against the fixture the
reference's own camera and SH functions produced (tests/golden/raster.npz); the conditions the committed scenes must meet for the
GPU comparison (tests/test_gpu_raster.py) to be exact where it claims to be; and the host side of the Python layer."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import raster_scenes as rs
import raster_twin as tw
from hostbuild import host_lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EPS = 2.0 ** -24

fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def hr():
    return host_lib("hostraster")


def _p(a, t=fp):
    return None if a is None else a.ctypes.data_as(t)


def preprocess(hr, cam, means3D, scales=None, rotations=None, cov6=None, shs=None, sh_degree=0, colors_precomp=None, mod=1.0, **_):
    c32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    means3D, scales, rotations, cov6, shs, colors_precomp = map(c32, (means3D, scales, rotations, cov6, shs, colors_precomp))
    n = means3D.shape[0]
    out_f, out_i = np.empty((n, 9), np.float32), np.empty((n, 5), np.int32)
    view, proj, campos = c32(cam.viewmatrix), c32(cam.projmatrix), c32(cam.campos)
    hr.hr_preprocess(n, _p(means3D), _p(scales), _p(rotations), C.c_float(mod), _p(cov6), _p(shs), 0 if shs is None else shs.shape[1],
                     sh_degree, _p(colors_precomp), _p(view), _p(proj), _p(campos), cam.image_width, cam.image_height,
                     C.c_float(cam.tanfovx), C.c_float(cam.tanfovy), _p(out_f), _p(out_i, ip))
    return out_f, out_i


def blend(hr, seq):
    rows = np.zeros((len(seq), 10), np.float32)
    for j, (dx, dy, A, B, Cc, op, col) in enumerate(seq):
        rows[j, :6], rows[j, 6:9] = (dx, dy, A, B, Cc, op), col
    out = np.empty(4, np.float32)
    hr.hr_blend.restype = C.c_int
    k = hr.hr_blend(len(seq), _p(rows), _p(out))
    return k, out


# ---- the committed scenes meet the conditions of the comparison -----------------------------------------------------------------

@pytest.mark.parametrize("key", rs.COMPARED, ids=lambda k: "-".join(map(str, k)))
def test_committed_scene_conditions(key):
    cam, sc, r64, r32 = rs.twins(*key)
    vis = r64.radii > 0
    raw = r64.splats.radius_raw[vis]
    assert np.abs(raw - np.round(raw)).min() > 1e-5           # 3 sqrt(lambda) nowhere near an integer: radii must match exactly
    assert np.array_equal(r64.radii, r32.radii)
    assert np.array_equal(r64.splats.rect[vis], r32.splats.rect[vis])
    d = np.sort(r64.splats.depth[vis])
    assert (np.diff(d) / d[1:]).min() > 1e-4                  # no two view depths closer than 1e-4 relative
    assert np.array_equal(r64.order, r32.order)
    if key[0] == "random":
        n = vis.size
        assert 0.15 * n < (~vis).sum() < 0.35 * n             # about a quarter outside the frustum or behind the camera
        assert r64.max_tile_entries > 256                     # the batch loop of the render kernel runs more than once
    if key[0] == "thin":
        assert vis.all() and r64.max_tile_entries == 700 and r64.alpha.max() < 1 - 1e-4     # T never saturates
    if key[0] == "front":
        only = tw.render(cam, rs.BG, **{k: v[:rs.n_front()] for k, v in sc.items()})
        assert np.array_equal(only.image, r64.image)          # no later layer shows
        assert r64.alpha.min() > 1 - 1e-3


def test_e32_and_the_left_out_share():
    """E32 = max |twin32 - twin64| over the compared pixels of the committed scenes; the constant in raster_scenes.py is this
    measurement, rounded up.  At most 1 % of a scene's pixels are left out."""
    worst = 0.0
    for key in rs.COMPARED:
        cam, sc, r64, r32 = rs.twins(*key)
        m = rs.compared_mask(r64, r32)
        share = 1.0 - m.mean()
        e = max(np.abs(r32.image - r64.image)[:, m].max(), np.abs(r32.alpha - r64.alpha)[:, m].max())
        print(key, "E32 = %.3g, left out %d of %d pixels (%.2f %%)" % (e, (~m).sum(), m.size, 100 * share))
        assert share <= rs.MAX_LEFT_OUT_SHARE
        worst = max(worst, e)
    assert 0.5 * rs.E32 < worst <= rs.E32
    assert rs.BOUND == 10 * rs.E32


# ---- raster_math.hpp on the host against the twin and the fixture ---------------------------------------------------------------

@pytest.mark.parametrize("k", (0, 1))
def test_projection_conic_radius_rectangle_against_float64(hr, k):
    cam, sc, r64, _ = rs.twins("random", k, 0)
    f, i = preprocess(hr, cam, **sc)
    sp = r64.splats
    assert np.array_equal(i[:, 0], r64.radii)
    vis = r64.radii > 0
    assert np.array_equal(i[vis, 1:], sp.rect[vis])
    # a pixel centre is a ratio of two 4-term dot products times W/2: relative 2^-24 steps on values of image size
    scale = max(cam.image_width, cam.image_height)
    assert np.abs(f[vis, 0] - sp.px[vis]).max() < 64 * EPS * scale and np.abs(f[vis, 1] - sp.py[vis]).max() < 64 * EPS * scale
    assert np.abs(f[vis, 5] - sp.depth[vis]).max() < 16 * EPS * 5
    # conic: three 3x3 products and a 2x2 inverse; the condition number of the inverse is lambda_max / lambda_min <= (a + c)^2 / det
    a_c = (sp.conic[vis, 0] + sp.conic[vis, 2])
    cond = a_c ** 2 / (sp.conic[vis, 0] * sp.conic[vis, 2] - sp.conic[vis, 1] ** 2)
    err = np.abs(f[vis, 2:5] - sp.conic[vis]).max(1)
    assert (err <= 256 * EPS * cond * np.abs(sp.conic[vis]).max(1)).all()


def test_cameras_are_the_reference_s(hr):
    """One point through both fixture cameras: the pixel centre the reference's matrices give (row vector times full_proj_transform,
    perspective divide) -- for camera 1 also straight from its intrinsics, u = fx x / z + cx - 0.5."""
    for k in (0, 1):
        cam = rs.fixture_camera(k)
        V = cam.viewmatrix.astype(np.float64)
        p = ((np.array([[0.2, -0.1, 2.5]]) - V[3, :3]) @ np.linalg.inv(V[:3, :3])).astype(np.float32)      # in front of the camera
        f, i = preprocess(hr, cam, p, scales=np.full((1, 3), 0.05, np.float32), rotations=np.array([[1, 0, 0, 0]], np.float32),
                          colors_precomp=np.zeros((1, 3), np.float32))
        h = np.append(p[0].astype(np.float64), 1.0) @ cam.projmatrix.astype(np.float64)
        want = ((h[:2] / h[3] + 1) * np.array([cam.image_width, cam.image_height]) - 1) / 2
        assert i[0, 0] > 0 and np.abs(f[0, :2] - want).max() < 1e-4
        if k == 1:
            w2c, K = rs.GOLD["cam1_w2c"], rs.GOLD["cam1_k"]
            c = w2c[:3, :3] @ p[0].astype(np.float64) + w2c[:3, 3]
            u = np.array([K[0, 0] * c[0] / c[2] + K[0, 2], K[1, 1] * c[1] / c[2] + K[1, 2]]) - 0.5
            assert np.abs(f[0, :2] - u).max() < 1e-4
        assert np.allclose(cam.campos, -cam.viewmatrix[3, :3] @ np.linalg.inv(cam.viewmatrix[:3, :3]), atol=1e-6)


@pytest.mark.parametrize("deg", (0, 1, 2, 3))
def test_sh_colour_against_the_reference(hr, deg):
    g = rs.GOLD
    cam = rs.fixture_camera(0)._replace(campos=g["sh_campos"])
    n = g["sh_positions"].shape[0]
    f, _ = preprocess(hr, cam, g["sh_positions"], scales=np.full((n, 3), 0.05, np.float32),
                      rotations=np.tile(np.array([[1, 0, 0, 0]], np.float32), (n, 1)), shs=g["sh_coeffs"], sh_degree=deg)
    want = g[f"sh_colors_deg{deg}"]
    # (deg + 1)^2 terms |C_k poly_k(dir)| <= 3 each, times the coefficient, summed in fp32
    bound = 64 * EPS * (0.5 + 3.0 * np.abs(g["sh_coeffs"][:, :(deg + 1) ** 2]).sum(1))
    assert (np.abs(f[:, 6:9] - want) <= bound).all()
    assert np.abs(tw.eval_sh_colour(deg, g["sh_coeffs"], g["sh_positions"], g["sh_campos"]) - want).max() < 1e-12
    assert (want == 0).any() or deg == 0                       # the clamp is exercised


def test_cov3d_precomp_is_the_scale_rotation_covariance(hr):
    cam, sc, r64, _ = rs.twins("random", 0, 0)
    cov = tw.cov3d(sc["scales"], sc["rotations"], 1.0).astype(np.float32)
    f1, i1 = preprocess(hr, cam, **sc)
    f2, i2 = preprocess(hr, cam, sc["means3D"], cov6=cov, colors_precomp=sc["colors_precomp"])
    assert np.array_equal(i1, i2)
    vis = i1[:, 0] > 0
    assert np.allclose(f1[vis], f2[vis], rtol=1e-4, atol=1e-6)


def test_blend_against_the_twin_on_recorded_sequences(hr):
    for key, pix in ((("random", 0, 0), (24, 24)), (("random", 1, 1), (20, 30)), (("thin",), (7, 9)), (("front",), (3, 12))):
        cam, sc, r64, _ = rs.twins(*key)
        _, seq = tw.render(cam, rs.BG, record=pix, **sc)
        assert len(seq) > (256 if key[0] == "thin" else 2) and not r64.near[pix]
        k, out = blend(hr, seq)
        T = 1.0 - r64.alpha[0][pix]
        assert abs(out[0] - T) <= rs.BOUND
        want = r64.image[(slice(None),) + pix] - T * rs.BG
        assert np.abs(out[1:] - want).max() <= rs.BOUND
        if key[0] == "front":
            assert k == 2                                       # finished when offered the third entry; 700 more were never looked at


# ---- known answers ---------------------------------------------------------------------------------------------------------------

def _one_gaussian(hr, opacity, sigma_px):
    """an isotropic Gaussian exactly on the centre of pixel (8, 8) of a 16 x 16 image (simple camera: focal 16 pixels)"""
    cam = tw.simple_camera(16, 16)
    z = 2.0
    mean = np.array([[(8 + 0.5 - 8) * z / 16.0, (8 + 0.5 - 8) * z / 16.0, z]], np.float32)     # px = 16 x / z + 7.5
    s = sigma_px * z / 16.0
    f, i = preprocess(hr, cam, mean, scales=np.full((1, 3), s, np.float32), rotations=np.array([[1, 0, 0, 0]], np.float32),
                      colors_precomp=np.array([[0.2, 0.5, 0.9]], np.float32))
    assert i[0, 0] > 0 and abs(f[0, 0] - 8.0) < 1e-5 and abs(f[0, 1] - 8.0) < 1e-5
    return f[0]


@pytest.mark.parametrize("opacity", (0.6, 1.0))
def test_one_isotropic_gaussian_on_a_pixel_centre(hr, opacity):
    sigma = 3.0
    f = _one_gaussian(hr, opacity, sigma)
    col = np.array([0.2, 0.5, 0.9])
    # off-axis distortion of the Jacobian at 0.5 px from the principal point is O((0.5 / 16)^2): the conic is 1 / (sigma^2 + 0.3)
    var = sigma ** 2 + 0.3
    assert abs(f[2] - 1 / var) < 2e-3 / var and abs(f[4] - 1 / var) < 2e-3 / var and abs(f[3]) < 1e-3 / var
    for dx, dy in ((0.0, 0.0), (1.0, 0.0), (0.0, -1.0)):
        k, out = blend(hr, [(dx, dy, f[2], f[3], f[4], opacity, col)])
        a = min(0.99, opacity * np.exp(-0.5 * (f[2] * dx * dx + f[4] * dy * dy)))
        assert k == 1 and abs(out[0] - (1 - a)) < 4 * EPS and np.abs(out[1:] - a * col).max() < 4 * EPS
        if dx == dy == 0.0:
            assert abs((1 - out[0]) - min(0.99, opacity)) < 2 * EPS              # alpha = min(0.99, opacity) at the centre
            image = out[1:] + out[0] * rs.BG
            assert np.abs(image - (min(0.99, opacity) * col + (1 - min(0.99, opacity)) * rs.BG)).max() < 4 * EPS


def test_opaque_layers_hide_what_lies_behind(hr):
    """alpha 0.99 leaves T = 0.01, alpha 0.9 then T = 1e-3; a third opaque layer would leave 1e-5 < 1e-4: the pixel is finished
    BEFORE it is added, and whatever follows is never looked at."""
    flat = lambda op, col: (0.0, 0.0, 0.1, 0.0, 0.1, op, np.array(col, np.float64))
    seq = [flat(1.0, (1, 0, 0)), flat(0.9, (0, 1, 0)), flat(1.0, (0, 0, 1)), flat(0.5, (1, 1, 1))]
    k, out = blend(hr, seq)
    assert k == 2
    assert abs(out[0] - 1e-3) < 1e-8 and np.abs(out[1:] - np.array([0.99, 0.01 * 0.9, 0.0])).max() < 1e-7
    k, out = blend(hr, seq[:2] + [flat(0.5, (0, 0, 1))])        # 1e-3 * 0.5 stays above 1e-4: added
    assert k == 3 and abs(out[3] - 0.5 * 1e-3) < 1e-8


def test_culls(hr):
    cam = tw.simple_camera(16, 16)
    iso = lambda v: [v, 0, 0, v, 0, v]
    means = np.array([[0, 0, 0.2], [0, 0, 0.1], [0, 0, -3], [40, 0, 2], [0, -40, 2], [0, 0, 2], [0, 0, 2]], np.float32)
    cov = np.array([iso(0.01)] * 5 + [[2.0 ** 34, 2.0 ** 34, 0, 2.0 ** 34, 0, 0], iso(0.01)], np.float32)
    _, i = preprocess(hr, cam, means, cov6=cov, colors_precomp=np.zeros((7, 3), np.float32))
    assert (i[:6, 0] == 0).all()          # z <= 0.2 (three), off-screen by more than the radius (two), det == 0 in fp32 (one)
    assert i[6, 0] > 0                    # the control


# ---- the Python layer ------------------------------------------------------------------------------------------------------------

def test_python_layer_imports_without_a_gpu_and_has_the_reference_s_names():
    from mpmavatar_amd import rasterizer as R
    assert R.GaussianRasterizationSettings._fields == ("image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier",
                                                       "viewmatrix", "projmatrix", "sh_degree", "campos", "prefiltered", "debug")
    assert "train_appearance.py" in R.__doc__ and "forward" in R.__doc__.lower()
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "mpmavatar_amd", "compat")]))
    code = ("from diff_gauss import GaussianRasterizationSettings, GaussianRasterizer\n"      # gaussian_renderer/__init__.py:14
            "import mpmavatar_amd.rasterizer as R\n"
            "assert GaussianRasterizer is R.GaussianRasterizer and GaussianRasterizationSettings is R.GaussianRasterizationSettings\n"
            "print('ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=os.path.join(ROOT, "tests"), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


def test_header_cites_the_reference_lines_of_the_rasteriser():
    header = open(os.path.join(ROOT, "include", "mpmhip.h")).read()
    for cite in ("gaussian_renderer/__init__.py:36-49", "gaussian_renderer/__init__.py:95-103", "utils/sh_utils.py:57-100",
                 "scene/cameras.py:26-39"):
        assert cite in header


def _decode_png(path):
    """8-bit RGB, filter 0 on every row -- the only form io_formats.write_png writes -- with nothing but zlib"""
    import struct
    import zlib
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(data):
        n, tag = struct.unpack(">I", data[at:at + 4])[0], data[at + 4:at + 8]
        body = data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF, tag
        chunks.append((tag, body))
        at += 12 + n
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(h, 1 + 3 * w)
    assert (raw[:, 0] == 0).all()
    return raw[:, 1:].reshape(h, w, 3)


def test_write_png_round_trips_pixels_and_rounding(tmp_path):
    from mpmavatar_amd import io_formats
    rng = np.random.default_rng(8)
    img = rng.random((3, 5, 7)).astype(np.float32)
    img[:, 0, 0] = [0.0, 1.0, 0.5]                       # 0, 255, 128 (127.5 + 0.5 truncated)
    img[:, 0, 1] = [-0.3, 1.7, 100.4 / 255.0]            # clamped to 0 and 255; 100.4 -> 100
    img[:, 0, 2] = [100.6 / 255.0, 254.49 / 255.0, 254.51 / 255.0]
    path = io_formats.write_png(str(tmp_path / "sub" / "a.png"), img)
    px = _decode_png(path)
    assert px.shape == (5, 7, 3)
    assert px[0, 0].tolist() == [0, 255, 128] and px[0, 1].tolist() == [0, 255, 100] and px[0, 2].tolist() == [101, 254, 255]
    want = np.floor(np.clip(img.astype(np.float64), 0, 1) * 255.0 + 0.5).transpose(1, 2, 0)
    assert np.abs(px.astype(np.float64) - want).max() <= 1 and (px == want).mean() > 0.99     # fp32 product: a tie may round either way
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:                                # an independent decoder, where there is one
        assert np.array_equal(np.asarray(Image.open(path).convert("RGB")), px)
    with pytest.raises(ValueError):
        io_formats.write_png(str(tmp_path / "b.png"), np.zeros((5, 7, 3), np.float32))
