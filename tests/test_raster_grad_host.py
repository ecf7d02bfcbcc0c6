"""The rasteriser's backward pass without a GPU: mpmavatar_amd/csrc/raster_grad_math.hpp compiled with g++
(tests/hostraster_grad/hostraster_grad.cpp, a serial statement of the whole pipeline) against the gradient autograd takes of the
float64 torch twin (tests/raster_twin_torch.py); the measurement of G32, the constant the GPU bound is built on; the conditions
the committed scenes must meet; torch.autograd.gradcheck of the twin as an anchor independent of our derivation; a known answer."""
import ctypes as C
import numpy as np
import pytest
import torch

import raster_grad_scenes as gs
import raster_scenes as rs
import raster_twin as tw
import raster_twin_torch as tt
from hostbuild import host_lib

fp = C.POINTER(C.c_float)
IDS = lambda k: "-".join(map(str, k))


@pytest.fixture(scope="module")
def hg():
    so = host_lib("hostraster_grad")
    so.hg_backward.restype = C.c_int64
    return so


def host_backward(hg, cam, sc, Wi, Wa, sh_degree=0, mod=1.0, bg=rs.BG):
    """-> dict of gradients (the names of the rasteriser's arguments), image, alpha"""
    c32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    p = lambda a: None if a is None else a.ctypes.data_as(fp)
    a = {k: c32(sc.get(k)) for k in ("means3D", "opacities", "scales", "rotations", "cov3Ds_precomp", "shs", "colors_precomp")}
    n = a["means3D"].shape[0]
    n_sh = 0 if a["shs"] is None else a["shs"].shape[1]
    out = {"means3D": np.full((n, 3), np.nan, np.float32), "means2D": np.full((n, 3), np.nan, np.float32),
           "opacities": np.full(a["opacities"].shape, np.nan, np.float32)}
    if a["cov3Ds_precomp"] is None:
        out["scales"], out["rotations"] = np.full((n, 3), np.nan, np.float32), np.full((n, 4), np.nan, np.float32)
    else:
        out["cov3Ds_precomp"] = np.full((n, 6), np.nan, np.float32)
    if a["shs"] is None:
        out["colors_precomp"] = np.full((n, 3), np.nan, np.float32)
    else:
        out["shs"] = np.full((n, n_sh, 3), np.nan, np.float32)
    H, W = cam.image_height, cam.image_width
    image, alpha = np.empty((3, H, W), np.float32), np.empty((1, H, W), np.float32)
    view, proj, campos, bg = c32(cam.viewmatrix), c32(cam.projmatrix), c32(cam.campos), c32(bg)
    Wi, Wa = c32(Wi), c32(Wa)
    hg.hg_backward(n, p(a["means3D"]), p(a["opacities"]), p(a["scales"]), p(a["rotations"]), C.c_float(mod), p(a["cov3Ds_precomp"]),
                   p(a["shs"]), n_sh, sh_degree, p(a["colors_precomp"]), p(view), p(proj), p(campos), W, H, C.c_float(cam.tanfovx),
                   C.c_float(cam.tanfovy), p(bg), p(Wi), p(Wa), p(out["means3D"]), p(out["means2D"]), p(out["opacities"]),
                   p(out.get("scales")), p(out.get("rotations")), p(out.get("cov3Ds_precomp")), p(out.get("shs")),
                   p(out.get("colors_precomp")), p(image), p(alpha))
    return out, image, alpha


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------

def test_g32_and_the_left_out_share():
    """G32 = worst relative error of the float32 torch twin's gradients against the float64 twin's over the committed scenes; the
    constant in raster_grad_scenes.py is this measurement, rounded up.  At most 1 % of a scene's pixels carry no weight."""
    worst = 0.0
    for key in rs.COMPARED:
        cam, sc, Wi, Wa, g64, g32, share, r64, r32 = gs.scene_grads(*key)
        errs = {k: gs.rel_err(g32[k], g64[k]) for k in g64 if np.abs(g64[k]).max() > 0}
        print(key, "left out %.2f %%;" % (100 * share), ", ".join("%s %.3g" % kv for kv in errs.items()))
        assert share <= gs.MAX_LEFT_OUT_SHARE
        worst = max(worst, max(errs.values()))
    print("G32 measured %.4g, committed %.4g" % (worst, gs.G32))
    assert 0.5 * gs.G32 < worst <= gs.G32
    assert gs.BOUND_G == 10 * gs.G32


@pytest.mark.parametrize("key", rs.COMPARED, ids=IDS)
def test_committed_scenes_keep_clear_of_the_clamps(key):
    cam, sc, Wi, Wa, g64, g32, share, r64, r32 = gs.scene_grads(*key)
    assert r64.clamp_margin > gs.CLAMP_MARGIN and r32.clamp_margin > gs.CLAMP_MARGIN
    if key[0] == "front":
        # the bound alpha clamp is exercised: the first Gaussian is clamped on all 256 pixels, well away from the threshold
        raw = sc["opacities"][0, 0] * np.exp(-0.5 * 2 * 16.0 ** 2 / (r64.base.splats.conic[0, 0] ** -1))
        assert raw > 0.99 * (1 + 1e-3)
        assert np.abs(g64["opacities"][0]).max() == 0.0 and np.abs(g64["colors_precomp"][0]).max() > 0.0


@pytest.mark.parametrize("deg", (0, 1, 2, 3))
def test_sh_scene_keeps_clear_of_the_clamps(deg):
    cam, sc, Wi, Wa, g64, g32, share, r64, r32 = gs.sh_grads(deg)
    assert r64.clamp_margin > gs.CLAMP_MARGIN and r32.clamp_margin > gs.CLAMP_MARGIN and share <= gs.MAX_LEFT_OUT_SHARE
    assert (r64.base.radii > 0).sum() > 20


@pytest.mark.parametrize("key", rs.COMPARED, ids=IDS)
def test_float64_torch_twin_is_the_numpy_twin(key):
    cam, sc, Wi, Wa, g64, g32, share, r64, r32 = gs.scene_grads(*key)
    _, _, n64, _ = rs.twins(*key)
    assert np.abs(r64.image.detach().numpy() - n64.image).max() < 1e-12
    assert np.abs(r64.alpha.detach().numpy() - n64.alpha).max() < 1e-12


# ---- raster_grad_math.hpp on the host against the float64 twin ------------------------------------------------------------------

@pytest.mark.parametrize("key", rs.COMPARED, ids=IDS)
def test_host_backward_against_float64(hg, key):
    cam, sc, Wi, Wa, g64, g32, share, r64, r32 = gs.scene_grads(*key)
    got, image, alpha = host_backward(hg, cam, sc, Wi, Wa)
    m = ~(r64.near | r32.near)
    assert np.abs(image - r64.image.detach().numpy())[:, m].max() <= rs.BOUND          # the driver's forward is the forward
    gs.check_grads(got, g64, IDS(key))
    if key[0] == "front":
        for k, g in got.items():
            assert (g[rs.n_front():] == 0).all(), k                                    # the hidden layers: exactly zero


@pytest.mark.parametrize("deg", (0, 1, 2, 3))
def test_host_backward_sh_path(hg, deg):
    cam, sc, Wi, Wa, g64, g32, share, r64, r32 = gs.sh_grads(deg)
    got, _, _ = host_backward(hg, cam, sc, Wi, Wa, sh_degree=deg)
    gs.check_grads(got, g64, f"sh degree {deg}")
    assert (got["shs"][:, (deg + 1) ** 2:] == 0).all()
    if deg > 0:
        # the view-direction path into means3D is there: without it the gradient differs
        plain = tt.render(cam, rs.BG, dtype=np.float64, **{**{k: v for k, v in sc.items() if k != "shs"},
                                                            "colors_precomp": r64.base.colours})
        assert gs.rel_err(tt.gradients(plain, Wi, Wa)["means3D"], g64["means3D"]) > 100 * gs.BOUND_G


def test_host_backward_cov3d_precomp_path(hg):
    cam, sc, Wi, Wa, g64, g32, share, r64, r32 = gs.precomp_grads()
    got, _, _ = host_backward(hg, cam, sc, Wi, Wa)
    gs.check_grads(got, g64, "cov3Ds_precomp")
    assert np.abs(g64["cov3Ds_precomp"][:, [1, 2, 4]]).max() > 0


# ---- anchors independent of our derivation -----------------------------------------------------------------------------------------

def _small_scene():
    cam = tw.simple_camera(16, 16)
    rng = np.random.default_rng(3)
    n = 6
    z = np.linspace(1.5, 3.0, n)
    means = np.stack([rng.uniform(-0.3, 0.3, n) * z, rng.uniform(-0.3, 0.3, n) * z, z], 1)
    return cam, dict(means3D=means, opacities=rng.uniform(0.3, 0.8, (n, 1)), colors_precomp=rng.uniform(0, 1, (n, 3)),
                     scales=rng.uniform(0.15, 0.4, (n, 3)), rotations=rng.normal(size=(n, 4)))


def _gradcheck(cam, sc, names, sh_degree=0):
    Wi, Wa = (torch.tensor(w) for w in gs.weights(16, 16))
    first = tt.render(cam, rs.BG, dtype=np.float64, sh_degree=sh_degree, **sc)
    assert not first.near.any() and (first.base.radii > 0).all() and first.alpha.max() > 0.5 and first.clamp_margin > 1e-3

    def loss(*ts):
        d = dict(sc, **{k: t.detach().numpy() for k, t in zip(names, ts)})
        r = tt.render(cam, rs.BG, dtype=np.float64, sh_degree=sh_degree, leaves=dict(zip(names, ts)), **d)
        assert np.array_equal(r.base.radii, first.base.radii) and np.array_equal(r.base.order, first.base.order)   # decisions held
        return (Wi * r.image).sum() + (Wa * r.alpha).sum()

    ts = [torch.tensor(np.asarray(sc[k], np.float64), requires_grad=True) for k in names]
    assert torch.autograd.gradcheck(loss, ts, eps=1e-6, atol=1e-6, rtol=1e-5)


def test_gradcheck_of_the_float64_twin():
    """torch.autograd.gradcheck (finite differences of the twin's own forward) on a 16 x 16 scene of six Gaussians, no decision
    of which is near a threshold: the twin's gradient is the derivative of its forward function with the decisions held fixed."""
    cam, sc = _small_scene()
    _gradcheck(cam, sc, ["means3D", "opacities", "colors_precomp", "scales", "rotations"])


def test_gradcheck_of_the_sh_and_precomp_paths():
    cam, sc = _small_scene()
    rng = np.random.default_rng(5)
    sc = {k: v for k, v in sc.items() if k not in ("scales", "rotations", "colors_precomp")}
    sc["cov3Ds_precomp"] = tw.cov3d(rng.uniform(0.15, 0.4, (6, 3)), rng.normal(size=(6, 4)), 1.0)
    sc["shs"] = rng.normal(0, 0.3, (6, 16, 3))
    cam = cam._replace(campos=np.array([0.3, -0.2, -0.5], np.float32))
    _gradcheck(cam, sc, ["means3D", "cov3Ds_precomp", "shs"], sh_degree=3)


def test_one_isotropic_gaussian_on_a_pixel_centre_has_d_image_d_colour_alpha(hg):
    cam = tw.simple_camera(16, 16)
    z, opacity = 2.0, 0.6
    sc = dict(means3D=np.array([[0.5 * z / 16.0, 0.5 * z / 16.0, z]], np.float32), opacities=np.array([[opacity]], np.float32),
              colors_precomp=np.array([[0.2, 0.5, 0.9]], np.float32), scales=np.full((1, 3), 3.0 * z / 16.0, np.float32),
              rotations=np.array([[1, 0, 0, 0]], np.float32))
    Wi, Wa = np.zeros((3, 16, 16), np.float32), np.zeros((1, 16, 16), np.float32)
    Wi[1, 8, 8] = 1.0                                           # L = the green value of the pixel the Gaussian is centred on
    got, image, alpha = host_backward(hg, cam, sc, Wi, Wa)
    assert abs(alpha[0, 8, 8] - opacity) < 1e-6                 # alpha = opacity at the centre
    assert np.abs(got["colors_precomp"][0] - np.array([0.0, opacity, 0.0])).max() < 1e-6
    # d image / d opacity = (colour - bg) exp(0)
    assert abs(got["opacities"][0, 0] - (0.5 - rs.BG[1])) < 1e-5
    Wi[:], Wa[0, 8, 8] = 0.0, 1.0                               # L = alpha of that pixel: d / d opacity = 1
    got, _, _ = host_backward(hg, cam, sc, Wi, Wa)
    assert abs(got["opacities"][0, 0] - 1.0) < 1e-5 and (got["colors_precomp"] == 0).all()
