"""The tables, the yardstick and the constants shared by tests/test_raster_extra_host.py and tests/test_gpu_raster_extra.py: the
rasteriser's extra attribute channels (mpmavatar_amd/csrc/raster_extra_math.hpp, raster_extra.hip).

THE YARDSTICK NEEDS NO NEW MATH.  extra_e = sum_k a_ke alpha_k T_k is the colour formula over a zero background, so the extras are
rendered through the existing twin (tests/raster_twin_torch.py) as colours, in groups of three channels padded with zeros, and the
gradients of L = sum Wi image + sum Wa alpha + sum Wx extra are the sum of raster_twin_torch.gradients() of the colour render and
of the padded renders: colors_precomp (or shs) takes the colour render's alone, extra_attrs the padded renders' colour gradients.
The weights are zero on every pixel that any of the renders, float64 or float32, marks near a threshold; the geometry is the same
in all of them, so the set is the colour render's own.  Each case is computed once (functools.lru_cache) and never modified.
Test infrastructure only."""
import ctypes as C
import functools
from typing import NamedTuple

import numpy as np

import hostbuild
import raster_grad_scenes as gs
import raster_scenes as rs
import raster_twin_torch as tt

# Measured on the CPU over raster_scenes.COMPARED with the seeded [N, 2] table and the combined loss below, over all gradient tensors,
# extra_attrs included (tests/test_raster_extra_host.py::test_g32x_and_the_left_out_share asserts it): G32X = max over scenes and
# tensors of max |g32 - g64| / max |g64|, float32 twin against float64.  The code under test plays no part in it.  The device and the
# host restatement must lie within BOUND_GX = 10 * G32X of the float64 twin: the project's factor, for the reasons given at
# raster_grad_scenes.py:17-19.  The forward goes against raster_scenes.BOUND.
G32X = 4.2e-6   # measured 4.15e-6 (rotations, odd 9 x 70); the other tensors and scenes 8.1e-8 .. 4.0e-6; extra_attrs at most 1.6e-6
BOUND_GX = 10 * G32X
E_REF = 2                       # the reference's table: upper and lower garment
E_OTHER = (1, 3, 5, 8)          # one scene each: a single channel, a full group, a partial second group, the most
OTHER_SCENE = ("odd", 33, 17)   # 300 Gaussians, 3 x 2 tiles, lanes outside the image


def table(n, E, seed=7):
    """[n, E] float32: channel 0 is a 0 / 1 labelling (the reference's garment table holds only such), the others uniform in [0, 1)"""
    rng = np.random.default_rng(3000 + seed)
    t = rng.uniform(0.0, 1.0, (n, E))
    t[:, 0] = rng.random(n) < 0.5
    return t.astype(np.float32)


def pad(a, axis=1):
    """the channels in groups of three, the last group padded with zeros -> list of arrays with 3 along `axis`"""
    a = np.moveaxis(np.asarray(a), axis, 0)
    groups = []
    for k in range(0, a.shape[0], 3):
        g = np.zeros((3,) + a.shape[1:], a.dtype)
        g[:a[k:k + 3].shape[0]] = a[k:k + 3]
        groups.append(np.ascontiguousarray(np.moveaxis(g, 0, axis)))
    return groups


def weights_extra(E, h, w, seed=2025):
    return np.random.default_rng(seed).normal(size=(E, h, w))


class Case(NamedTuple):
    cam: object
    sc: dict
    extra: np.ndarray     # [n, E] float32
    Wi: np.ndarray        # float32 weights with the near pixels zeroed (zero altogether when the loss leaves the output out)
    Wa: np.ndarray
    Wx: np.ndarray
    g64: dict             # gradients of the float64 twin by argument name, "extra_attrs" among them
    g32: dict
    share: float          # share of the pixels left out
    near: np.ndarray      # [H, W] bool
    image64: np.ndarray   # the float64 twin's outputs
    alpha64: np.ndarray
    extra64: np.ndarray   # [E, H, W]
    radii: np.ndarray
    colour_only64: dict   # gradients of the colour render alone (the composition rule's first term)


def _renders(cam, sc, extra, dtype, sh_degree):
    colour = tt.render(cam, rs.BG, dtype=dtype, sh_degree=sh_degree, **sc)
    geometry = {k: v for k, v in sc.items() if k not in ("colors_precomp", "shs")}
    padded = [tt.render(cam, np.zeros(3), dtype=dtype, colors_precomp=g, **geometry) for g in pad(extra)]
    return colour, padded


def _compose(colour, padded, Wi, Wa, Wx, E):
    """gradients of the combined loss: gradients() of the colour render plus gradients() of every padded render"""
    first = tt.gradients(colour, Wi, Wa)
    total = {k: v.copy() for k, v in first.items()}
    cols = []
    for r, w in zip(padded, pad(Wx, axis=0)):
        g = tt.gradients(r, w, np.zeros_like(Wa))
        cols.append(g.pop("colors_precomp"))
        for k, v in g.items():
            total[k] = total[k] + v
    total["extra_attrs"] = np.concatenate(cols, 1)[:, :E]
    return total, first


def twins(cam, sc, extra, sh_degree=0, use_image=True, use_alpha=True, use_extra=True):
    E = extra.shape[1]
    c64, p64 = _renders(cam, sc, extra, np.float64, sh_degree)
    c32, p32 = _renders(cam, sc, extra, np.float32, sh_degree)
    near = c64.near | c32.near
    for r in p64 + p32:
        near = near | r.near
    h, w = cam.image_height, cam.image_width
    Wi, Wa = gs.weights(h, w)
    Wx = weights_extra(E, h, w)
    for W, use in ((Wi, use_image), (Wa, use_alpha), (Wx, use_extra)):
        W[:, near] = 0.0
        if not use:
            W[:] = 0.0
    Wi, Wa, Wx = (W.astype(np.float32) for W in (Wi, Wa, Wx))          # what the device is handed
    g64, first = _compose(c64, p64, Wi, Wa, Wx, E)
    g32, _ = _compose(c32, p32, Wi, Wa, Wx, E)
    extra64 = np.concatenate([r.image.detach().numpy() for r in p64])[:E]
    out = Case(cam, sc, extra, Wi, Wa, Wx, g64, g32, float(near.mean()), near, c64.image.detach().numpy(), c64.alpha.detach().numpy(),
               extra64, c64.base.radii, first)
    for a in (Wi, Wa, Wx, extra64, *g64.values(), *g32.values()):
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def scene_case(key, E=E_REF, use=("image", "alpha", "extra")):
    """a named scene of raster_scenes with the seeded table; `use` names the outputs the loss reads"""
    cam, sc, _, _ = rs.twins(*key)
    return twins(cam, sc, table(sc["means3D"].shape[0], E), use_image="image" in use, use_alpha="alpha" in use, use_extra="extra" in use)


@functools.lru_cache(maxsize=None)
def precomp_case():
    cam, sc = gs.precomp_scene()
    return twins(cam, sc, table(sc["means3D"].shape[0], E_REF))


@functools.lru_cache(maxsize=None)
def sh_case(deg=2):
    cam, sc = gs.sh_scene()
    return twins(cam, sc, table(sc["means3D"].shape[0], E_REF), sh_degree=deg)


def check_grads(got, g64, what=""):
    """raster_grad_scenes.check_grads at BOUND_GX (prints before asserting)"""
    return gs.check_grads(got, g64, what, bound=BOUND_GX)


def check_forward(case, image, alpha, extra, what=""):
    """image, alpha and the extras within raster_scenes.BOUND of the float64 twin on the pixels that are not left out"""
    m = ~case.near
    errs = [np.abs(np.asarray(got, np.float64) - ref)[:, m].max() if m.any() else 0.0
            for got, ref in ((image, case.image64), (alpha, case.alpha64), (extra, case.extra64))]
    print(what, "max |. - twin64| image %.3g alpha %.3g extra %.3g (bound %.3g)" % (*errs, rs.BOUND))
    assert max(errs) <= rs.BOUND, (what, errs)


# ---- the host restatement ----------------------------------------------------------------------------------------------------------

def host():
    so = hostbuild.host_lib("hostraster_extra")
    so.hx_backward.restype = C.c_int64
    return so


def sanitizer_program():
    """the same file as a stand-alone program under AddressSanitizer and UBSan (run as a subprocess; nothing is loaded into Python)"""
    return hostbuild.host_program("hostraster_extra", name="hostraster_extra_asan",
                                  flags=["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                         "-DHOSTRASTER_EXTRA_MAIN"])


def host_backward(so, case, bg=rs.BG):
    """-> (gradients by argument name, image, alpha, extra) of tests/hostraster_extra for a scales / rotations / colours case"""
    fp = C.POINTER(C.c_float)
    c32 = lambda a: np.ascontiguousarray(a, np.float32)
    p = lambda a: a.ctypes.data_as(fp)
    cam, sc = case.cam, case.sc
    a = {k: c32(sc[k]) for k in ("means3D", "opacities", "scales", "rotations", "colors_precomp")}
    n, E = a["means3D"].shape[0], case.extra.shape[1]
    H, W = cam.image_height, cam.image_width
    out = {k: np.full(s, np.nan, np.float32) for k, s in (("means3D", (n, 3)), ("means2D", (n, 3)), ("opacities", a["opacities"].shape),
                                                          ("scales", (n, 3)), ("rotations", (n, 4)), ("colors_precomp", (n, 3)),
                                                          ("extra_attrs", (n, E)))}
    image, alpha, extra = (np.full((c, H, W), np.nan, np.float32) for c in (3, 1, E))
    view, proj, bg, table_ = c32(cam.viewmatrix), c32(cam.projmatrix), c32(bg), c32(case.extra)
    Wi, Wa, Wx = c32(case.Wi), c32(case.Wa), c32(case.Wx)
    entries = so.hx_backward(n, p(a["means3D"]), p(a["opacities"]), p(a["scales"]), p(a["rotations"]), C.c_float(1.0), p(a["colors_precomp"]),
                             p(table_), E, p(view), p(proj), W, H, C.c_float(cam.tanfovx), C.c_float(cam.tanfovy), p(bg), p(Wi), p(Wa), p(Wx),
                             p(out["means3D"]), p(out["means2D"]), p(out["opacities"]), p(out["scales"]), p(out["rotations"]),
                             p(out["colors_precomp"]), p(out["extra_attrs"]), p(image), p(alpha), p(extra))
    assert entries >= 0
    return out, image, alpha, extra
