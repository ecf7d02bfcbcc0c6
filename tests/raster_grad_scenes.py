"""The loss, the yardstick gradients and the constants shared by tests/test_raster_grad_host.py and tests/test_gpu_raster_grad.py.

The loss is L = sum Wi image + sum Wa alpha with fixed seeded normal weights, set to zero on every pixel that either torch twin
(float64, float32; tests/raster_twin_torch.py) marks near a threshold -- the NumPy twins' conditions plus
|opacity exp(power) / 0.99 - 1| < 1e-4 for a Gaussian that contributes.  At most MAX_LEFT_OUT_SHARE of a scene's pixels may be
left out.  Each scene's twins are computed once (functools.lru_cache) and never modified.  Test infrastructure only."""
import functools

import numpy as np

import raster_scenes as rs
import raster_twin as tw
import raster_twin_torch as tt

# Measured on the CPU over raster_scenes.COMPARED and all gradient tensors (tests/test_raster_grad_host.py::test_g32_and_the_left_out_share
# asserts it): G32 = max over scenes and tensors of max |g32 - g64| / max |g64|, float32 torch twin against float64.  The code
# under test plays no part in it.  The GPU and the host backward must lie within BOUND_G = 10 * G32 of the float64 twin; the
# factor is the forward test's (a different exp, FMA contraction) and also covers a different summation order and T rebuilt by
# division (2.4e-6 relative at worst through the 700 thin layers in fp32).
G32 = 3.3e-6   # measured 3.23e-6 (rotations, fixture camera 0, seed 0); the other tensors and scenes 3.3e-7 .. 2.9e-6
BOUND_G = 10 * G32
MAX_LEFT_OUT_SHARE = rs.MAX_LEFT_OUT_SHARE
CLAMP_MARGIN = 1e-4    # no visible Gaussian within this relative distance of the frustum clamp or of the SH zero clamp


def weights(h, w, seed=2024):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(3, h, w)), rng.normal(size=(1, h, w))


def grad_twins(cam, sc, sh_degree=0, use_image=True, use_alpha=True):
    """-> (Wi, Wa, g64, g32, left-out share, r64, r32): the weights with the near pixels zeroed, and the gradients of both twins"""
    r64 = tt.render(cam, rs.BG, dtype=np.float64, sh_degree=sh_degree, **sc)
    r32 = tt.render(cam, rs.BG, dtype=np.float32, sh_degree=sh_degree, **sc)
    Wi, Wa = weights(cam.image_height, cam.image_width)
    near = r64.near | r32.near
    Wi[:, near] = 0.0
    Wa[:, near] = 0.0
    if not use_image:
        Wi[:] = 0.0
    if not use_alpha:
        Wa[:] = 0.0
    Wi, Wa = Wi.astype(np.float32), Wa.astype(np.float32)      # what the device is handed
    g64, g32 = tt.gradients(r64, Wi, Wa), tt.gradients(r32, Wi, Wa)
    for a in (Wi, Wa, *g64.values(), *g32.values()):
        a.setflags(write=False)
    return Wi, Wa, g64, g32, float(near.mean()), r64, r32


@functools.lru_cache(maxsize=None)
def scene_grads(name, *args):
    cam, sc, _, _ = rs.twins(name, *args)
    return (cam, sc) + grad_twins(cam, sc)


def precomp_scene():
    """random scene, camera 1 seed 0, with the covariance handed over as cov3Ds_precomp (float32 values of the float64 formula)"""
    cam, sc, _, _ = rs.twins("random", 1, 0)
    pre = {k: v for k, v in sc.items() if k not in ("scales", "rotations")}
    pre["cov3Ds_precomp"] = tw.cov3d(sc["scales"], sc["rotations"], 1.0).astype(np.float32)
    return cam, pre


@functools.lru_cache(maxsize=None)
def precomp_grads():
    cam, sc = precomp_scene()
    return (cam, sc) + grad_twins(cam, sc)


def sh_scene():
    """the fixture's SH data (positions, coefficients, camera 0) with seeded opacities, scales and rotations"""
    g = rs.GOLD
    cam = rs.fixture_camera(0)
    n = g["sh_positions"].shape[0]
    rng = np.random.default_rng(4)
    return cam, dict(means3D=g["sh_positions"], opacities=rng.uniform(0.2, 0.9, (n, 1)).astype(np.float32),
                     scales=rng.uniform(0.05, 0.3, (n, 3)).astype(np.float32), rotations=rng.normal(size=(n, 4)).astype(np.float32),
                     shs=g["sh_coeffs"])


@functools.lru_cache(maxsize=None)
def sh_grads(deg):
    cam, sc = sh_scene()
    return (cam, sc) + grad_twins(cam, sc, sh_degree=deg)


def rel_err(g, g64):
    """max |g - g64| / max |g64|; g64 identically zero is the caller's case"""
    return float(np.abs(np.asarray(g, np.float64).reshape(g64.shape) - g64).max() / np.abs(g64).max())


def check_grads(got, g64, what="", bound=None):
    """every tensor of `got` within BOUND_G of the float64 twin; a tensor whose float64 gradient is identically zero must be finite
    and at most BOUND_G * max |g64 of scales| (or of the largest other tensor where there are no scales).  Prints before asserting."""
    bound = BOUND_G if bound is None else bound
    worst = 0.0
    ref_scale = np.abs(g64["scales"]).max() if "scales" in g64 else max(np.abs(v).max() for v in g64.values())
    fails = []
    for k, ref in g64.items():
        g = np.asarray(got[k], np.float64).reshape(ref.shape)
        if ref.size == 0:
            continue
        if np.abs(ref).max() == 0.0:
            ok = bool(np.isfinite(g).all() and np.abs(g).max() <= bound * ref_scale)
            print(what, k, "float64 gradient is zero; max |g| = %.3g (allowed %.3g)" % (np.abs(g).max(), bound * ref_scale))
        else:
            e = rel_err(g, ref)
            worst = max(worst, e)
            ok = bool(np.isfinite(g).all() and e <= bound)
            print(what, k, "max |g - g64| / max |g64| = %.3g (bound %.3g)" % (e, bound))
        if not ok:
            fails.append(k)
    assert not fails, (what, fails)
    return worst
