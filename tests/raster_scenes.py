"""Scenes shared by tests/test_raster_host.py and tests/test_gpu_raster.py, with the float64 / float32 twins of each computed once
(functools.lru_cache) and never modified.  Cameras come from tests/golden/raster.npz (the reference's own camera functions) or, for
the hand-made scenes, from raster_twin.simple_camera.  Test infrastructure only."""
import functools
import os

import numpy as np

import raster_twin as tw

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raster.npz"))
H, W = int(GOLD["image_height"]), int(GOLD["image_width"])
SEEDS = (0, 1)
BG = np.array([0.1, 0.35, 0.6], np.float32)


def fixture_camera(k, h=H, w=W):
    g = lambda name: GOLD[f"cam{k}_{name}"]
    return tw.Camera(h, w, float(g("tanfovx")), float(g("tanfovy")), g("world_view_transform"), g("full_proj_transform"), g("camera_center"))


def random_scene(cam, seed, n=600, centre=(24.0, 24.0)):
    """n Gaussians in front of `cam`: view depths a permuted linspace(1, 5, n) (no two closer than 1e-4 relative), mapped to the
    world with the inverse camera pose; about a quarter outside the frustum or behind the camera; pixel centres clustered around
    `centre` so that one tile's list is longer than one batch of the render kernel."""
    rng = np.random.default_rng(1000 + seed)
    Hh, Ww = cam.image_height, cam.image_width
    z = rng.permutation(np.linspace(1.0, 5.0, n))
    ux = np.clip((2 * centre[0] + 1) / Ww - 1 + rng.normal(0, 0.3, n), -0.95, 0.95)     # ndc of the pixel centre
    uy = np.clip((2 * centre[1] + 1) / Hh - 1 + rng.normal(0, 0.3, n), -0.95, 0.95)
    kind = rng.random(n)
    out = kind < 0.15                      # far outside the frustum: the rectangle is empty
    ux = np.where(out, rng.choice([-1.0, 1.0], n) * rng.uniform(3.0, 5.0, n), ux)
    behind = (kind >= 0.15) & (kind < 0.25)
    z = np.where(behind, -z, z)
    # ndc = x / (tanfov z) for a centred camera; the off-centre one only shifts the cluster
    p_cam = np.stack([ux * cam.tanfovx * z, uy * cam.tanfovy * z, z], 1)
    V = np.asarray(cam.viewmatrix, np.float64)
    means = ((p_cam - V[3, :3]) @ np.linalg.inv(V[:3, :3])).astype(np.float32)
    scales = np.exp(rng.uniform(np.log(0.01), np.log(0.25), (n, 3))).astype(np.float32)
    rots = rng.normal(size=(n, 4)).astype(np.float32)
    opac = rng.uniform(0.05, 1.0, (n, 1)).astype(np.float32)
    cols = rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32)
    return dict(means3D=means, opacities=opac, colors_precomp=cols, scales=scales, rotations=rots)


def thin_scene(front=False):
    """16 x 16 image, 700 Gaussians that all cover the one tile, opacities 0.01-0.03 (drawn towards the low end), so that T never
    saturates through three batches.  Their centres lie on a ring 20-30 pixels from the middle of the tile with 40-60 pixels of
    standard deviation: across the tile alpha stays above 1/255 and the power away from 0, so no decision is near a threshold.
    front=True puts three nearly opaque, tile-filling Gaussians before everything: every pixel finishes at the third (T = 0.01,
    then 5e-4, then the test value 5e-5 < 1e-4, none of them near the threshold) and no thin layer shows."""
    rng = np.random.default_rng(77)
    cam = tw.simple_camera(16, 16)
    n, focal = 700, 16.0
    z = rng.permutation(np.linspace(1.0, 5.0, n))
    ang, d = rng.uniform(0, 2 * np.pi, n), rng.uniform(20.0, 30.0, n)
    means = np.stack([d * np.cos(ang) * z / focal, d * np.sin(ang) * z / focal, z], 1).astype(np.float32)
    scales = (rng.uniform(40.0, 60.0, (n, 3)) * z[:, None] / focal).astype(np.float32)
    sc = dict(means3D=means, opacities=(0.01 + 0.02 * rng.random((n, 1)) ** 6).astype(np.float32),
              colors_precomp=rng.uniform(0, 1, (n, 3)).astype(np.float32), scales=scales, rotations=rng.normal(size=(n, 4)).astype(np.float32))
    if front:
        f = dict(means3D=np.array([[3.0, 1.0, 0.5], [-3.0, 2.0, 0.6], [2.0, -4.0, 0.7]], np.float32), opacities=np.array([[1.0], [0.95], [0.9]], np.float32),
                 colors_precomp=np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32), scales=np.full((3, 3), 50.0, np.float32),
                 rotations=np.tile(np.array([[1, 0, 0, 0]], np.float32), (3, 1)))
        sc = {k: np.concatenate([f[k], sc[k]]) for k in sc}
    return cam, sc


def n_front():
    return 3


@functools.lru_cache(maxsize=None)
def twins(name, *args):
    """(camera, scene, float64 render, float32 render) of a named scene"""
    if name == "random":
        k, seed = args
        cam = fixture_camera(k)
        sc = random_scene(cam, seed)
    elif name == "thin":
        cam, sc = thin_scene(front=False)
    elif name == "front":
        cam, sc = thin_scene(front=True)
    elif name == "odd":
        h, w = args
        cam = tw.simple_camera(h, w)
        sc = random_scene(cam, 5, n=300, centre=(w / 2, h / 2))
    else:
        raise KeyError(name)
    r64 = tw.render(cam, BG, dtype=np.float64, **sc)
    r32 = tw.render(cam, BG, dtype=np.float32, **sc)
    for a in (r64.image, r64.alpha, r32.image, r32.alpha):
        a.setflags(write=False)
    return cam, sc, r64, r32


COMPARED = [("random", k, s) for k in (0, 1) for s in SEEDS] + [("thin",), ("front",), ("odd", 9, 70), ("odd", 33, 17)]

# Measured on the CPU over the COMPARED scenes (tests/test_raster_host.py::test_e32_and_the_left_out_share asserts both):
# E32 = max |twin32 - twin64| over image and alpha on the pixels that are not left out.  The GPU must lie within
# BOUND = 10 * E32 of the float64 twin: the factor covers a different exp and FMA contraction.
E32 = 1.3e-6   # measured 1.29e-6 (fixture camera 1, seed 0); the other scenes 0.4e-7 .. 8.7e-7
BOUND = 10 * E32
MAX_LEFT_OUT_SHARE = 0.01


def compared_mask(r64, r32=None):
    """pixels that enter the image comparison: no decision near a threshold in either twin"""
    m = ~r64.near
    if r32 is not None:
        m &= ~r32.near
    return m
