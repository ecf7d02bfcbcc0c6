"""The forward rasteriser on the GPU (mpmavatar_amd/csrc/raster.hip through mpmavatar_amd.rasterizer) against the float64 twin
(tests/raster_twin.py) on the scenes of tests/raster_scenes.py.  Radii must be EXACTLY equal; image and alpha must lie within
raster_scenes.BOUND = 10 * E32 of the twin on every pixel none of whose decisions was near a threshold (at most 1 % are left out);
E32 and the conditions that make this possible are measured and asserted on the CPU in tests/test_raster_host.py.
Every comparison prints its figures before it asserts (run with -s)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import raster_scenes as rs
import raster_twin as tw

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = rs.BOUND


def _dev():
    import torch
    return torch.device("cuda:0")


def _t(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def settings(cam, bg=rs.BG, sh_degree=0, scale_modifier=1.0):
    from mpmavatar_amd.rasterizer import GaussianRasterizationSettings
    return GaussianRasterizationSettings(image_height=cam.image_height, image_width=cam.image_width, tanfovx=cam.tanfovx,
                                         tanfovy=cam.tanfovy, bg=_t(np.asarray(bg, np.float32)), scale_modifier=scale_modifier,
                                         viewmatrix=_t(cam.viewmatrix), projmatrix=_t(cam.projmatrix), sh_degree=sh_degree,
                                         campos=_t(np.asarray(cam.campos, np.float32)), prefiltered=False, debug=False)


def gpu_render(cam, sc, rasterizer=None, **kw):
    """-> (image [3,H,W], alpha [1,H,W], radii [n]) as NumPy arrays, and the rasteriser (for its stats)"""
    from mpmavatar_amd.rasterizer import GaussianRasterizer
    r = rasterizer or GaussianRasterizer(raster_settings=settings(cam, **kw))
    args = {k: _t(v) for k, v in sc.items()}
    import torch
    args.setdefault("means2D", torch.zeros_like(args["means3D"], requires_grad=True))       # as the reference passes it
    for k in ("shs", "colors_precomp", "scales", "rotations", "cov3Ds_precomp"):
        args.setdefault(k, None)
    out = r(**args)
    assert len(out) == 6 and out[1] is None and out[2] is None and out[5] is None
    image, alpha, radii = out[0], out[3], out[4]
    assert not image.requires_grad and image.grad_fn is None and radii.dtype == torch.int32
    assert tuple(image.shape) == (3, cam.image_height, cam.image_width) and tuple(alpha.shape) == (1, cam.image_height, cam.image_width)
    return image.cpu().numpy(), alpha.cpu().numpy(), radii.cpu().numpy(), r


def check_against_twin(got, r64, what=""):
    image, alpha, radii = got[:3]
    assert np.array_equal(radii, r64.radii), what
    m = rs.compared_mask(r64)
    share = 1.0 - m.mean()
    e_img, e_alpha = np.abs(image - r64.image)[:, m].max(), np.abs(alpha - r64.alpha)[:, m].max()
    print(what, "max |image - twin64| = %.3g, max |alpha - twin64| = %.3g (bound %.3g), left out %d of %d pixels"
          % (e_img, e_alpha, BOUND, (~m).sum(), m.size))
    assert share <= rs.MAX_LEFT_OUT_SHARE, what
    assert e_img <= BOUND and e_alpha <= BOUND, what


@pytest.mark.parametrize("k", (0, 1))
@pytest.mark.parametrize("seed", rs.SEEDS)
def test_random_scene_against_the_twin(k, seed):
    cam, sc, r64, _ = rs.twins("random", k, seed)
    got = gpu_render(cam, sc)
    check_against_twin(got, r64, f"camera {k} seed {seed}")
    st = got[3].stats()
    assert st["max_tile_entries"] == r64.max_tile_entries > 256          # the batch loop ran more than once
    assert st["n_visible"] == int((r64.radii > 0).sum()) and st["n_entries"] > 0 and st["scratch_bytes"] > 0


def test_thin_layers_through_three_batches():
    cam, sc, r64, _ = rs.twins("thin")
    got = gpu_render(cam, sc)
    check_against_twin(got, r64, "thin")
    assert got[3].stats()["max_tile_entries"] == 700


def test_early_exit_hides_the_later_layers():
    cam, sc, r64, _ = rs.twins("front")
    got = gpu_render(cam, sc)
    check_against_twin(got, r64, "front")
    only = gpu_render(cam, {k: v[:rs.n_front()] for k, v in sc.items()})
    assert np.array_equal(got[0], only[0]) and np.array_equal(got[1], only[1])     # the 700 layers behind change no bit


def test_culled_scene_is_the_background():
    cam = tw.simple_camera(16, 16)
    iso = lambda v: [v, 0, 0, v, 0, v]
    means = np.array([[0, 0, 0.2], [0, 0, 0.1], [0, 0, -3], [40, 0, 2], [0, -40, 2], [0, 0, 2]], np.float32)
    cov = np.array([iso(0.01)] * 5 + [[2.0 ** 34, 2.0 ** 34, 0, 2.0 ** 34, 0, 0]], np.float32)      # the last: det == 0 in fp32
    sc = dict(means3D=means, opacities=np.ones((6, 1), np.float32), colors_precomp=np.ones((6, 3), np.float32), cov3Ds_precomp=cov)
    image, alpha, radii, r = gpu_render(cam, sc)
    assert (radii == 0).all() and (alpha == 0).all()
    assert np.array_equal(image, np.broadcast_to(rs.BG[:, None, None], image.shape))
    assert r.stats()["n_entries"] == 0 and r.stats()["n_visible"] == 0
    empty = {k: v[:0] for k, v in sc.items()}                                                   # n == 0 renders the background
    image0, alpha0, radii0, _ = gpu_render(cam, empty)
    assert np.array_equal(image0, image) and (alpha0 == 0).all() and radii0.shape == (0,)


def test_equal_depths_go_by_index():
    cam = tw.simple_camera(16, 16)
    mean = np.array([[0.05, -0.03, 2.0]], np.float32)
    two = lambda a, b: np.concatenate([a, b])
    red, blue = np.array([[1, 0, 0]], np.float32), np.array([[0, 0, 1]], np.float32)
    base = dict(means3D=two(mean, mean), opacities=np.full((2, 1), 0.8, np.float32), scales=np.full((2, 3), 0.3, np.float32),
                rotations=np.tile(np.array([[1, 0, 0, 0]], np.float32), (2, 1)))
    imgs = []
    for cols in (two(red, blue), two(blue, red)):
        sc = dict(base, colors_precomp=cols)
        got = gpu_render(cam, sc)
        check_against_twin(got, tw.render(cam, rs.BG, **sc), "ties")
        imgs.append(got[0])
    # at the centre the front one weighs 0.8 and the one behind 0.8 * 0.2
    assert imgs[0][0, 8, 8] > 0.7 and imgs[0][2, 8, 8] < 0.3 and imgs[1][2, 8, 8] > 0.7 and imgs[1][0, 8, 8] < 0.3


def test_determinism_and_scratch_growth():
    from mpmavatar_amd.rasterizer import GaussianRasterizer
    cam, sc, r64, _ = rs.twins("random", 0, 0)
    one = GaussianRasterizer(settings(cam), private_scratch=True)
    first = gpu_render(cam, sc, rasterizer=one)
    small_bytes = one.stats()["scratch_bytes"]
    big_cam = tw.simple_camera(128, 128)
    big = rs.random_scene(big_cam, 9, n=20000, centre=(64.0, 64.0))
    one.raster_settings = settings(big_cam)
    b = gpu_render(big_cam, big, rasterizer=one)
    assert np.isfinite(b[0]).all() and b[1].max() > 0.5 and (b[2] > 0).sum() > 10000
    assert one.stats()["scratch_bytes"] > small_bytes                                           # the scratch grew ...
    grown = one.stats()["scratch_bytes"]
    one.raster_settings = settings(cam)
    third = gpu_render(cam, sc, rasterizer=one)
    assert one.stats()["scratch_bytes"] == grown                                                # ... and is reused
    fresh = gpu_render(cam, sc, rasterizer=GaussianRasterizer(settings(cam), private_scratch=True))
    for a, b_, c in zip(first[:3], third[:3], fresh[:3]):
        assert np.array_equal(a, b_) and np.array_equal(a, c)


@pytest.mark.parametrize("deg", (0, 1, 2, 3))
def test_sh_path_equals_the_reference_s_colours(deg):
    g = rs.GOLD
    cam = rs.fixture_camera(0)
    assert np.array_equal(np.asarray(cam.campos, np.float32), g["sh_campos"])
    n = g["sh_positions"].shape[0]
    rng = np.random.default_rng(4)
    base = dict(means3D=g["sh_positions"], opacities=rng.uniform(0.2, 0.9, (n, 1)).astype(np.float32),
                scales=rng.uniform(0.05, 0.3, (n, 3)).astype(np.float32), rotations=rng.normal(size=(n, 4)).astype(np.float32))
    a = gpu_render(cam, dict(base, shs=g["sh_coeffs"]), sh_degree=deg)
    b = gpu_render(cam, dict(base, colors_precomp=g[f"sh_colors_deg{deg}"].astype(np.float32)))
    assert np.array_equal(a[2], b[2]) and (a[2] > 0).sum() > 20 and a[1].max() > 0.5
    assert np.abs(a[0] - b[0]).max() <= BOUND and np.array_equal(a[1], b[1])


def test_cov3d_precomp_path_equals_the_scale_rotation_path():
    cam, sc, r64, _ = rs.twins("random", 1, 0)
    a = gpu_render(cam, sc)
    pre = {k: v for k, v in sc.items() if k not in ("scales", "rotations")}
    pre["cov3Ds_precomp"] = tw.cov3d(sc["scales"], sc["rotations"], 1.0).astype(np.float32)
    b = gpu_render(cam, pre)
    assert np.array_equal(a[2], b[2])
    m = rs.compared_mask(r64)
    assert np.abs(a[0] - b[0])[:, m].max() <= BOUND and np.abs(a[1] - b[1])[:, m].max() <= BOUND
    check_against_twin(b, r64, "cov3Ds_precomp")


@pytest.mark.parametrize("shape", ((9, 70), (33, 17)))
def test_odd_image_shapes(shape):
    cam, sc, r64, _ = rs.twins("odd", *shape)
    check_against_twin(gpu_render(cam, sc), r64, f"{shape[0]} x {shape[1]}")


def test_end_to_end_from_simulated_vertices_to_the_image():
    """12 x 12-vertex synthetic garment -> MeshFrames -> BoundGaussians.render_inputs (with `extra` primitives) ->
    GaussianRasterizer(**args), against the twin fed the very arrays the rasteriser was handed."""
    import torch
    from mpmavatar_amd import garment
    from mpmavatar_amd.mesh_frames import MeshFrames
    from mpmavatar_amd.rasterizer import GaussianRasterizer
    from mpmavatar_amd.render_inputs import BoundGaussians
    rng = np.random.default_rng(12)
    verts, faces = garment.grid_sheet(12, 12, -0.6, 0.6, 2.0, 3.2, -0.2)
    verts = verts + np.stack([0 * verts[:, 0], 0.1 * np.sin(5 * verts[:, 0]) * np.cos(3 * verts[:, 2]), 0 * verts[:, 0]], 1)
    n_f = faces.shape[0]
    n, m = 2 * n_f, 30
    f32 = lambda a: _t(np.asarray(a, np.float32))
    g = BoundGaussians(f32(rng.normal(0, 0.3, (n, 3))), f32(rng.normal(size=(n, 4))), f32(rng.normal(-0.5, 0.4, (n, 3))),
                       f32(rng.normal(0.5, 1.5, (n, 1))), f32(rng.normal(size=(n, 1, 3))), f32(rng.normal(size=(n, 3, 3))),
                       _t(rng.integers(0, n_f, n)))
    fr = MeshFrames(_t(faces.astype(np.int32)))
    fr.set_mesh_by_verts(f32(verts))
    extra = (f32(rng.uniform([-0.5, -0.4, 1.5], [0.5, 0.4, 3.0], (m, 3))), f32(rng.uniform(0, 1, (m, 3))), f32(rng.uniform(0.3, 1, (m, 1))),
             f32(rng.uniform(0.01, 0.05, (m, 3))), f32(rng.normal(size=(m, 4))))
    args = g.render_inputs(fr, override_color=f32(rng.uniform(0, 1, (n, 3))), extra=extra)
    cam = tw.simple_camera(40, 56)
    image, _, _, alpha, radii, _ = GaussianRasterizer(raster_settings=settings(cam))(**args)
    host = {k: v.detach().cpu().numpy() for k, v in args.items() if v is not None and k != "means2D"}
    r64 = tw.render(cam, rs.BG, **host)
    assert (r64.radii > 0).sum() > n // 2 and r64.alpha.max() > 0.9
    check_against_twin((image.cpu().numpy(), alpha.cpu().numpy(), radii.cpu().numpy()), r64, "end to end")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "mpmavatar_amd", "compat")]))
    code = ("from diff_gauss import GaussianRasterizationSettings, GaussianRasterizer\n"          # gaussian_renderer/__init__.py:14
            "import mpmavatar_amd.rasterizer as R\n"
            "assert GaussianRasterizer is R.GaussianRasterizer and GaussianRasterizationSettings is R.GaussianRasterizationSettings")
    assert subprocess.run([sys.executable, "-c", code], env=env, cwd=os.path.join(ROOT, "tests"), timeout=300).returncode == 0


def test_error_paths_return_invalid_raise_and_launch_nothing():
    import torch
    from mpmavatar_amd import _lib as L
    from mpmavatar_amd.rasterizer import GaussianRasterizer
    lib = L.load()
    cam, sc, _, _ = rs.twins("odd", 9, 70)
    d = {k: _t(v) for k, v in sc.items()}
    n = d["means3D"].shape[0]
    shs = torch.zeros(n, 16, 3, device=_dev())
    cov = torch.zeros(n, 6, device=_dev())
    st = settings(cam)
    image = torch.full((3, 9, 70), -7.0, device=_dev())
    alpha = torch.full((1, 9, 70), -7.0, device=_dev())
    radii = torch.full((n,), -7, dtype=torch.int32, device=_dev())
    h = L.vp()
    assert lib.mpmhip_raster_create(0, None, C.byref(h)) == L.OK

    def forward(n_=n, height=9, width=70, shs_=None, n_sh=0, colors=d["colors_precomp"], scales=d["scales"], rots=d["rotations"],
                cov_=None, deg=0):
        cs = L.RasterSettings(height, width, cam.tanfovx, cam.tanfovy, L.f3(0, 0, 0), 1.0, deg, st.viewmatrix.data_ptr(),
                              st.projmatrix.data_ptr(), st.campos.data_ptr())
        p = lambda t: None if t is None else t.data_ptr()
        return lib.mpmhip_raster_forward(h, C.byref(cs), n_, d["means3D"].data_ptr(), p(shs_), n_sh, p(colors), d["opacities"].data_ptr(),
                                         p(scales), p(rots), p(cov_), image.data_ptr(), alpha.data_ptr(), radii.data_ptr())

    bad = [dict(n_=-1), dict(height=0), dict(width=-3), dict(shs_=shs, n_sh=16), dict(colors=None),
           dict(cov_=cov), dict(scales=None, rots=None), dict(rots=None), dict(scales=None, cov_=cov),
           dict(colors=None, shs_=shs, n_sh=16, deg=4), dict(colors=None, shs_=shs, n_sh=8, deg=3), dict(colors=None, shs_=shs, n_sh=16, deg=-1)]
    for kw in bad:
        assert forward(**kw) == L.ERR_INVALID, kw
    torch.cuda.synchronize()
    assert (image == -7).all() and (alpha == -7).all() and (radii == -7).all()                    # nothing was launched
    assert forward() == L.OK and forward(colors=None, shs_=shs, n_sh=16, deg=3) == L.OK           # the control
    torch.cuda.synchronize()
    assert (alpha >= 0).all()
    lib.mpmhip_raster_destroy(h)

    r = GaussianRasterizer(st)
    ok = dict(d, means2D=None, shs=None, cov3Ds_precomp=None)
    for kw in (dict(shs=shs), dict(colors_precomp=None), dict(cov3Ds_precomp=cov), dict(scales=None, rotations=None), dict(rotations=None),
               dict(means3D=d["means3D"].double()), dict(means3D=d["means3D"].cpu()), dict(scales=d["scales"][:, :2]),
               dict(opacities=d["opacities"][:-1]), dict(colors_precomp=d["colors_precomp"].t().contiguous().t()),
               dict(rotations=d["rotations"].cpu())):
        with pytest.raises(RuntimeError):
            r(**dict(ok, **kw))
    for bad_settings in (st._replace(image_height=0), st._replace(sh_degree=4), st._replace(viewmatrix=st.viewmatrix.double())):
        with pytest.raises(RuntimeError):
            GaussianRasterizer(bad_settings)(**dict(ok, **(dict(shs=shs, colors_precomp=None) if bad_settings.sh_degree == 4 else {})))
