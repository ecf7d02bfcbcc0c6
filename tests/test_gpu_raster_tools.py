"""What stands around the rasteriser on the GPU: the stage timing that tools/raster_bench.py reads (mpmhip_raster_profile) and
examples/render_demo.py end to end, small."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import raster_scenes as rs
from test_gpu_raster import gpu_render, settings
from test_raster_host import _decode_png

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stage_profile_counts_frames_and_leaves_the_image_alone():
    from mpmavatar_amd import _lib as L
    from mpmavatar_amd.rasterizer import GaussianRasterizer
    cam, sc, _, _ = rs.twins("random", 0, 0)
    r = GaussianRasterizer(settings(cam), private_scratch=True)
    before = gpu_render(cam, sc, rasterizer=r)
    hd = r._last
    stage, frames = (C.c_double * 6)(), C.c_int64(-1)
    assert hd.lib.mpmhip_raster_profile(hd.ptr, 1, stage, C.byref(frames)) == L.OK
    assert frames.value == 0 and all(v == 0.0 for v in stage)             # nothing was accumulated while it was off
    during = [gpu_render(cam, sc, rasterizer=r) for _ in range(2)]
    assert hd.lib.mpmhip_raster_profile(hd.ptr, 0, stage, C.byref(frames)) == L.OK
    ms = list(stage)
    print("stage ms over 2 frames:", ms)
    assert frames.value == 2
    assert all(np.isfinite(v) and v >= 0.0 for v in ms) and ms[5] > 0.0 and sum(ms) < 2000.0    # the render stage took time
    after = gpu_render(cam, sc, rasterizer=r)
    assert hd.lib.mpmhip_raster_profile(hd.ptr, 0, stage, C.byref(frames)) == L.OK
    assert frames.value == 2 and list(stage) == ms                        # off: nothing more is added
    for got in during + [after]:
        for a, b in zip(before[:3], got[:3]):
            assert np.array_equal(a, b)                                   # bitwise the same image, alpha and radii
    assert hd.lib.mpmhip_raster_profile(None, 1, None, None) == L.ERR_INVALID


def test_render_demo_end_to_end(tmp_path):
    """Solver -> MeshFrames -> render_inputs -> rasteriser -> frame_NNN.png (examples/render_demo.py), small."""
    import torch
    spec = importlib.util.spec_from_file_location("render_demo", os.path.join(ROOT, "examples", "render_demo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(["--out", str(tmp_path), "--frames", "2", "--substeps", "20", "--size", "64", "--gaussians-per-face", "2"])
    image, mask, radii = out["image"], out["mask"], out["radii"]
    assert tuple(image.shape) == (3, 64, 64) and torch.isfinite(image).all() and torch.isfinite(mask).all()
    covered = float((mask > 0.5).float().mean())
    print("render_demo at 64 x 64: covered share %.3f, visible %d of %d" % (covered, int((radii > 0).sum()), radii.numel()))
    assert 0.05 < covered < 0.95                                          # the garment is in the frame and does not fill it
    assert int((radii > 0).sum()) > radii.numel() // 2
    for k in (1, 2):
        px = _decode_png(str(tmp_path / f"frame_{k:03d}.png"))
        assert px.shape == (64, 64, 3)
        assert (px == 255).all(2).any() and not (px == 255).all()          # white background and something on it
    last = np.floor(np.clip(image.cpu().numpy().astype(np.float64), 0, 1) * 255.0 + 0.5).transpose(1, 2, 0)
    assert np.abs(px.astype(np.float64) - last).max() <= 1                # the file is the returned image
