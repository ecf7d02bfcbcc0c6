#!/usr/bin/env python
"""Time the forward rasteriser (csrc/raster.hip) at the size of the reference's renders: 200,000 Gaussians bound to the faces of
the S3 garment (scenes.garment_cylinder, 79,600 faces) at 1024 x 1024, 20 warm-up and 100 timed frames.

    python tools/raster_bench.py [--gaussians 200000] [--size 1024] [--warmup 20] [--frames 100] [--out file.json]

Reported: milliseconds per frame of the whole call (HIP events on torch's current stream around the timed frames, frames
+ render_inputs + rasteriser, and the rasteriser alone), and per stage of the pipeline from the library's own event brackets
(mpmhip_raster_profile, a second pass: the brackets make every frame wait for its end)."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from mpmavatar_amd import _lib as L
from mpmavatar_amd import scenes
from mpmavatar_amd.mesh_frames import MeshFrames
from mpmavatar_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer, look_at_camera
from mpmavatar_amd.render_inputs import BoundGaussians

STAGES = ("preprocess", "scan_and_readback", "duplicate", "sort", "ranges", "render")


def events_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=200000)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("raster_bench.py measures on the GPU; there is none")
    dev = torch.device("cuda:0")
    sc = scenes.garment_cylinder()
    faces = torch.as_tensor(sc.faces, device=dev)
    verts = torch.as_tensor(np.asarray(sc.x[sc.n_elements + sc.n_traditional:], np.float32), device=dev).contiguous()
    n_f, n = faces.shape[0], a.gaussians
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)
    binding = (torch.arange(n, device=dev) % n_f).to(torch.int32)
    gaussians = BoundGaussians(0.35 * rnd(n, 3) * torch.tensor([1.0, 1.0, 0.05], device=dev), rnd(n, 4), -0.6 + 0.2 * rnd(n, 3), 2.0 + rnd(n, 1),
                               torch.zeros(n, 1, 3, device=dev), torch.zeros(n, 0, 3, device=dev), binding)
    colors = torch.rand(n, 3, device=dev, generator=g)
    frames = MeshFrames(faces)
    centre = verts.mean(0).cpu().numpy()
    view, proj, campos, tanfov = look_at_camera(centre + np.array([0.0, 0.15, -1.6]), centre, 40.0, dev)
    settings = GaussianRasterizationSettings(a.size, a.size, tanfov, tanfov, torch.zeros(3, device=dev), 1.0, view, proj, 0, campos, False, False)
    rast = GaussianRasterizer(settings, private_scratch=True)
    state = {}

    def inputs():
        frames.set_mesh_by_verts(verts)
        state["args"] = gaussians.render_inputs(frames, override_color=colors)

    def render():
        state["out"] = rast(**state["args"])

    def frame():
        inputs()
        render()

    for _ in range(a.warmup):
        frame()
    frame_ms = events_ms(frame, a.frames)
    raster_ms = events_ms(render, a.frames)
    st = rast.stats()
    hd = rast._last
    stage = (C.c_double * len(STAGES))()
    count = C.c_int64()
    assert hd.lib.mpmhip_raster_profile(hd.ptr, 1, None, None) == L.OK
    for _ in range(a.frames):
        render()
    assert hd.lib.mpmhip_raster_profile(hd.ptr, 0, stage, C.byref(count)) == L.OK
    image, alpha = state["out"][0], state["out"][3]
    res = {"gaussians": n, "faces": int(n_f), "image": [a.size, a.size], "warmup": a.warmup, "frames": a.frames,
           "frame_ms_inputs_and_raster": frame_ms, "frame_ms_raster": raster_ms,
           "stage_ms": {k: stage[i] / max(1, count.value) for i, k in enumerate(STAGES)},
           "covered_pixels_share": float((alpha > 0.5).float().mean()), "finite": bool(torch.isfinite(image).all()), **st}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
