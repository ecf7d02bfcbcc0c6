#!/usr/bin/env python
"""Time the forward rasteriser (csrc/raster.hip) at the size of the reference's renders: 200,000 Gaussians bound to the faces of
the S3 garment (scenes.garment_cylinder, 79,600 faces) at 1024 x 1024, 20 warm-up and 100 timed frames.

    python tools/raster_bench.py [--gaussians 200000] [--size 1024] [--warmup 20] [--frames 100] [--out file.json]
    python tools/raster_bench.py --backward [...]      the backward pass on the same frame -> profiles/raster_bench_backward.json

Reported: milliseconds per frame of the whole call (HIP events on torch's current stream around the timed frames, frames
+ render_inputs + rasteriser, and the rasteriser alone), and per stage of the pipeline from the library's own event brackets
(mpmhip_raster_profile, a second pass: the brackets make every frame wait for its end).

--backward times, each stage over the timed frames between two HIP events, the plain forward call, the forward call that
records its state (mpmhip_raster_forward_grad), the copy of that state (mpmhip_raster_save) and the backward pass
(mpmhip_raster_backward with both incoming gradients), and reports backward / forward and the traffic of the per-entry row
buffer: 36 B per (tile, Gaussian) entry written once and read once, over the backward pass's time."""
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


def backward_mode(a, rast, args, settings, dev, n, n_f):
    h = w = a.size
    hd = rast._handle(dev)
    lib = hd.lib
    view, proj, campos = settings.viewmatrix.contiguous(), settings.projmatrix.contiguous(), settings.campos.contiguous()
    cs = L.RasterSettings(h, w, settings.tanfovx, settings.tanfovy, L.f3(0.0, 0.0, 0.0), 1.0, 0, view.data_ptr(), proj.data_ptr(),
                          campos.data_ptr())
    t = {k: args[k].detach().contiguous() for k in ("means3D", "colors_precomp", "opacities", "scales", "rotations")}
    image, alpha = torch.empty(3, h, w, device=dev), torch.empty(1, h, w, device=dev)
    radii = torch.empty(n, dtype=torch.int32, device=dev)
    fwd = (hd.ptr, C.byref(cs), n, t["means3D"].data_ptr(), None, 0, t["colors_precomp"].data_ptr(), t["opacities"].data_ptr(),
           t["scales"].data_ptr(), t["rotations"].data_ptr(), None, image.data_ptr(), alpha.data_ptr(), radii.data_ptr())

    def ok(rc):
        if rc != L.OK:
            raise L.MPMHipError(rc, "raster call failed")

    ok(lib.mpmhip_raster_forward_grad(*fwd))
    size, entries = C.c_int64(), C.c_int64()
    ok(lib.mpmhip_raster_saved_bytes(hd.ptr, C.byref(size), C.byref(entries)))
    saved = torch.empty(size.value, dtype=torch.uint8, device=dev)
    g = torch.Generator(device=dev).manual_seed(1)
    g_image, g_alpha = torch.randn(3, h, w, device=dev, generator=g), torch.randn(1, h, w, device=dev, generator=g)
    d = {k: torch.empty_like(v) for k, v in t.items()}
    d["means2D"] = torch.empty(n, 3, device=dev)
    bwd = fwd[:11] + (saved.data_ptr(), size.value, entries.value, g_image.data_ptr(), g_alpha.data_ptr(), d["means3D"].data_ptr(),
                      d["means2D"].data_ptr(), None, d["colors_precomp"].data_ptr(), d["opacities"].data_ptr(), d["scales"].data_ptr(),
                      d["rotations"].data_ptr(), None)
    stages = {"forward": lambda: ok(lib.mpmhip_raster_forward(*fwd)), "forward_with_state": lambda: ok(lib.mpmhip_raster_forward_grad(*fwd)),
              "save": lambda: ok(lib.mpmhip_raster_save(hd.ptr, saved.data_ptr(), size.value)), "backward": lambda: ok(lib.mpmhip_raster_backward(*bwd))}
    ok(lib.mpmhip_raster_save(hd.ptr, saved.data_ptr(), size.value))
    ms = {}
    for name, fn in stages.items():
        if name == "save":
            ok(lib.mpmhip_raster_forward_grad(*fwd))       # the state to copy is the newest frame's
        for _ in range(a.warmup):
            fn()
        ms[name] = events_ms(fn, a.frames)
    first = {k: v.clone() for k, v in d.items()}
    ok(lib.mpmhip_raster_backward(*bwd))
    torch.cuda.synchronize()
    row_bytes = 36 * entries.value
    res = {"gaussians": n, "faces": n_f, "image": [h, w], "warmup": a.warmup, "frames": a.frames, "stage_ms": ms,
           "backward_over_forward": ms["backward"] / ms["forward"], "training_frame_ms": ms["forward_with_state"] + ms["save"] + ms["backward"],
           "n_entries": entries.value, "saved_bytes": size.value, "row_buffer_bytes": row_bytes,
           "row_buffer_bytes_per_s_over_backward": 2 * row_bytes / (ms["backward"] * 1e-3),
           "finite": bool(all(torch.isfinite(v).all() for v in d.values())),
           "bitwise_repeatable": bool(all(torch.equal(first[k], d[k]) for k in d)),
           "grad_abs_max": {k: float(v.abs().max()) for k, v in d.items()}}
    line = json.dumps(res)
    print(line)
    out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "raster_bench_backward.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=200000)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--out", default=None)
    ap.add_argument("--backward", action="store_true")
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

    if a.backward:
        inputs()
        return backward_mode(a, rast, state["args"], settings, dev, n, int(n_f))
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
