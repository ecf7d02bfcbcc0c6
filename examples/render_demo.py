#!/usr/bin/env python
"""From simulated vertices to images without leaving the GPU: the reference's eval / demo loop (train_material_params.py:742-872,
run_demo.py:514-604) on the synthetic garment, with the rasteriser that the reference takes from the diff_gauss extension:

    per frame:  num_substeps x p2g2p (one fused call, mesh advected on the device)
                -> MeshFrames.set_mesh_by_verts(particle_x) -> BoundGaussians.render_inputs -> GaussianRasterizer -> frame_NNN.png

    python examples/render_demo.py --out /tmp/render_demo --frames 5 --substeps 200 [--size 512] [--gaussians-per-face 4]

The Gaussians are synthetic (random offsets on their faces, colour by height); the camera looks at the garment from the front.
Forward only: nothing here can train the appearance.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpmavatar_amd import harness, io_formats, scenes  # noqa: E402
from mpmavatar_amd.mesh_frames import MeshFrames  # noqa: E402
from mpmavatar_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer, look_at_camera  # noqa: E402
from mpmavatar_amd.render_inputs import BoundGaussians  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="/tmp/mpmhip_render_demo")
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--substeps", type=int, default=200)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--gaussians-per-face", type=int, default=4)
    a = ap.parse_args(argv)
    sc = scenes.small_garment()
    sim = harness.build_solver(sc, "cuda:0")
    dev = sim.solver.device
    ne, nt = sc.n_elements, sc.n_traditional
    frames = MeshFrames(torch.as_tensor(sc.faces, device=dev))
    g = torch.Generator(device=dev).manual_seed(0)
    n_g = a.gaussians_per_face * ne
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)
    binding = torch.arange(ne, device=dev, dtype=torch.int32).repeat_interleave(a.gaussians_per_face)
    gaussians = BoundGaussians(0.35 * rnd(n_g, 3) * torch.tensor([1.0, 1.0, 0.05], device=dev), rnd(n_g, 4), -0.6 + 0.2 * rnd(n_g, 3),
                               2.0 + rnd(n_g, 1), torch.zeros(n_g, 1, 3, device=dev), torch.zeros(n_g, 0, 3, device=dev), binding)
    rest = sim.state.particle_x[ne + nt:]
    height = (rest[:, 1] - rest[:, 1].min()) / (rest[:, 1].max() - rest[:, 1].min())
    face_h = height[torch.as_tensor(sc.faces, device=dev).long()].mean(1)[binding.long()]
    colors = torch.stack([0.2 + 0.7 * face_h, 0.3 + 0.3 * torch.sin(12 * face_h) ** 2, 0.9 - 0.7 * face_h], 1).contiguous()
    centre = rest.mean(0).cpu().numpy()
    view, proj, campos, tanfov = look_at_camera(centre + np.array([0.0, 0.15, -1.6]), centre, 40.0, dev)
    settings = GaussianRasterizationSettings(image_height=a.size, image_width=a.size, tanfovx=tanfov, tanfovy=tanfov,
                                             bg=torch.ones(3, device=dev), scale_modifier=1.0, viewmatrix=view, projmatrix=proj,
                                             sh_degree=0, campos=campos, prefiltered=False, debug=False)
    t_sim = t_render = 0.0
    for frame in range(a.frames):
        t0 = time.perf_counter()
        harness.run(sim, a.substeps, fused=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        frames.set_mesh_by_verts(sim.state.particle_x[ne + nt:].contiguous())
        args = gaussians.render_inputs(frames, override_color=colors)
        image, _, _, mask, radii, _ = GaussianRasterizer(raster_settings=settings)(**args)     # gaussian_renderer/__init__.py:51,95
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        t_sim, t_render = t_sim + t1 - t0, t_render + t2 - t1
        assert torch.isfinite(image).all() and mask.max() > 0.5 and (radii > 0).any()
        io_formats.write_png(os.path.join(a.out, f"frame_{frame + 1:03d}.png"), image.cpu().numpy())
    print(f"{a.frames} frames x {a.substeps} substeps of {sc.name}: simulation {1e3 * t_sim / a.frames:.1f} ms/frame, frames + Gaussians + "
          f"{a.size} x {a.size} image {1e3 * t_render / a.frames:.2f} ms/frame ({n_g} Gaussians, {int((radii > 0).sum())} visible); "
          f"frame_NNN.png under {a.out}")
    return dict(image=image, mask=mask, radii=radii)


if __name__ == "__main__":
    main()
