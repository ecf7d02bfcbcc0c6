#!/usr/bin/env python
"""A shadowed frame without leaving the GPU: the reference's eval loop (train_material_params.py:794-881) with the Blender AO bake
(train_material_params.py:819-822, blender/bake.py) replaced by mpmavatar_amd.ao_bake, on a sheet that falls onto a sphere:

    per frame:  num_substeps x p2g2p -> AOBaker.bake(sheet + sphere) -> aomap/NNN.png
                -> shadow map (a stand-in: the AO map itself, where the reference runs its ShadowUNet) -> shaded_colors
                -> MeshFrames / BoundGaussians.render_inputs -> GaussianRasterizer -> frame_NNN.png

    python examples/ao_bake_demo.py --out /tmp/ao_bake_demo --frames 4 --substeps 150 [--size 384] [--ao-res 256]

The UV mesh is the simulated sheet (planar UVs over the whole map) plus the static sphere (UVs outside the map: it covers no texel
and only occludes).  The sheet's faces are baked with the winding that turns their normals towards the sphere, the side the camera
sees.  The Gaussians are synthetic, as in examples/render_demo.py.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpmavatar_amd import harness, io_formats, scenes  # noqa: E402
from mpmavatar_amd.ao_bake import AOBaker  # noqa: E402
from mpmavatar_amd.mesh_frames import MeshFrames  # noqa: E402
from mpmavatar_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer, look_at_camera  # noqa: E402
from mpmavatar_amd.render_inputs import BoundGaussians  # noqa: E402
from mpmavatar_amd.shading import ShadowSampler  # noqa: E402

SH_C0 = 0.28209479177387814


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="/tmp/mpmhip_ao_bake_demo")
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--substeps", type=int, default=150)
    ap.add_argument("--size", type=int, default=384)
    ap.add_argument("--ao-res", type=int, default=256)
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--gaussians-per-face", type=int, default=4)
    a = ap.parse_args(argv)
    sc = scenes.small_sheet()
    sim = harness.build_solver(sc, "cuda:0")
    dev = sim.solver.device
    ne, nt = sc.n_elements, sc.n_traditional
    rest = sim.state.particle_x[ne + nt:]
    n_v = rest.shape[0]

    # the UV mesh: the sheet, then the sphere
    sheet_faces = np.asarray(sc.faces, np.int32)
    sphere_v, sphere_f = np.asarray(sc.mesh_vertices, np.float32), np.asarray(sc.mesh_faces, np.int32)
    faces = np.concatenate([sheet_faces[:, [0, 2, 1]], sphere_f + n_v]).astype(np.int32)
    r = rest.cpu().numpy().astype(np.float64)
    span = lambda x: 0.02 + 0.96 * (x - x.min()) / (x.max() - x.min())
    vt = np.concatenate([np.stack([span(r[:, 0]), span(r[:, 2])], -1), np.full((len(sphere_v), 2), 2.0) + sphere_v[:, [0, 2]]]).astype(np.float32)
    baker = AOBaker(torch.as_tensor(faces, device=dev), vt, faces.copy(), height=a.ao_res, width=a.ao_res, samples=a.samples)
    sphere = torch.as_tensor(sphere_v, device=dev)

    # where each sheet face reads the shadow map: its UV centre, in [-1, 1] with v flipped (scene/mesh_gaussian_model.py:109-111)
    uv_c = torch.as_tensor(vt[sheet_faces].mean(1), device=dev)
    sampler = ShadowSampler(torch.stack([2.0 * uv_c[:, 0] - 1.0, 1.0 - 2.0 * uv_c[:, 1]], -1).contiguous(), a.ao_res, a.ao_res)

    frames = MeshFrames(torch.as_tensor(sheet_faces, device=dev))
    g = torch.Generator(device=dev).manual_seed(0)
    n_g = a.gaussians_per_face * ne
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)
    binding = torch.arange(ne, device=dev, dtype=torch.int32).repeat_interleave(a.gaussians_per_face)
    face_x = rest[torch.as_tensor(sheet_faces, device=dev).long()].mean(1)[binding.long()]
    stripes = 0.5 + 0.5 * torch.sin(40.0 * face_x[:, 0]) * torch.sin(40.0 * face_x[:, 2])
    colors = torch.stack([0.55 + 0.4 * stripes, 0.75 - 0.2 * stripes, 0.5 + 0.1 * stripes], 1)
    gaussians = BoundGaussians(0.35 * rnd(n_g, 3) * torch.tensor([1.0, 1.0, 0.05], device=dev), rnd(n_g, 4), -0.6 + 0.2 * rnd(n_g, 3),
                               3.0 + rnd(n_g, 1), ((colors - 0.5) / SH_C0)[:, None, :].contiguous(), torch.zeros(n_g, 0, 3, device=dev), binding)
    centre = rest.mean(0).cpu().numpy()
    view, proj, campos, tanfov = look_at_camera(centre + np.array([0.0, -1.1, -0.9]), centre + np.array([0.0, -0.1, 0.0]), 45.0, dev)  # from below
    settings = GaussianRasterizationSettings(image_height=a.size, image_width=a.size, tanfovx=tanfov, tanfovy=tanfov,
                                             bg=torch.ones(3, device=dev), scale_modifier=1.0, viewmatrix=view, projmatrix=proj,
                                             sh_degree=0, campos=campos, prefiltered=False, debug=False)
    t = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    bake_ms, mean_ao = 0.0, []
    for frame in range(a.frames):
        harness.run(sim, a.substeps, fused=True)
        verts = sim.state.particle_x[ne + nt:]
        t[0].record()
        ao = baker.bake(torch.cat([verts, sphere]))                                  # in place of uvmesh/NNN.obj -> Blender -> aomap/NNN.png
        t[1].record()
        shadow_map = ao[None, None]                                                  # the reference: shadow_net(ao_map)["shadow_map"]
        frames.set_mesh_by_verts(verts.contiguous())
        args = gaussians.render_inputs(frames)
        shaded = gaussians.shaded_colors(args["means3D"], campos, 0, shadow_map=shadow_map, sampler=sampler)
        args = gaussians.render_inputs(frames, override_color=shaded)
        image, _, _, mask, radii, _ = GaussianRasterizer(raster_settings=settings)(**args)
        torch.cuda.synchronize()
        bake_ms += t[0].elapsed_time(t[1])
        covered = baker.coverage[0] >= 0
        assert torch.isfinite(image).all() and torch.isfinite(ao).all() and mask.max() > 0.5 and (radii > 0).any()
        assert 0.0 <= float(ao.min()) and float(ao.max()) <= 1.0 and float(ao[covered].max()) > 0.9
        mean_ao.append(float(ao[covered].mean()))
        baker.write_png(os.path.join(a.out, "aomap"), frame + 1, ao)
        io_formats.write_png(os.path.join(a.out, f"frame_{frame + 1:03d}.png"), image.cpu().numpy())
    print(f"{a.frames} frames x {a.substeps} substeps of {sc.name}: AO bake of {len(faces)} faces at {a.ao_res} x {a.ao_res}, S = {a.samples}: "
          f"{bake_ms / a.frames:.2f} ms/frame (the first frame included); mean AO on the sheet per frame "
          f"{' '.join(f'{m:.3f}' for m in mean_ao)}; aomap/NNN.png and frame_NNN.png under {a.out}")
    return dict(image=image, ao=ao, mean_ao=mean_ao)


if __name__ == "__main__":
    main()
