#!/usr/bin/env python
"""One appearance-training loop on the device, the call sequence of the reference's train_appearance.py:97-160 without its dataset:

    per step:  verts = verts_orig + verts_offset            (select_mesh_by_timestep, scene/mesh_gaussian_model.py:122-134)
               frames.set_mesh_by_verts(verts)              -> mpmhip_face_frames
               args = gaussians.render_inputs(frames, ...)  -> mpmhip_render_inputs
               image = GaussianRasterizer(settings)(**args) -> mpmhip_raster_forward_grad
               loss, Ll1, ssim = image_loss(image, target)  -> mpmhip_image_loss_forward
               loss.backward()                              -> image loss, rasteriser, binding and face-frame backward kernels
               optimizer.step()                             (torch.optim.Adam, as the reference)

    python examples/appearance_step_demo.py [--steps 30] [--size 64] [--colors] [--reg]

The mesh is a 320-face icosphere with two Gaussians per face.  The target image is rendered from perturbed parameters and perturbed
vertices; Adam then moves ``_xyz``, ``_rotation``, ``_scaling``, ``_opacity`` and a per-vertex ``verts_offset`` towards it, and the
loss it prints falls.  Without ``--colors`` the colours are fixed (``override_color``).  With it they are the reference's
``shadow * convert_SH(...)`` (train_appearance.py:120-123) in one more launch, ``gaussians.shaded_colors`` -> mpmhip_shade_colors:
degree-1 SH features and an 8 x 8 shadow map (a leaf standing in for the output of the shadow network, which stays the caller's
torch module) are leaves too, and the target is rendered from perturbed ones.  With ``--reg`` the six regularisation terms of
train_appearance.py:136-150 are added to the loss with the weights of train_appearance.py:87 and the thresholds of
arguments/__init__.py:137-138, in two more calls, ``MeshRegularizer`` -> mpmhip_mesh_reg_forward and ``gaussian_regularizers`` ->
mpmhip_gauss_reg_forward, and printed.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpmavatar_amd import garment  # noqa: E402
from mpmavatar_amd.image_loss import image_loss  # noqa: E402
from mpmavatar_amd.mesh_frames import MeshFrames  # noqa: E402
from mpmavatar_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer, look_at_camera  # noqa: E402
from mpmavatar_amd.regularizers import MeshRegularizer, gaussian_terms  # noqa: E402
from mpmavatar_amd.render_inputs import BoundGaussians  # noqa: E402
from mpmavatar_amd.shading import ShadowSampler  # noqa: E402

PER_FACE = 2
SH_DEGREE, MAP_SIZE = 1, 8
REG_NAMES = ("normal", "iso", "eq_faces_weight", "opacity", "xyz", "scale")
REG_WEIGHTS = (0.1, 20.0, 1000.0, 0.05, 1.0, 1.0)        # train_appearance.py:87
THRESHOLD_XYZ, THRESHOLD_SCALE = 1.0, 0.6                # arguments/__init__.py:137-138


class Scene:
    """Everything one training step needs; ``params`` are the five leaves the optimiser moves (eight with ``colors``)."""

    def __init__(self, size=64, device="cuda:0", seed=0, eye=(0.0, 0.3, -2.0), colors=False, reg=False):
        dev = torch.device(device)
        g = torch.Generator(device="cpu").manual_seed(seed)
        rnd = lambda *s: torch.randn(*s, generator=g)
        verts, faces = garment.icosphere(2, 0.5, (0.0, 0.0, 0.0))
        self.verts_orig = torch.tensor(np.asarray(verts, np.float32), device=dev)
        self.frames = MeshFrames(torch.tensor(np.asarray(faces, np.int32), device=dev))
        self.reg = MeshRegularizer(self.frames.faces, self.verts_orig) if reg else None
        self.reg_weights, self.reg_terms = torch.tensor(REG_WEIGHTS, device=dev), None
        n_f = faces.shape[0]
        n = PER_FACE * n_f
        binding = torch.arange(n_f, dtype=torch.int32).repeat_interleave(PER_FACE).to(dev)
        # the parameters the target image was rendered from, and the perturbed ones training starts at
        true = {"_xyz": 0.3 * rnd(n, 3) * torch.tensor([1.0, 1.0, 0.05]), "_rotation": rnd(n, 4), "_scaling": -0.7 + 0.2 * rnd(n, 3),
                "_opacity": 1.5 + rnd(n, 1)}
        start = {"_xyz": true["_xyz"] + 0.1 * rnd(n, 3), "_rotation": true["_rotation"] + 0.3 * rnd(n, 4),
                 "_scaling": true["_scaling"] + 0.3 * rnd(n, 3), "_opacity": true["_opacity"] + rnd(n, 1)}
        true_offset = 0.01 * rnd(*self.verts_orig.shape)
        centre = self.verts_orig[self.frames.faces.long()].mean(1)[binding.long()]
        self.colors = (0.5 + centre / (2 * centre.norm(dim=1, keepdim=True))).contiguous()       # colour by direction, fixed
        view, proj, campos, tanfov = look_at_camera(np.array(eye, np.float64), np.zeros(3), 40.0, dev)
        self.settings = GaussianRasterizationSettings(image_height=size, image_width=size, tanfovx=tanfov, tanfovy=tanfov,
                                                      bg=torch.ones(3, device=dev), scale_modifier=1.0, viewmatrix=view, projmatrix=proj,
                                                      sh_degree=0, campos=campos, prefiltered=False, debug=False)
        sh_true = sh_start = (torch.zeros(n, 1, 3, device=dev), torch.zeros(n, 0, 3, device=dev))
        self.campos, self.sampler, self.shadow_map = campos, None, None
        if colors:
            # the colour by direction as the DC term (colour = C0 dc + 0.5), a little view dependence, and a shadow that darkens one side;
            # each face samples the map at the direction of its centre
            k = (SH_DEGREE + 1) ** 2
            dc = ((self.colors - 0.5) / 0.28209479177387814).cpu()[:, None, :]
            sh_true = (dc.to(dev).contiguous(), (0.1 * rnd(n, k - 1, 3)).to(dev))
            sh_start = ((dc + 0.5 * rnd(n, 1, 3)).to(dev).contiguous(), torch.zeros(n, k - 1, 3, device=dev))
            face_centre = self.verts_orig[self.frames.faces.long()].mean(1)
            self.sampler = ShadowSampler((face_centre / face_centre.norm(dim=1, keepdim=True))[:, :2].contiguous(), MAP_SIZE, MAP_SIZE)
            ramp = torch.linspace(0.4, 1.0, MAP_SIZE)
            map_true, map_start = (ramp[None, :] * torch.ones(MAP_SIZE, 1)).to(dev), torch.full((MAP_SIZE, MAP_SIZE), 0.8, device=dev)
        with torch.no_grad():
            self.verts_offset = true_offset.to(dev)
            self.gaussians = BoundGaussians(*[true[k].to(dev).contiguous() for k in ("_xyz", "_rotation", "_scaling", "_opacity")], *sh_true, binding)
            if colors:
                self.shadow_map = map_true
            self.target = self.render()[0]
        self.verts_offset = torch.nn.Parameter(torch.zeros_like(self.verts_orig))
        leaves = [torch.nn.Parameter(start[k].to(dev).contiguous()) for k in ("_xyz", "_rotation", "_scaling", "_opacity")]
        self.params = dict(zip(("_xyz", "_rotation", "_scaling", "_opacity"), leaves), verts_offset=self.verts_offset)
        if colors:
            sh_start = tuple(torch.nn.Parameter(t) for t in sh_start)
            self.shadow_map = torch.nn.Parameter(map_start)
            self.params.update(_features_dc=sh_start[0], _features_rest=sh_start[1], shadow_map=self.shadow_map)
        self.gaussians = BoundGaussians(*leaves, *sh_start, binding)

    def render(self):
        """-> (image [3, size, size], radii [n]) from the current parameters"""
        self.frames.set_mesh_by_verts(self.verts_orig + self.verts_offset)
        args = self.gaussians.render_inputs(self.frames, override_color=self.colors)
        if self.sampler is not None:             # train_appearance.py:120-123: the colours of this step, from this step's means3D
            args["colors_precomp"] = self.gaussians.shaded_colors(args["means3D"], self.campos, SH_DEGREE, shadow_map=self.shadow_map,
                                                                  sampler=self.sampler)
        image, _, _, _, radii, _ = GaussianRasterizer(raster_settings=self.settings)(**args)
        return image, radii

    def loss(self):
        """-> (loss, radii): train_appearance.py:132,134 without the LPIPS term, plus the regularisers of :136-150 with ``reg``"""
        image, radii = self.render()
        loss = image_loss(image, self.target, 0.2)[0]
        if self.reg is not None:
            p = self.params
            terms = torch.cat([self.reg.terms(self.frames.verts), gaussian_terms(p["_opacity"], p["_xyz"], p["_scaling"], radii, THRESHOLD_XYZ,
                                                                                THRESHOLD_SCALE)])
            self.reg_terms = terms.detach()
            loss = loss + (self.reg_weights * terms).sum()
        return loss, radii


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--colors", action="store_true", help="train SH features and a shadow map too (mpmhip_shade_colors)")
    ap.add_argument("--reg", action="store_true", help="add the six weighted regularisation terms (mpmhip_mesh_reg_*, mpmhip_gauss_reg_*)")
    a = ap.parse_args(argv)
    sc = Scene(a.size, colors=a.colors, reg=a.reg)
    lr = {"_xyz": 5e-3, "_rotation": 1e-2, "_scaling": 1e-2, "_opacity": 2e-2, "verts_offset": 1e-3, "_features_dc": 1e-2,
          "_features_rest": 5e-3, "shadow_map": 1e-2}
    opt = torch.optim.Adam([{"params": [p], "lr": lr[k], "name": k} for k, p in sc.params.items()], eps=1e-15)
    losses = []
    for step in range(a.steps + 1):
        opt.zero_grad(set_to_none=True)
        loss, radii = sc.loss()
        losses.append(float(loss.detach()))
        if step % 5 == 0:
            print(f"step {step:3d}  loss {losses[-1]:.6f}  ({int((radii > 0).sum())} of {radii.numel()} Gaussians on screen)")
            if a.reg:
                print("          " + "  ".join(f"{k} {v:.3g}" for k, v in zip(REG_NAMES, sc.reg_terms.tolist())))
        if step == a.steps:
            break
        loss.backward()
        opt.step()
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    print(f"loss {losses[0]:.6f} -> {losses[-1]:.6f} in {a.steps} Adam steps over {', '.join(sc.params)}")
    return losses


if __name__ == "__main__":
    main()
