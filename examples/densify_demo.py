#!/usr/bin/env python
"""An appearance-training loop that crosses one densification, the last block of the reference's loop (train_appearance.py:245-257)
on the device:

    per step:  loss.backward()                                  as examples/appearance_step_demo.py
               stats.add(means2D.grad, radii)                   -> mpmhip_densify_stats_add (max_radii2D, xyz_gradient_accum, denom)
               optimizer.step()
    once:      res = densify_and_prune(..., stats, ...)         -> mpmhip_densify_plan, one read-back, mpmhip_densify_emit
               res.swap_into(optimizer, names)                  the new parameters and Adam moments; `step` stays
               reset_opacity(_opacity, optimizer, name)         -> mpmhip_reset_opacity (with --reset)
    then the same steps on the grown set.

    python examples/densify_demo.py [--steps 12] [--size 64] [--reset]

The scene is the one of appearance_step_demo.py (a 320-face icosphere, two Gaussians per face, fixed colours).  The reference's
thresholds presume its images and its scene: densify_grad_threshold = 0.0002 is a gradient in its pixels and percent_dense = 0.01 a
fraction of its scene radius.  This toy scene has neither, so the demo takes max_grad and the dense limit from the statistics it has
just gathered (the 70th percentile of the mean gradient, the median world scale), which makes it clone, split and prune whatever
the image size; a trainer passes the reference's constants.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from appearance_step_demo import Scene  # noqa: E402
from mpmavatar_amd.densify import DensifyStats, adam_moments, densify_and_prune, reset_opacity  # noqa: E402
from mpmavatar_amd.rasterizer import GaussianRasterizer  # noqa: E402
from mpmavatar_amd.render_inputs import BoundGaussians  # noqa: E402

GAUSSIAN_LEAVES = ("_xyz", "_rotation", "_scaling", "_opacity")
LR = {"_xyz": 5e-3, "_rotation": 1e-2, "_scaling": 1e-2, "_opacity": 2e-2, "verts_offset": 1e-3}
EXTENT = 1.0                                  # the icosphere's diameter


class DensifyScene(Scene):
    """the scene of appearance_step_demo.py whose render keeps ``means2D`` as a leaf, as the reference keeps its screenspace_points"""

    def render(self):
        self.frames.set_mesh_by_verts(self.verts_orig + self.verts_offset)
        args = self.gaussians.render_inputs(self.frames, override_color=self.colors)
        self.means2D = args["means2D"].requires_grad_(torch.is_grad_enabled())
        image, _, _, _, radii, _ = GaussianRasterizer(raster_settings=self.settings)(**args)
        return image, radii


def steps(sc, opt, stats, count, losses):
    for _ in range(count):
        opt.zero_grad(set_to_none=True)
        loss, radii = sc.loss()
        loss.backward()
        stats.add(sc.means2D.grad, radii)
        opt.step()
        losses.append(float(loss.detach()))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12, help="Adam steps before the densification, and again after it")
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--reset", action="store_true", help="reset_opacity after the densification too")
    a = ap.parse_args(argv)
    sc = DensifyScene(a.size)
    opt = torch.optim.Adam([{"params": [p], "lr": LR[k], "name": k} for k, p in sc.params.items()], eps=1e-15)
    g = sc.gaussians
    n = g._xyz.shape[0]
    stats = DensifyStats(n, g._xyz.device)
    losses = []
    steps(sc, opt, stats, a.steps, losses)

    # thresholds from the statistics (module docstring); a trainer passes opt.densify_grad_threshold and opt.percent_dense
    mean_grad = torch.nan_to_num(stats.xyz_gradient_accum / stats.denom).reshape(-1)
    world = (torch.exp(g._scaling.detach()) * sc.frames.face_scaling.detach()[g.binding.long()]).amax(1)
    max_grad, dense = float(torch.quantile(mean_grad, 0.7)), float(world.median())
    names = {k: k for k in GAUSSIAN_LEAVES}
    res = densify_and_prune(g._xyz, g._features_dc, g._features_rest, g._opacity, g._scaling, g._rotation, g.binding, sc.frames.faces.shape[0],
                            sc.frames.face_scaling, stats, max_grad, 0.005, EXTENT, 20, dense / EXTENT, moments=adam_moments(opt, names),
                            generator=torch.Generator(device=g._xyz.device).manual_seed(0))
    new = res.swap_into(opt, names)
    if a.reset:
        new["_opacity"] = reset_opacity(new["_opacity"], opt, "_opacity")
    sc.params.update(new)
    sc.gaussians = BoundGaussians(new["_xyz"], new["_rotation"], new["_scaling"], new["_opacity"], res._features_dc, res._features_rest, res.binding)
    sc.colors = sc.colors[res.src.long()].contiguous()
    print(f"densification: {n} -> {res.n_out} Gaussians ({res.n_cloned} cloned, {res.n_split} split, {res.n_pruned} pruned); "
          f"every face keeps {int(res.binding_counter.min())} .. {int(res.binding_counter.max())}")
    assert res.n_out != n and res.n_cloned > 0 and res.n_split > 0 and int(res.binding_counter.min()) >= 1 and stats.n == res.n_out
    assert all(opt.state[new[k]]["exp_avg"].shape == new[k].shape and float(opt.state[new[k]]["step"]) == a.steps for k in GAUSSIAN_LEAVES)

    before = len(losses)
    steps(sc, opt, stats, a.steps, losses)
    assert all(np.isfinite(losses)) and losses[before - 1] < losses[0] and losses[-1] < losses[before], losses
    print(f"loss {losses[0]:.6f} -> {losses[before - 1]:.6f} on {n} Gaussians, {losses[before]:.6f} -> {losses[-1]:.6f} on {res.n_out}")
    return losses, res


if __name__ == "__main__":
    main()
