#!/usr/bin/env python
"""The appearance-training loop with every step of it on the device, the chain of examples/appearance_step_demo.py carried on through
the optimiser (train_appearance.py:112 and :260-261) and across a densification (:245-257):

    once:      groups = appearance_param_groups(...)          the reference's nine groups: xyz, f_dc, f_rest (lr 0), opacity, scaling,
               optimizer = FusedAdam(groups, lr=0.0, eps=1e-15)                       rotation, verts, cams, shadow
    per step:  update_learning_rate(optimizer, iteration)     the xyz and verts schedules
               loss.backward()                                as examples/appearance_step_demo.py --colors --reg
               stats.add(means2D.grad, radii)                 -> mpmhip_densify_stats_add
               optimizer.step()                               -> mpmhip_adam_step: one launch for all groups
               optimizer.zero_grad(set_to_none=True)
    once each: reset_opacity(_opacity, optimizer)             -> mpmhip_reset_opacity, in front of the first iteration
               densify_and_prune(...) + swap_into(optimizer)  -> mpmhip_densify_plan / _emit, half way

    python examples/appearance_train_demo.py [--steps 30] [--size 64] [--shadow-net] [--lpips VGG16.pth LIN.pth] [--image-head]

The scene is the one of appearance_step_demo.py with colours (a 320-face icosphere, two Gaussians per face, degree-1 SH, an 8 x 8
shadow map standing in for the output of the shadow network); ``cams`` is the affine of the rendered image (train_appearance.py:126),
three gains and three offsets.  The rates are this toy scene's, not the reference's defaults, and so are the densification
thresholds (examples/densify_demo.py says why).  The opacities are reset before the first iteration, so every loss printed is part
of the recovery from it; the demo fails if the last loss is not below the first.

``--shadow-net`` puts the first line of the colour path (train_appearance.py:120) in place of the bare map: per step
``AOBaker.bake(verts)`` -> ``ShadowUNet(ao_map)["shadow_map"]`` -> ``shaded_colors``, with ``shadow_net.parameters()`` as the
``shadow`` group.  The sphere's UVs are its vertex directions (front and back share texels; the baker keeps one face per texel),
the AO map is 32 x 32, the network works at 16 x 16 with four channels and hands the 8 x 8 map on.

``--lpips VGG16.pth LIN.pth`` adds the third term of train_appearance.py:133-134, ``lambda_lpips * lpips_net(image[None], gt[None])``
with the reference's lambda_lpips = 0.1, from mpmavatar_amd/lpips.py over the caller's two weight files (torchvision's VGG16 state dict
and the upstream vgg.pth).  Off by default: the weights are not shipped.

``--image-head`` puts the reference's own two lines between the render call and the loss (train_appearance.py:126-127) in place of
the bare affine: ``camera_image(image, alpha, cam_m, cam_c, None)`` of mpmavatar_amd/image_head.py -- the gain is ``exp(cam_m)`` with
``cam_m`` starting at zero, the image is multiplied by the rasteriser's alpha and clipped to [0, 1], in one launch forward and two
backward.  Without the flag the example runs as it always did.
"""
import argparse
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from appearance_step_demo import MAP_SIZE, SH_DEGREE, Scene  # noqa: E402
from mpmavatar_amd.ao_bake import AOBaker  # noqa: E402
from mpmavatar_amd.densify import DensifyStats, adam_moments, densify_and_prune, reset_opacity  # noqa: E402
from mpmavatar_amd.image_head import camera_image, compose_gt  # noqa: E402
from mpmavatar_amd.image_loss import image_loss  # noqa: E402
from mpmavatar_amd.lpips import LPIPS  # noqa: E402
from mpmavatar_amd.optim import FusedAdam, appearance_param_groups, update_learning_rate  # noqa: E402
from mpmavatar_amd.rasterizer import GaussianRasterizer  # noqa: E402
from mpmavatar_amd.render_inputs import BoundGaussians  # noqa: E402
from mpmavatar_amd.shadow_net import ShadowUNet  # noqa: E402

EXTENT = 1.0
LAMBDA_LPIPS = 0.1                      # arguments/__init__.py
AO_SIZE = 32
# the names of arguments/__init__.py:115-126 with rates for this scene
OPT = SimpleNamespace(position_lr_init=5e-3, position_lr_final=5e-4, position_lr_delay_mult=0.01, position_lr_max_steps=30,
                      verts_lr_init=1e-3, verts_lr_final=1e-4, verts_lr_delay_mult=0.01, verts_lr_max_steps=30, feature_lr=1e-2,
                      opacity_lr=5e-2, scaling_lr=1e-2, rotation_lr=1e-2)


class TrainScene(Scene):
    """the scene of appearance_step_demo.py --colors whose render keeps ``means2D`` as a leaf and whose image passes the camera's
    affine"""

    def __init__(self, size, shadow_net=False, lpips=None, image_head=False):
        super().__init__(size, colors=True)
        dev = self.verts_orig.device
        self.lpips_net = LPIPS.from_checkpoints(*lpips).to(dev) if lpips else None
        self.image_head = image_head                     # cam_m is then the logarithm of the gain: it starts at zero
        self.cam_m = torch.nn.Parameter(torch.zeros(3, device=dev) if image_head else torch.ones(3, device=dev))
        self.cam_c = torch.nn.Parameter(torch.zeros(3, device=dev))
        if image_head:                  # train_appearance.py:108: the ground truth is composed with ITS mask, the target render's alpha
            self.target = compose_gt(self.target, self.alpha)
        self.baker = self.shadow_net = None
        if shadow_net:
            direction = self.verts_orig / self.verts_orig.norm(dim=1, keepdim=True)
            vt = (0.5 + 0.5 * direction[:, :2]).cpu().numpy().astype(np.float32)
            self.baker = AOBaker(self.frames.faces, vt, self.frames.faces.cpu().numpy().astype(np.int32), height=AO_SIZE, width=AO_SIZE,
                                 samples=64)
            with torch.no_grad():
                ao_mean = self.baker.bake(self.verts_orig)[None].cpu()
            self.shadow_net = ShadowUNet(uv_size=MAP_SIZE, ao_mean=ao_mean, shadow_size=16, n_dims=4, biases=False).to(dev)

    def render(self):
        self.frames.set_mesh_by_verts(self.verts_orig + self.verts_offset)
        if getattr(self, "shadow_net", None) is not None:       # train_appearance.py:120: this frame's AO map through the network
            self.shadow_map = self.shadow_net(self.baker.bake((self.verts_orig + self.verts_offset).detach())[None])["shadow_map"]
        args = self.gaussians.render_inputs(self.frames, override_color=self.colors)
        args["colors_precomp"] = self.gaussians.shaded_colors(args["means3D"], self.campos, SH_DEGREE, shadow_map=self.shadow_map, sampler=self.sampler)
        self.means2D = args["means2D"].requires_grad_(torch.is_grad_enabled())
        image, _, _, self.alpha, radii, _ = GaussianRasterizer(raster_settings=self.settings)(**args)
        return image, radii

    def loss(self):
        image, radii = self.render()
        if self.image_head:             # train_appearance.py:126-127
            image = camera_image(image, self.alpha, self.cam_m, self.cam_c, None)
        else:
            image = image * self.cam_m[:, None, None] + self.cam_c[:, None, None]
            image = image.contiguous()
        loss = image_loss(image, self.target, 0.2)[0]
        if self.lpips_net is not None:  # train_appearance.py:133-134
            loss = loss + LAMBDA_LPIPS * self.lpips_net(image.unsqueeze(0), self.target.unsqueeze(0)).reshape(())
        return loss, radii


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--shadow-net", action="store_true", help="train a ShadowUNet behind AOBaker in place of the bare shadow map")
    ap.add_argument("--lpips", nargs=2, metavar=("VGG16.pth", "LIN.pth"), default=None,
                    help="add lambda_lpips * LPIPS from these two weight files (torchvision's VGG16 state dict, the upstream vgg.pth)")
    ap.add_argument("--image-head", action="store_true",
                    help="the reference's affine, mask and clip between the render call and the loss: mpmavatar_amd.image_head.camera_image")
    a = ap.parse_args(argv)
    sc = TrainScene(a.size, a.shadow_net, a.lpips, a.image_head)
    if a.image_head:
        print("image head: camera_image(image, alpha, cam_m, cam_c, None) between the render call and the loss")
    p = sc.params
    shadow = list(sc.shadow_net.parameters()) if a.shadow_net else [p["shadow_map"]]
    groups = appearance_param_groups(p["_xyz"], p["_features_dc"], p["_features_rest"], p["_opacity"], p["_scaling"], p["_rotation"],
                                     p["verts_offset"], [sc.cam_m, sc.cam_c], shadow, OPT, spatial_lr_scale=1.0)
    opt = FusedAdam(groups, lr=0.0, eps=1e-15)
    p["_opacity"] = reset_opacity(p["_opacity"], opt)
    print(f"reset_opacity: every opacity at most {float(torch.sigmoid(p['_opacity'].detach()).max()):.3f}")
    rebuild = lambda dc, rest, binding: BoundGaussians(p["_xyz"], p["_rotation"], p["_scaling"], p["_opacity"], dc, rest, binding)
    sc.gaussians = rebuild(p["_features_dc"], p["_features_rest"], sc.gaussians.binding)
    stats = DensifyStats(p["_xyz"].shape[0], p["_xyz"].device)
    rest_start = p["_features_rest"].detach().clone()
    losses = []
    for iteration in range(1, a.steps + 1):
        rates = update_learning_rate(opt, iteration)
        loss, radii = sc.loss()
        loss.backward()
        stats.add(sc.means2D.grad, radii)
        opt.step()
        opt.zero_grad(set_to_none=True)
        losses.append(float(loss.detach()))
        print(f"iteration {iteration:3d}  loss {losses[-1]:.6f}  xyz lr {rates['xyz']:.2e}  verts lr {rates['verts']:.2e}  {stats.n} Gaussians")
        if iteration == a.steps // 2:
            g, n = sc.gaussians, stats.n
            mean_grad = torch.nan_to_num(stats.xyz_gradient_accum / stats.denom).reshape(-1)
            world = (torch.exp(g._scaling.detach()) * sc.frames.face_scaling.detach()[g.binding.long()]).amax(1)
            res = densify_and_prune(g._xyz, g._features_dc, g._features_rest, g._opacity, g._scaling, g._rotation, g.binding, sc.frames.faces.shape[0],
                                    sc.frames.face_scaling, stats, float(torch.quantile(mean_grad, 0.7)), 0.005, EXTENT, 20,
                                    float(world.median()) / EXTENT, moments=adam_moments(opt),
                                    generator=torch.Generator(device=g._xyz.device).manual_seed(0))
            p.update(res.swap_into(opt))
            sc.gaussians = rebuild(p["_features_dc"], p["_features_rest"], res.binding)
            sc.colors = sc.colors[res.src.long()].contiguous()
            rest_start = rest_start[res.src.long()]
            print(f"densification: {n} -> {res.n_out} Gaussians ({res.n_cloned} cloned, {res.n_split} split, {res.n_pruned} pruned)")
            assert res.n_out != n and stats.n == res.n_out and float(opt.state[p["_xyz"]]["step"]) == iteration
    assert torch.equal(p["_features_rest"].detach(), rest_start) and opt.state[p["_features_rest"]]["exp_avg"].any()      # lr == 0: moments only
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    print(f"loss {losses[0]:.6f} -> {losses[-1]:.6f} in {a.steps} steps of FusedAdam over {', '.join(g['name'] for g in opt.param_groups)}")
    return losses


if __name__ == "__main__":
    main()
