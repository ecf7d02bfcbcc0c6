#!/usr/bin/env python
"""One mesh-tracking loop on the device, the call sequence of the reference's preprocess/train_mesh_lbs_actorshq.py (get_loss :228-303)
without its dataset, its SMPL-X forward and pytorch3d:

    per step:  rendervar = fg.render_vars(vertices, log_scales, logit_opacities)   -> mpmhip_track_render_vars   (params2rendervar)
               im, _, _, msk, radius, _ = GaussianRasterizer(cam)(**rendervar)     -> mpmhip_raster_forward_grad
               im = exp(cam_m[id])[:, None, None] * im + cam_c[id][:, None, None]  (torch: three ops, no mask at this stage)
               losses['im'] = image_loss(im, gt, 0.2); losses['msk'] = l1_loss(msk, gt_msk)
               losses['area'], ['scale'], ['opacity'] = fg.losses(...)             -> mpmhip_track_terms_forward
               losses['normal'], ['iso'], ['eq_faces_weight'] = reg(vertices)      -> mpmhip_mesh_reg_forward
               losses['collision_l'] = collision_penalty(vertices[cloth_v_idx], smplx_v, smplx_vn)   -> mpmhip_track_collision_forward
               loss.backward(); optimizer.step()                                   (FusedAdam, initialize_optimizer's groups :182-193)

    python examples/tracking_step_demo.py [--steps 30] [--size 64] [--cloth-mask] [--dress4d]

``--cloth-mask`` adds the 4D-DRESS script's garment term (preprocess/train_mesh_lbs_4ddress.py:260-277, :299, :306): a synthetic
two-garment labelling of the faces (upper: face centre above the equator, lower: below) goes in as ``extra_attrs``, the rasteriser's
sixth slot is the rendered garment mask, and ``losses['cloth_mask'] = l1_loss(cloth_mask, gt_cloth_mask)`` enters with weight 2.

``--dress4d`` adds the other terms of that script's first timestep: ``losses['laplacian'] = lap.loss(vertices)`` (:363, weight 1;
``MeshLaplacian`` stands for the dense ``laplacian_matrix`` of :212-214 -> mpmhip_track4d_laplacian_forward) and ``scale_ratio``,
``scale_edge_ratio``, ``scale_edge_ratio_var`` = ``fg.scale_ratio_losses(vertices, rendervar['scales'])`` (:361, weights 10, 1000, 10
-> mpmhip_track4d_scale_ratio_forward).

The mesh is a 320-face icosphere of radius 0.5 with one Gaussian per face and a smaller sphere inside as the body, its vertex normals
from ``VertexNormals``.  The ground-truth image and mask are rendered from a displaced copy of the mesh with other colours; Adam then
moves ``vertices``, ``rgb_colors``, ``logit_opacities``, ``log_scales``, ``cam_m`` and ``cam_c`` with the reference's learning rates
and the loss it prints falls.  The weights are the reference's defaults (:287-291 and its argparse defaults).
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpmavatar_amd import garment  # noqa: E402
from mpmavatar_amd.image_loss import image_loss, l1_loss  # noqa: E402
from mpmavatar_amd.optim import FusedAdam  # noqa: E402
from mpmavatar_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer, look_at_camera  # noqa: E402
from mpmavatar_amd.regularizers import MeshRegularizer  # noqa: E402
from mpmavatar_amd.tracking import FaceGaussians, MeshLaplacian, VertexNormals, collision_penalty  # noqa: E402

# loss_weights of get_loss (:287-291) with the argparse defaults (:545-553)
WEIGHTS = {"im": 1.0, "msk": 1.0, "scale": 1.0, "normal": 0.1, "opacity": 0.05, "iso": 20.0, "area": 50.0, "eq_faces_weight": 1000.0,
           "collision_l": 10.0, "cloth_mask": 2.0,               # cloth_mask: train_mesh_lbs_4ddress.py:306, the 4D-DRESS script alone
           "laplacian": 1.0, "scale_ratio": 10.0, "scale_edge_ratio": 1000.0, "scale_edge_ratio_var": 10.0}      # :369, likewise
LR_MEANS3D, LR_COLORS = 0.00004, 0.0025                  # --lr_means3D, --lr_colors


class Scene:
    """Everything one tracking step needs; ``params`` are the six leaves of the reference's ``params`` dict."""

    def __init__(self, size=64, device="cuda:0", seed=0, eye=(0.0, 0.3, -2.0), cloth_mask=False, dress4d=False):
        dev = torch.device(device)
        g = torch.Generator(device="cpu").manual_seed(seed)
        rnd = lambda *s: torch.randn(*s, generator=g)
        verts, faces = garment.icosphere(2, 0.5, (0.0, 0.0, 0.0))
        body_v, body_f = garment.icosphere(2, 0.4995, (0.0, 0.0, 0.0))           # 0.0005 inside the cloth: closer than eps, the hinge is active
        verts0 = torch.tensor(np.asarray(verts, np.float32), device=dev)
        self.faces = torch.tensor(np.asarray(faces, np.int32), device=dev)
        self.fg = FaceGaussians(self.faces)
        self.reg = MeshRegularizer(self.faces, verts0)                           # neighbor_dist, neighbor_weight from the first frame
        self.lap = MeshLaplacian(self.faces) if dress4d else None                # in place of variables['laplacian_matrix']
        self.smplx_v = torch.tensor(np.asarray(body_v, np.float32), device=dev)
        self.smplx_vn = VertexNormals(torch.tensor(np.asarray(body_f, np.int32), device=dev))(self.smplx_v)
        self.cloth_v_idx = torch.arange(verts0.shape[0], device=dev)
        n_f = self.faces.shape[0]
        view, proj, campos, tanfov = look_at_camera(np.array(eye, np.float64), np.zeros(3), 40.0, dev)
        self.cam = GaussianRasterizationSettings(image_height=size, image_width=size, tanfovx=tanfov, tanfovy=tanfov,
                                                 bg=torch.zeros(3, device=dev), scale_modifier=1.0, viewmatrix=view, projmatrix=proj,
                                                 sh_degree=0, campos=campos, prefiltered=False, debug=False)
        scene_radius = 1.1 * float(np.linalg.norm(eye))                          # 1.1 x the farthest camera, as the reference takes it
        # one disc per face: the radius of a disc of the face's area, flat along the normal (log_scales[:, 2] = -100)
        log_scales = torch.full((n_f, 3), -100.0, device=dev)
        log_scales[:, :2] = 0.5 * torch.log(self.fg.face_areas(verts0) / torch.pi)[:, None]
        centre = verts0[self.faces.long()].mean(1)
        colour = (0.5 + centre / (2 * centre.norm(dim=1, keepdim=True))).contiguous()                 # colour by direction
        # variables['cloth_mask'] of the 4D-DRESS script: [F, 2], upper and lower garment, 0 / 1 (data, not trained)
        upper = (centre[:, 1] > 0).float()
        self.cloth_table = torch.stack([upper, 1 - upper], 1).contiguous() if cloth_mask else None
        # the ground truth: a displaced copy (2 % larger, 0.004 of noise) with shifted colours and a camera gain
        with torch.no_grad():
            self.params = {"vertices": (1.02 * verts0 + 0.004 * rnd(*verts0.shape).to(dev)).contiguous(),
                           "rgb_colors": (colour + 0.1 * rnd(n_f, 3).to(dev)).clamp(0, 1).contiguous(), "logit_opacities": torch.full((n_f, 1), 3.0, device=dev),
                           "log_scales": log_scales, "cam_m": torch.full((1, 3), 0.05, device=dev), "cam_c": torch.full((1, 3), 0.02, device=dev)}
            self.gt_im, self.gt_msk, _, self.gt_cloth_mask = self.render()
        self.params = {"vertices": verts0.clone(), "rgb_colors": colour, "logit_opacities": torch.zeros(n_f, 1, device=dev),
                       "log_scales": log_scales.clone(), "cam_m": torch.zeros(1, 3, device=dev), "cam_c": torch.zeros(1, 3, device=dev)}
        self.params = {k: torch.nn.Parameter(v.contiguous()) for k, v in self.params.items()}
        self.lrs = {"vertices": LR_MEANS3D * scene_radius, "rgb_colors": LR_COLORS, "logit_opacities": 0.05, "log_scales": 0.001, "cam_m": 1e-4,
                    "cam_c": 1e-4}                                               # initialize_optimizer :182-193
        self.losses = {}

    def render(self, curr_id=0):
        """-> (im [3, size, size] behind the camera affine, msk [1, size, size], radius [F], cloth_mask [2, size, size] or None); the
        Gaussians' scales stay in ``self.scales`` for the scale-ratio terms"""
        p = self.params
        rendervar = self.fg.render_vars(p["vertices"], p["log_scales"], p["logit_opacities"], extra_attrs=self.cloth_table)
        self.scales = rendervar["scales"]
        rendervar["colors_precomp"] = p["rgb_colors"]
        rendervar["means2D"] = torch.zeros_like(rendervar["means3D"], requires_grad=True)
        im, _, _, msk, radius, cloth_mask = GaussianRasterizer(raster_settings=self.cam)(**rendervar)
        im = torch.exp(p["cam_m"][curr_id])[:, None, None] * im + p["cam_c"][curr_id][:, None, None]
        return im, msk, radius, cloth_mask

    def loss(self):
        p = self.params
        im, msk, radius, cloth_mask = self.render()
        losses = {"im": image_loss(im, self.gt_im, 0.2)[0], "msk": l1_loss(msk, self.gt_msk)}
        if cloth_mask is not None:
            losses["cloth_mask"] = l1_loss(cloth_mask, self.gt_cloth_mask)       # :306
        losses["area"], losses["scale"], losses["opacity"] = self.fg.losses(p["vertices"], p["log_scales"], p["logit_opacities"])
        losses["normal"], losses["iso"], losses["eq_faces_weight"] = self.reg(p["vertices"])
        losses["collision_l"] = collision_penalty(p["vertices"][self.cloth_v_idx], self.smplx_v, self.smplx_vn, return_average=True)
        if self.lap is not None:                                                 # :361 (the initial timestep) and :363
            losses["scale_ratio"], losses["scale_edge_ratio"], losses["scale_edge_ratio_var"] = self.fg.scale_ratio_losses(p["vertices"], self.scales)
            losses["laplacian"] = self.lap.loss(p["vertices"])
        self.losses = {k: float(v.detach()) for k, v in losses.items()}
        return sum(WEIGHTS[k] * v for k, v in losses.items()), radius


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--cloth-mask", action="store_true")
    ap.add_argument("--dress4d", action="store_true")
    a = ap.parse_args(argv)
    sc = Scene(a.size, cloth_mask=a.cloth_mask, dress4d=a.dress4d)
    opt = FusedAdam([{"params": [v], "name": k, "lr": sc.lrs[k]} for k, v in sc.params.items()], lr=0.0, eps=1e-15)
    losses = []
    for step in range(a.steps + 1):
        opt.zero_grad(set_to_none=True)
        loss, radius = sc.loss()
        losses.append(float(loss.detach()))
        if step % 5 == 0:
            print(f"step {step:3d}  loss {losses[-1]:.6f}  ({int((radius > 0).sum())} of {radius.numel()} Gaussians on screen)")
            print("          " + "  ".join(f"{k} {v:.3g}" for k, v in sc.losses.items()))
        if step == a.steps:
            break
        loss.backward()
        opt.step()
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    print(f"loss {losses[0]:.6f} -> {losses[-1]:.6f}")
    return losses


if __name__ == "__main__":
    main()
