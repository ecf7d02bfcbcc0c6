"""What the rasteriser is handed: from device-resident simulated vertices to the argument lists of the reference's
render call (/root/reference/gaussian_renderer/__init__.py:52-103) without leaving the GPU.

The reference writes every simulated frame to an OBJ file, has Blender bake ambient occlusion, reads the meshes back and only then
poses the Gaussians and renders (train_material_params.py:819-845, run_demo.py:540-604).  The geometry half of that detour is not
needed: ``MeshFrames.set_mesh_by_verts`` takes the solver's ``particle_x`` as it lies in HBM, and ``BoundGaussians.render_inputs``
returns exactly ``means3D, means2D, opacities, scales, rotations`` (+ the caller's ``shs`` / ``colors_precomp`` and the ``extra``
primitives concatenated behind, :84-91) in one launch (``mpmhip_render_inputs``).  The rasteriser they go to is
``mpmavatar_amd/rasterizer.py``; the AO bake is ``mpmavatar_amd/ao_bake.py``, from the same vertices on the device, so the OBJ files (``io_formats.UVMeshWriter``) are needed only by a caller who still wants Blender's bake.

    frames = MeshFrames(faces);  frames.set_mesh_by_verts(sim2wld(state.particle_x[n_e + n_t:]))
    args = gaussians.render_inputs(frames, override_color=colors, extra=(xyz, colors, opacity, scales, rotations))
    rasterizer(**args)          # keys: means3D means2D shs colors_precomp opacities scales rotations cov3Ds_precomp

Training (train_appearance.py).  With grad mode on, ``means3D``, ``opacities``, ``scales`` and ``rotations`` carry a graph back to
whichever of ``_xyz``, ``_rotation``, ``_scaling``, ``_opacity`` (``nn.Parameter`` or not), the four frame tensors and the ``extra``
tensors require grad; the forward is the same launch with the same bits, the backward is ``mpmhip_render_inputs_backward``
(csrc/frames_backward.hip), and the ``extra`` rows get the upstream rows back.  ``colors_precomp`` / ``shs`` are torch's own ``cat``.
``means2D`` stays a fresh zero tensor outside the graph: a trainer that wants ``viewspace_points.grad`` for densification calls
``args["means2D"].requires_grad_(True)`` before the render call, as the reference does with its ``screenspace_points``.  With grad mode
off, or with nothing requiring grad, nothing changes and the outputs carry no ``grad_fn``.
"""
from __future__ import annotations

import torch

from . import _lib as L
from ._call import expect, wants_grad
from .mesh_frames import MeshFrames, _Bind, _GaussianTable, _launch_bind


class BoundGaussians:
    """The parameters of a mesh-bound GaussianModel that the render call reads (scene/gaussian_model.py:45-73): raw ``_xyz`` (face-local),
    ``_rotation``, ``_scaling``, ``_opacity``, ``_features_dc`` / ``_features_rest`` and ``binding`` (Gaussian -> face)."""

    def __init__(self, xyz, rotation, scaling, opacity, features_dc, features_rest, binding):
        self._xyz, self._rotation, self._scaling = expect(xyz, torch.float32, "_xyz", last=3), \
            expect(rotation, torch.float32, "_rotation", last=4), expect(scaling, torch.float32, "_scaling", last=3)
        self._opacity = expect(opacity, torch.float32, "_opacity", last=1)
        self._features_dc, self._features_rest = features_dc, features_rest
        self.binding = expect(binding.to(torch.int32).contiguous(), torch.int32, "binding")
        n = self.binding.numel()
        if not (self._xyz.shape[0] == self._rotation.shape[0] == self._scaling.shape[0] == self._opacity.shape[0] == n):
            raise RuntimeError("BoundGaussians: parameter tensors must have one row per binding entry")
        L.load()                                 # a missing library is reported here, not at the first launch
        self._gtable = _GaussianTable()

    @property
    def get_features(self):  # gaussian_model.py:153-157
        return torch.cat((self._features_dc, self._features_rest), dim=1)

    def shaded_colors(self, means3D, campos, active_sh_degree, shadow_map=None, sampler=None):
        """-> colors [n, 3] for ``override_color`` (train_appearance.py:120-123): the model's SH features seen from ``campos`` at
        ``means3D`` (the ``means3D`` of render_inputs, first n rows), times the shadow map sampled at each Gaussian's face
        (``sampler``: shading.ShadowSampler) where one is given.  One launch, with a backward (mpmavatar_amd/shading.py)."""
        from .shading import shaded_colors
        return shaded_colors(self._features_dc, self._features_rest, active_sh_degree, means3D, campos, binding=self.binding,
                             shadow_map=shadow_map, sampler=sampler, gtable=self._gtable)

    def render_inputs(self, frames: MeshFrames, override_color=None, extra=None):
        """-> dict of the rasteriser's keyword arguments (gaussian_renderer/__init__.py:94-102).  extra = (xyz [m,3], colors [m,3],
        opacity [m,1], scales [m,3], rotations [m,4]) as run_demo.py builds it (needs override_color, like the reference)."""
        if frames.face_center is None:
            raise RuntimeError("call frames.set_mesh_by_verts first")
        dev = self.binding.device
        n, m = self.binding.numel(), 0
        ex = [None] * 5
        if extra is not None:
            if override_color is None:
                raise RuntimeError("extra primitives carry precomputed colours: pass override_color for the bound Gaussians too")
            ex = [expect(t.contiguous(), torch.float32, f"extra[{i}]", last=w) for i, (t, w) in enumerate(zip(extra, (3, 3, 1, 3, 4)))]
            m = ex[0].shape[0]
        fr = (frames.face_center, frames.face_orien_mat, frames.face_orien_quat, frames.face_scaling)
        params, tail = (self._xyz, self._rotation, self._scaling, self._opacity), (ex[0], ex[2], ex[3], ex[4])
        means2D = torch.empty(n + m, 3, dtype=torch.float32, device=dev)     # cleared by the same launch; a fresh leaf, outside the graph
        if wants_grad(*params, *fr, *tail):
            out = _Bind.apply(self._gtable, self.binding, True, means2D.data_ptr(), self.binding, *fr, *params, *tail)
        else:
            out = _launch_bind(True, means2D.data_ptr(), self.binding, fr, params, tail)
        means3D, rots, scales, opac = out
        shs = colors = None
        if override_color is None:
            shs = self.get_features                      # SH -> RGB in the rasteriser (:81)
        else:
            colors = override_color if extra is None else torch.cat([override_color, ex[1]])   # :91
        return {"means3D": means3D, "means2D": means2D, "shs": shs, "colors_precomp": colors, "opacities": opac, "scales": scales,
                "rotations": rots, "cov3Ds_precomp": None}
