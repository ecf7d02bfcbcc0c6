"""Per-face frames and bound Gaussians on the GPU: the step right after the solver in the reference's render loop
(SURVEY.md 8(f) N3).  Mirrors the relevant surface of the reference's ``MeshGaussianModel`` / ``GaussianModel``
(/root/reference/scene/mesh_gaussian_model.py:137-146, scene/gaussian_model.py:112-151) over two HIP kernels
(``mpmhip_face_frames``, ``mpmhip_bind_gaussians``): simulated vertices stay on the device,

    frames = MeshFrames(faces)                       # faces: [n_f, 3] int tensor (cloth + body mesh)
    frames.set_mesh_by_verts(sim2wld(state.particle_x[n_e + n_t:]))
    xyz, rot, scale = frames.get_xyz(binding, _xyz), frames.get_rotation(binding, _rotation), frames.get_scaling(binding, _scaling)

and feed the rasteriser.  No CPU fallback: tensors must live on an MI355X.

Gradients.  With grad mode on, ``set_mesh_by_verts(verts)`` of a ``verts`` that requires grad gives frame tensors that carry a graph
back to ``verts`` (``verts_orig[t] + verts_offset[t]`` of the appearance loop), and the getters give outputs that carry a graph back to
whichever of their floating inputs -- the raw parameters, the four frame tensors -- require grad.  The forward is the same launch
with the same bits; the backward is ``mpmhip_face_frames_backward`` / ``mpmhip_render_inputs_backward`` (csrc/frames_backward.hip):
the exact derivative of the forward kernels' expressions with every discrete decision held fixed (the quaternion branch, the sign
inside the absolute value, a clamp that binds passes zero slope), fp32, no atomics, the same bits on every run.  There is no double
backward.  With grad mode off, or with no floating input requiring grad, nothing changes: the outputs carry no ``grad_fn``.
"""
from __future__ import annotations

import torch

from . import _lib as L
from ._call import call, csr, expect, ptr, upstream, wants_grad


def _launch_face_frames(faces, v):
    n_f = faces.shape[0]
    dev = v.device
    new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    center, mat, quat, scale = new(n_f, 3), new(n_f, 3, 3), new(n_f, 4), new(n_f, 1)
    call("mpmhip_face_frames", dev, v.data_ptr(), faces.data_ptr(), n_f, center.data_ptr(), mat.data_ptr(), quat.data_ptr(), scale.data_ptr())
    return center, mat, quat, scale


def _launch_bind(render, means2D, binding, frame, params, extra):
    """One launch of the binding: mpmhip_render_inputs (``render``: all four parameters, n + m rows with the ``extra`` tensors behind,
    means2D cleared through its pointer) or mpmhip_bind_gaussians (any of xyz / rotation / scaling).  -> (means3D / xyz, rotations,
    scales, opacities), None where a parameter was not given."""
    dev = binding.device
    n, m = binding.numel(), (0 if extra[0] is None else extra[0].shape[0])
    o_xyz, o_rot, o_scl, o_opa = [None if t is None else torch.empty(n + m, w, dtype=torch.float32, device=dev)
                                  for t, w in zip(params, (3, 4, 3, 1))]
    xyz, rot, scl, opa = params
    if render:
        call("mpmhip_render_inputs", dev, n, m, binding.data_ptr(), xyz.data_ptr(), rot.data_ptr(), scl.data_ptr(), opa.data_ptr(),
             *[t.data_ptr() for t in frame], *[ptr(t) for t in extra], o_xyz.data_ptr(), means2D, o_opa.data_ptr(), o_scl.data_ptr(),
             o_rot.data_ptr())
    else:
        call("mpmhip_bind_gaussians", dev, n, binding.data_ptr(), ptr(xyz), ptr(rot), ptr(scl), *[t.data_ptr() for t in frame],
             ptr(o_xyz), ptr(o_rot), ptr(o_scl))
    return o_xyz, o_rot, o_scl, o_opa


class _FaceFrames(torch.autograd.Function):
    """verts -> (face_center, face_orien_mat, face_orien_quat, face_scaling): the forward launch of set_mesh_by_verts with a backward."""

    @staticmethod
    def forward(ctx, verts, faces, vtable):
        out = _launch_face_frames(faces, verts)
        ctx.faces, ctx.vtable = faces, vtable
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(verts, out[1], out[2])
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_center, g_mat, g_quat, g_scale):
        verts, mat, quat = ctx.saved_tensors
        faces = ctx.faces
        n_f, n_v, dev = faces.shape[0], verts.shape[0], verts.device
        start, corners = ctx.vtable.get(faces, n_v)
        g = [upstream(t) for t in (g_center, g_mat, g_quat, g_scale)]
        d_corners = torch.empty(n_f, 3, 3, dtype=torch.float32, device=dev)
        d_verts = torch.empty_like(verts)
        call("mpmhip_face_frames_backward", dev, verts.data_ptr(), faces.data_ptr(), n_f, n_v, mat.data_ptr(), quat.data_ptr(),
             *[ptr(t) for t in g], start.data_ptr(), corners.data_ptr(), d_corners.data_ptr(), d_verts.data_ptr())
        return d_verts, None, None


class _Bind(torch.autograd.Function):
    """The binding launch (mpmhip_render_inputs with ``render``, else mpmhip_bind_gaussians) with a backward.  Outputs: (means3D / xyz,
    rotations, scales, opacities), None where an input was not given; with ``render`` they have n + m rows, the ``extra`` tensors behind.
    ``table`` is the caller's face -> Gaussian table (_GaussianTable); ``key`` is the caller's binding tensor, which the table is
    keyed on; means2D is written through its pointer and is no part of the graph."""

    @staticmethod
    def forward(ctx, table, key, render, means2D, binding, center, mat, quat, fscale, xyz, rot, scl, opa, x_xyz, x_opa, x_scl, x_rot):
        out = _launch_bind(render, means2D, binding, (center, mat, quat, fscale), (xyz, rot, scl, opa), (x_xyz, x_opa, x_scl, x_rot))
        n = binding.numel()
        ctx.table, ctx.n, ctx.n_f = table, n, fscale.shape[0]
        ctx.key = (key, key.data_ptr(), key._version)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(binding, mat, quat, fscale, xyz, rot, scl, opa)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_xyz, g_rot, g_scl, g_opa):
        binding, mat, quat, fscale, xyz, rot, scl, opa = ctx.saved_tensors
        n, n_f, dev = ctx.n, ctx.n_f, binding.device
        need_face, need_param, need_extra = ctx.needs_input_grad[5:9], ctx.needs_input_grad[9:13], ctx.needs_input_grad[13:17]
        g = [upstream(t) for t in (g_xyz, g_rot, g_scl, g_opa)]
        d_xyz, d_rot, d_scl, d_opa = [torch.empty_like(t) if want and t is not None else None
                                      for want, t in zip(need_param, (xyz, rot, scl, opa))]
        d_face = [None] * 4
        start = items = None
        if any(need_face):
            start, items = ctx.table.get(ctx.key, binding, n_f)
            d_face = [torch.empty(n_f, w, dtype=torch.float32, device=dev) for w in (3, 9, 4, 1)]
        call("mpmhip_render_inputs_backward", dev, n, n_f, binding.data_ptr(), ptr(xyz), ptr(rot), ptr(scl), ptr(opa), mat.data_ptr(),
             quat.data_ptr(), fscale.data_ptr(), ptr(g[0]), ptr(g[3]), ptr(g[2]), ptr(g[1]), ptr(d_xyz), ptr(d_rot), ptr(d_scl), ptr(d_opa),
             ptr(start), ptr(items), *[ptr(t) for t in d_face])
        d_center, d_mat, d_quat, d_fscale = [t if want else None for t, want in zip(d_face, need_face)]
        if d_mat is not None:
            d_mat = d_mat.view(n_f, 3, 3)
        # the rows behind the bound Gaussians are the `extra` tensors copied: their gradients are the upstream rows
        tails = [t[n:] if want and t is not None else None for want, t in zip(need_extra, (g[0], g[3], g[2], g[1]))]
        return (None, None, None, None, None, d_center, d_mat, d_quat, d_fscale, d_xyz, d_rot, d_scl, d_opa, *tails)


class _GaussianTable:
    """The face -> Gaussian table of the backward pass, built at the first backward and kept while the binding tensor it was built
    from is the same storage at the same version: densification (a new tensor) or an in-place edit rebuilds it."""

    def __init__(self):
        self._t = None

    def get(self, key, binding, n_f):
        tensor, ptr, version = key
        t = self._t
        if t is None or t[0] is not tensor or t[1:4] != (ptr, version, n_f):
            self._t = t = (tensor, ptr, version, n_f) + csr(binding, n_f, "binding")   # holds `tensor`: its address is not reused
        return t[4], t[5]


class _VertexTable:
    """The vertex -> corner table (corner = 3 * face + position) of the backward pass: the faces are fixed, so it is built once per
    vertex count."""

    def __init__(self):
        self._t = None

    def get(self, faces, n_v):
        if self._t is None or self._t[0] != n_v:
            self._t = (n_v,) + csr(faces, n_v, "faces")
        return self._t[1:]


class MeshFrames:
    def __init__(self, faces: torch.Tensor):
        self.faces = expect(faces.to(torch.int32).contiguous(), torch.int32, "faces", last=3)
        L.load()                                 # a missing library is reported here, not at the first launch
        self._vtable, self._gtable = _VertexTable(), _GaussianTable()
        self.verts = None
        self.face_center = self.face_orien_mat = self.face_orien_quat = self.face_scaling = None

    # mesh_gaussian_model.py:137-146
    def set_mesh_by_verts(self, verts: torch.Tensor):
        v = expect(verts, torch.float32, "verts", last=3)
        if v.device != self.faces.device:
            raise RuntimeError("verts and faces must be on the same device")
        self.verts = v
        if wants_grad(v):
            out = _FaceFrames.apply(v, self.faces, self._vtable)
        else:
            out = _launch_face_frames(self.faces, v)
        self.face_center, self.face_orien_mat, self.face_orien_quat, self.face_scaling = out

    def _bind(self, binding, xyz_local=None, rotation=None, scaling=None):
        if self.face_center is None:
            raise RuntimeError("call set_mesh_by_verts first")
        b = expect(binding.to(torch.int32).contiguous(), torch.int32, "binding")
        for t, name, w in ((xyz_local, "_xyz", 3), (rotation, "_rotation", 4), (scaling, "_scaling", 3)):
            if t is not None:
                expect(t, torch.float32, name, last=w)
        fr = (self.face_center, self.face_orien_mat, self.face_orien_quat, self.face_scaling)
        if wants_grad(xyz_local, rotation, scaling, *fr):
            out = _Bind.apply(self._gtable, binding, False, None, b, *fr, xyz_local, rotation, scaling, None, None, None, None, None)
        else:
            out = _launch_bind(False, None, b, fr, (xyz_local, rotation, scaling, None), (None,) * 4)
        return list(out[:3])

    # gaussian_model.py:141-151 / :124-138 / :112-122 (binding is not None branch)
    def get_xyz(self, binding, xyz_local):
        return self._bind(binding, xyz_local=xyz_local)[0]

    def get_rotation(self, binding, rotation):
        return self._bind(binding, rotation=rotation)[1]

    def get_scaling(self, binding, scaling):
        return self._bind(binding, scaling=scaling)[2]

    def get_all(self, binding, xyz_local, rotation, scaling):
        """All three in one launch."""
        return tuple(self._bind(binding, xyz_local, rotation, scaling))
