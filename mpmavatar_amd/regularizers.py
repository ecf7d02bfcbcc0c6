"""The regularisation terms of the appearance loop on the device (train_appearance.py:136-150): what the reference computes on
every iteration between ``render(...)`` and ``loss.backward()`` besides the image loss,

    reg_losses["normal"]          = gaussians.normal_loss()        # scene/mesh_gaussian_model.py:203-220
    reg_losses["opacity"]         = gaussians.opacity_loss()       # :222-223
    reg_losses["iso"]             = gaussians.iso_loss()           # :225-231
    reg_losses["eq_faces_weight"] = gaussians.area_loss()          # :233-246
    reg_losses["xyz"]   = F.relu(gaussians._xyz[visibility_filter].norm(dim=1) - opt.threshold_xyz).mean()
    reg_losses["scale"] = F.relu(torch.exp(gaussians._scaling[visibility_filter]) - opt.threshold_scale).norm(dim=1).mean()

as two fused ops (csrc/reg.hip) with exact backward passes:

    reg = MeshRegularizer(faces, gaussians.verts_orig[0])                    # once per mesh
    normal, iso, eq_faces = reg(verts)                                       # per iteration: 0-dim fp32 tensors
    opacity, xyz, scale = gaussian_regularizers(_opacity, _xyz, _scaling, radii, opt.threshold_xyz, opt.threshold_scale)

The backward is the exact derivative with every discrete decision held fixed (sign(0) = 0 inside an absolute value, a relu that binds
and the norm of an all-zero row have zero slope), fp32, no atomics: the same input gives the same bits.  There is no double backward.
With grad mode off, or with nothing requiring grad, the same launch gives the same bits with no ``grad_fn`` and nothing saved.  A
zero-area face gives NaN in ``normal`` and no visible Gaussian gives NaN in ``xyz`` and ``scale``, as in the reference.  No CPU
fallback: tensors must live on an MI355X.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from ._call import call, csr, expect, ptr, upstream, wants_grad

K = 3             # MPMHIP_REG_K
_TPB = 256        # MPMHIP_REG_TPB


def adjacent_faces(faces, k=3):
    """faces [F, 3] (array or tensor) -> the [F, k] int64 array of utils/general_utils.py:286-316, row for row, order included: a
    face's neighbours across its edges, edges in the order in which a walk over (face, corner) first meets them and the faces of an
    edge in ascending (face, corner); a row longer than k is cut from the end, a shorter one is filled with the face's own index.
    Host, once per mesh.  (A face that repeats a vertex is outside what this reproduces.)"""
    f = np.asarray(faces.detach().cpu() if isinstance(faces, torch.Tensor) else faces).astype(np.int64).reshape(-1, 3)
    n_f = f.shape[0]
    out = np.repeat(np.arange(n_f, dtype=np.int64)[:, None], k, 1)
    if n_f == 0:
        return out
    a, b = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)                        # incidence e = 3 * face + corner
    key = np.minimum(a, b) * (int(f.max()) + 1) + np.maximum(a, b)
    _, first, inv = np.unique(key, return_index=True, return_inverse=True)
    rank = np.empty(first.shape[0], np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(first.shape[0])       # an edge's place in first-seen order
    erank = rank[inv.reshape(-1)]
    order = np.argsort(erank, kind="stable")                                 # incidences grouped by edge, ascending e within one
    count = np.bincount(erank)
    start = np.concatenate([[0], np.cumsum(count)])[:-1]
    g_edge = erank[order]
    pos = np.arange(order.shape[0]) - start[g_edge]                          # an incidence's place within its edge
    rows, others, keys = [], [], []
    for d in range(int(count.max())):                                        # the d-th face of the edge, for every other incidence
        sel = (count[g_edge] > d) & (pos != d)
        rows.append(order[sel] // 3)
        others.append(order[start[g_edge[sel]] + d] // 3)
        keys.append(g_edge[sel] * int(count.max()) + d)
    rows, others, keys = np.concatenate(rows), np.concatenate(others), np.concatenate(keys)
    by = np.lexsort((keys, rows))                                            # per face: by edge, then by place within the edge
    rows, others = rows[by], others[by]
    slot = np.arange(rows.shape[0]) - np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n_f))])[rows]
    keep = slot < k
    out[rows[keep], slot[keep]] = others[keep]
    return out


def _vis_ptrs(vis):
    return (None, vis.data_ptr()) if vis.dtype == torch.bool else (vis.data_ptr(), None)


def _launch_mesh(reg, verts, sq_dist=None):
    dev = verts.device
    terms, stats = torch.empty(3, dtype=torch.float32, device=dev), torch.empty(2, dtype=torch.float32, device=dev)
    scratch = torch.empty(3 * ((reg.n_faces + _TPB - 1) // _TPB) + (reg.n_faces + 1) // 2, dtype=torch.float64, device=dev)
    call("mpmhip_mesh_reg_forward", dev, verts.data_ptr(), reg.n_verts, reg.faces.data_ptr(), reg.n_faces, reg.face_neighbors.data_ptr(),
         reg.neighbor_dist.data_ptr(), reg.neighbor_weight.data_ptr(), scratch.data_ptr(), terms.data_ptr(), stats.data_ptr(), ptr(sq_dist))
    return terms, stats


class _MeshReg(torch.autograd.Function):
    """verts -> [normal, iso, area]: the forward launches with a backward"""

    @staticmethod
    def forward(ctx, verts, reg):
        terms, stats = _launch_mesh(reg, verts)
        ctx.reg = reg
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(verts, stats)
        return terms

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_terms):
        verts, stats = ctx.saved_tensors
        g = upstream(g_terms)
        if g is None:
            return None, None
        reg, dev = ctx.reg, verts.device
        start, items = reg._vertex_table()
        d_stencil = torch.empty(reg.n_faces, 1 + K, 3, 3, dtype=torch.float32, device=dev)
        d_verts = torch.empty_like(verts)
        call("mpmhip_mesh_reg_backward", dev, verts.data_ptr(), reg.n_verts, reg.faces.data_ptr(), reg.n_faces, reg.face_neighbors.data_ptr(),
             reg.neighbor_dist.data_ptr(), reg.neighbor_weight.data_ptr(), stats.data_ptr(), g.data_ptr(), start.data_ptr(), items.data_ptr(),
             d_stencil.data_ptr(), d_verts.data_ptr())
        return d_verts, None


class MeshRegularizer:
    """The three mesh terms for one mesh.  faces [F, 3]; verts0 [V, 3] = ``gaussians.verts_orig[0]``, from which ``neighbor_dist`` and
    ``neighbor_weight`` are taken exactly as scene/mesh_gaussian_model.py:91-98, on the device; face_neighbors: the reference's [F, 3]
    array if the caller has it, else ``adjacent_faces(faces)``.  The vertex -> stencil table of the backward pass is built at the
    first backward."""

    def __init__(self, faces: torch.Tensor, verts0: torch.Tensor, face_neighbors=None):
        self.faces = expect(faces.to(torch.int32).contiguous(), torch.int32, "faces", last=3, rows=True)
        v0 = expect(verts0, torch.float32, "verts0", last=3, rows=True)
        dev = self.faces.device
        if v0.device != dev:
            raise RuntimeError("verts0 and faces must be on the same device")
        self.n_faces, self.n_verts = self.faces.shape[0], v0.shape[0]
        if self.n_faces * 12 * 3 > 2 ** 31 - 1:
            raise RuntimeError(f"MeshRegularizer: {self.n_faces} faces are more than the stencil table can index")
        if int(self.faces.min()) < 0 or int(self.faces.max()) >= self.n_verts:
            raise RuntimeError(f"faces: index out of range [0, {self.n_verts})")
        if face_neighbors is None:
            face_neighbors = torch.from_numpy(adjacent_faces(self.faces, K))
        nb = torch.as_tensor(face_neighbors).to(device=dev, dtype=torch.int32).contiguous()
        if tuple(nb.shape) != (self.n_faces, K):
            raise RuntimeError(f"face_neighbors: expected shape {(self.n_faces, K)}, got {tuple(nb.shape)}")
        if int(nb.min()) < 0 or int(nb.max()) >= self.n_faces:
            raise RuntimeError(f"face_neighbors: index out of range [0, {self.n_faces})")
        L.load()                                 # a missing library is reported here, not at the first launch
        self.face_neighbors = nb
        # the set-up: one forward launch on verts0 that stores the squared centre distances (the two inputs play no part in them)
        self.neighbor_dist = self.neighbor_weight = torch.zeros(self.n_faces, K, dtype=torch.float32, device=dev)
        sq = torch.empty(self.n_faces, K, dtype=torch.float32, device=dev)
        _launch_mesh(self, v0.detach(), sq)
        self.neighbor_weight = torch.exp(-2000 * sq)
        self.neighbor_dist = torch.sqrt(sq)
        self._table = None

    def _vertex_table(self):
        if self._table is None:
            nbx = torch.cat([torch.arange(self.n_faces, dtype=torch.int32, device=self.faces.device)[:, None], self.face_neighbors], 1)
            self._table = csr(self.faces[nbx.long()], self.n_verts, "faces")       # S[f, s, c], item = 12 f + 3 s + c
        return self._table

    def terms(self, verts: torch.Tensor) -> torch.Tensor:
        """-> the [3] tensor (normal, iso, eq_faces_weight), for callers who weight with a tensor product"""
        v = expect(verts, torch.float32, "verts", shape=(self.n_verts, 3))
        if v.device != self.faces.device:
            raise RuntimeError("verts and faces must be on the same device")
        if wants_grad(v):
            return _MeshReg.apply(v, self)
        return _launch_mesh(self, v)[0]

    def __call__(self, verts: torch.Tensor):
        return self.terms(verts).unbind(0)


def _launch_gauss(opacity, xyz, scaling, vis, t_xyz, t_scale):
    dev, n = xyz.device, xyz.shape[0]
    terms = torch.empty(3, dtype=torch.float32, device=dev)
    n_visible = torch.zeros(1, dtype=torch.int32, device=dev)
    if n == 0:                                   # the means of empty tensors
        return terms.fill_(float("nan")), n_visible
    scratch = torch.empty(4 * ((n + _TPB - 1) // _TPB), dtype=torch.float64, device=dev)
    call("mpmhip_gauss_reg_forward", dev, n, opacity.data_ptr(), xyz.data_ptr(), scaling.data_ptr(), *_vis_ptrs(vis), t_xyz, t_scale,
         scratch.data_ptr(), terms.data_ptr(), n_visible.data_ptr())
    return terms, n_visible


class _GaussReg(torch.autograd.Function):
    """(_opacity, _xyz, _scaling) -> [opacity, xyz, scale]: the forward launches with a backward"""

    @staticmethod
    def forward(ctx, opacity, xyz, scaling, vis, t_xyz, t_scale):
        terms, n_visible = _launch_gauss(opacity, xyz, scaling, vis, t_xyz, t_scale)
        ctx.thresholds = (t_xyz, t_scale)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(opacity, xyz, scaling, vis, n_visible)
        return terms

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_terms):
        opacity, xyz, scaling, vis, n_visible = ctx.saved_tensors
        g = upstream(g_terms)
        if g is None:
            return (None,) * 6
        d_opa, d_xyz, d_scl = [torch.empty_like(t) if want else None for want, t in zip(ctx.needs_input_grad[:3], (opacity, xyz, scaling))]
        n = xyz.shape[0]
        if n > 0:
            call("mpmhip_gauss_reg_backward", xyz.device, n, opacity.data_ptr(), xyz.data_ptr(), scaling.data_ptr(), *_vis_ptrs(vis),
                 *ctx.thresholds, n_visible.data_ptr(), g.data_ptr(), ptr(d_opa), ptr(d_xyz), ptr(d_scl))
        return d_opa, d_xyz, d_scl, None, None, None


def gaussian_terms(_opacity, _xyz, _scaling, radii, threshold_xyz, threshold_scale) -> torch.Tensor:
    """-> the [3] tensor (opacity, xyz, scale).  _opacity [n, 1] or [n], _xyz [n, 3], _scaling [n, 3]: the model's raw parameters;
    radii: the rasteriser's int32 [n] (visible = radii > 0) or a bool [n]."""
    xyz = expect(_xyz, torch.float32, "_xyz", last=3)
    n = xyz.shape[0]
    if xyz.dim() != 2:
        raise RuntimeError("_xyz: expected an [n, 3] tensor")
    scaling = expect(_scaling, torch.float32, "_scaling", shape=(n, 3))
    opacity = expect(_opacity, torch.float32, "_opacity")
    if tuple(opacity.shape) not in ((n, 1), (n,)):
        raise RuntimeError(f"_opacity: expected shape {(n, 1)}, got {tuple(opacity.shape)}")
    if not (isinstance(radii, torch.Tensor) and radii.dtype in (torch.int32, torch.bool)):
        raise RuntimeError("radii: expected an int32 or bool tensor on the GPU")
    vis = expect(radii, radii.dtype, "radii", shape=(n,))
    if not (xyz.device == scaling.device == opacity.device == vis.device):
        raise RuntimeError("gaussian_regularizers: the tensors must be on the same device")
    L.load()
    t_xyz, t_scale = float(threshold_xyz), float(threshold_scale)
    if wants_grad(opacity, xyz, scaling):
        return _GaussReg.apply(opacity, xyz, scaling, vis, t_xyz, t_scale)
    return _launch_gauss(opacity, xyz, scaling, vis, t_xyz, t_scale)[0]


def gaussian_regularizers(_opacity, _xyz, _scaling, radii, threshold_xyz, threshold_scale):
    """-> (opacity, xyz, scale): 0-dim fp32 tensors with a graph back to the three parameters"""
    return gaussian_terms(_opacity, _xyz, _scaling, radii, threshold_xyz, threshold_scale).unbind(0)
