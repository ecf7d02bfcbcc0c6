"""The mesh tracking step on the device (preprocess/train_mesh_lbs_actorshq.py and train_mesh_lbs_4ddress.py): what one iteration of
the reference's tracking loop computes between the trained ``vertices`` and the rasteriser's argument list, and the loss terms the
appearance loop does not have (csrc/track.hip, csrc/track_math.hpp; csrc/track4d.hip, csrc/track4d_math.hpp):

    fg = FaceGaussians(faces)                                                     # once per mesh
    rendervar = fg.render_vars(vertices, log_scales, logit_opacities)             # params2rendervar :209-225, one Gaussian per face
    rendervar = fg.render_vars(..., extra_attrs=variables['cloth_mask'])          # the 4D-DRESS one, train_mesh_lbs_4ddress.py:260-277
    area, scale, opacity = fg.losses(vertices, log_scales, logit_opacities)       # losses['area'], ['scale'], ['opacity'] :242-268
    smplx_vn = VertexNormals(body_faces)(smplx_v)                                 # compute_vertex_normals, utils/geo_utils.py:8-19
    collision = collision_penalty(vertices[cloth_v_idx], smplx_v, smplx_vn)       # preprocess/losses/physics.py:6-20
    lap = MeshLaplacian(faces)                                                    # once per mesh, for laplacian_matrix of 4ddress :212-214
    laplacian = lap.loss(vertices)                                                # losses['laplacian'], train_mesh_lbs_4ddress.py:363
    ratio, edge_ratio, edge_ratio_var = fg.scale_ratio_losses(vertices, rendervar['scales'])    # scale_ratio_loss :279-292, :361

The rest of the iteration is already here: ``rasterizer.GaussianRasterizer``, ``image_loss`` and ``l1_loss``, ``MeshRegularizer``
(normal, iso, eq_faces_weight) and ``FusedAdam``.  INTEGRATION.md, "Before the solver: the tracking step", has the switch-over.

What is pinned by the reference's own code (tests/golden/track.npz): the barycentres, the frame matrices x | y | z, the face normals
and areas, the vertex normals, the penalty in its three modes and its nearest indices.  UNCONFIRMED: the matrix -> quaternion map,
which restates pytorch3d.transforms.matrix_to_quaternion (pytorch3d is not installed where the fixtures are made, and its older
releases leave the sign alone): the roots sqrt(max(0, 1 +- m00 +- m11 +- m22)), the candidate rows divided by twice the root
floored at 0.1, the row of the largest root, then the sign that makes w >= 0.  ``q`` and ``-q`` render the same image.

Rules: fp32 arithmetic, fp64 sums in a fixed order, no floating-point atomics, so the same inputs give the same bits, values and
gradients.  The backward is the exact derivative of the forward with every discrete decision held fixed (the longest edge, the
quaternion's branch and sign, sign(0) = 0, the hinge with slope exactly 1/2 where eps - d == 0); there is no double backward.  With
grad mode off, or with nothing requiring grad, the same launch gives the same bits with no ``grad_fn`` and nothing saved.  A
zero-area face gives NaN and a vertex in no face a NaN normal, as in the reference.  No CPU fallback: tensors must live on an MI355X.
"""
from __future__ import annotations

import torch

from . import _lib as L
from ._call import call, csr, expect, ptr, upstream, wants_grad

_TPB = 256        # MPMHIP_TRACK_TPB
_MODES = {"distance": 0, "average": 1, "cubed": 2}     # MPMHIP_TRACK_DISTANCE, _AVERAGE, _CUBED


class _Mesh:
    """faces [F, 3] checked once, and the vertex -> corner table (item = 3 f + c, ascending within a vertex), which needs the vertex
    count and is built at its first use"""

    def __init__(self, faces: torch.Tensor):
        if not isinstance(faces, torch.Tensor) or faces.dtype not in (torch.int32, torch.int64):
            raise RuntimeError("faces: expected an int32 or int64 tensor on the GPU")
        self.faces = expect(faces.to(torch.int32).contiguous(), torch.int32, "faces", last=3, rows=True)
        self.n_faces = self.faces.shape[0]
        if int(self.faces.min()) < 0:
            raise RuntimeError("faces: negative index")
        self.n_verts_min = int(self.faces.max()) + 1
        L.load()                                 # a missing library is reported here, not at the first launch
        self._table_key = self._table_value = None

    def _verts(self, verts, name="vertices"):
        v = expect(verts, torch.float32, name, last=3)
        if v.dim() != 2 or v.shape[0] < self.n_verts_min:
            raise RuntimeError(f"{name}: expected [V, 3] with V >= {self.n_verts_min}, got {tuple(v.shape)}")
        if v.device != self.faces.device:
            raise RuntimeError(f"{name} and faces must be on the same device")
        return v

    def _table(self, n_verts):
        if self._table_key != n_verts:
            self._table_key, self._table_value = n_verts, csr(self.faces, n_verts, "faces")
        return self._table_value


def _empty(dev, *shape):
    return torch.empty(*shape, dtype=torch.float32, device=dev)


def _launch_render(fg, v, ls, lo):
    dev, n_f = v.device, fg.n_faces
    means, rot, scales, opac = _empty(dev, n_f, 3), _empty(dev, n_f, 4), _empty(dev, n_f, 3), _empty(dev, n_f, 1)
    call("mpmhip_track_render_vars", dev, v.data_ptr(), v.shape[0], fg.faces.data_ptr(), n_f, ls.data_ptr(), lo.data_ptr(), means.data_ptr(),
         rot.data_ptr(), scales.data_ptr(), opac.data_ptr())
    return means, rot, scales, opac


def _grads(ctx, v, ls, lo):
    """(d_verts, d_log_scales, d_logit_opacities) to be written, None where not wanted, and the table and stencil d_verts needs"""
    fg = ctx.fg
    d_v, d_ls, d_lo = [torch.empty_like(t) if want else None for want, t in zip(ctx.needs_input_grad[:3], (v, ls, lo))]
    start, items, stencil = None, None, None
    if d_v is not None:
        start, items = fg._table(v.shape[0])
        stencil = _empty(v.device, fg.n_faces, 3, 3)
    return d_v, d_ls, d_lo, start, items, stencil


class _RenderVars(torch.autograd.Function):
    """(vertices, log_scales, logit_opacities) -> (means3D, rotations, scales, opacities)"""

    @staticmethod
    def forward(ctx, v, ls, lo, fg):
        out = _launch_render(fg, v, ls, lo)
        ctx.fg = fg
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(v, ls, lo)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_means, g_rot, g_scales, g_opac):
        v, ls, lo = ctx.saved_tensors
        fg = ctx.fg
        g = [upstream(t) for t in (g_means, g_rot, g_scales, g_opac)]
        if all(t is None for t in g):
            return None, None, None, None
        d_v, d_ls, d_lo, start, items, stencil = _grads(ctx, v, ls, lo)
        call("mpmhip_track_render_vars_backward", v.device, v.data_ptr(), v.shape[0], fg.faces.data_ptr(), fg.n_faces, ls.data_ptr(),
             lo.data_ptr(), *[ptr(t) for t in g], ptr(start), ptr(items), ptr(stencil), ptr(d_v), ptr(d_ls), ptr(d_lo))
        return d_v, d_ls, d_lo, None


def _launch_terms(fg, v, ls, lo):
    dev = v.device
    terms = _empty(dev, 3)
    scratch = torch.empty(3 * ((fg.n_faces + _TPB - 1) // _TPB), dtype=torch.float64, device=dev)
    call("mpmhip_track_terms_forward", dev, v.data_ptr(), v.shape[0], fg.faces.data_ptr(), fg.n_faces, ls.data_ptr(), lo.data_ptr(),
         scratch.data_ptr(), terms.data_ptr())
    return terms


class _Terms(torch.autograd.Function):
    """(vertices, log_scales, logit_opacities) -> [area, scale, opacity]"""

    @staticmethod
    def forward(ctx, v, ls, lo, fg):
        terms = _launch_terms(fg, v, ls, lo)
        ctx.fg = fg
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(v, ls, lo)
        return terms

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_terms):
        v, ls, lo = ctx.saved_tensors
        fg = ctx.fg
        g = upstream(g_terms)
        if g is None:
            return None, None, None, None
        d_v, d_ls, d_lo, start, items, stencil = _grads(ctx, v, ls, lo)
        call("mpmhip_track_terms_backward", v.device, v.data_ptr(), v.shape[0], fg.faces.data_ptr(), fg.n_faces, ls.data_ptr(), lo.data_ptr(),
             g.data_ptr(), ptr(start), ptr(items), ptr(stencil), ptr(d_v), ptr(d_ls), ptr(d_lo))
        return d_v, d_ls, d_lo, None


class FaceGaussians(_Mesh):
    """One Gaussian per face of one mesh: the four computed entries of ``params2rendervar`` and the loss terms on them.  faces [F, 3]
    (int32 or int64); vertices [V, 3] with V beyond the largest index; log_scales [F, 3]; logit_opacities [F, 1] or [F]."""

    def _inputs(self, vertices, log_scales, logit_opacities):
        v = self._verts(vertices)
        ls = expect(log_scales, torch.float32, "log_scales", shape=(self.n_faces, 3))
        lo = expect(logit_opacities, torch.float32, "logit_opacities")
        if tuple(lo.shape) not in ((self.n_faces, 1), (self.n_faces,)):
            raise RuntimeError(f"logit_opacities: expected shape {(self.n_faces, 1)}, got {tuple(lo.shape)}")
        if not (ls.device == lo.device == v.device):
            raise RuntimeError("FaceGaussians: the tensors must be on the same device")
        return v, ls, lo

    def render_vars(self, vertices, log_scales, logit_opacities, extra_attrs=None) -> dict:
        """-> {means3D [F, 3], rotations [F, 4] WXYZ, scales [F, 3], opacities [F, 1]}; ``colors_precomp`` and ``means2D`` are the
        caller's.  The quaternion conversion is UNCONFIRMED against pytorch3d (module docstring); ``q`` and ``-q`` render alike.
        ``extra_attrs`` [F, E], the 4D-DRESS script's ``variables['cloth_mask']`` (train_mesh_lbs_4ddress.py:260-277), is handed on under
        its key as it is, for the rasteriser's sixth slot; without it the dict has no such key."""
        v, ls, lo = self._inputs(vertices, log_scales, logit_opacities)
        if extra_attrs is not None and (not isinstance(extra_attrs, torch.Tensor) or extra_attrs.dim() != 2 or extra_attrs.shape[0] != self.n_faces):
            raise RuntimeError(f"extra_attrs: expected a tensor of shape ({self.n_faces}, E)")
        out = _RenderVars.apply(v, ls, lo, self) if wants_grad(v, ls, lo) else _launch_render(self, v, ls, lo)
        rendervar = dict(zip(("means3D", "rotations", "scales", "opacities"), out))
        if extra_attrs is not None:
            rendervar["extra_attrs"] = extra_attrs
        return rendervar

    def terms(self, vertices, log_scales, logit_opacities) -> torch.Tensor:
        """-> the [3] tensor (area, scale, opacity), for callers who weight with a tensor product"""
        v, ls, lo = self._inputs(vertices, log_scales, logit_opacities)
        return _Terms.apply(v, ls, lo, self) if wants_grad(v, ls, lo) else _launch_terms(self, v, ls, lo)

    def losses(self, vertices, log_scales, logit_opacities):
        """-> (area, scale, opacity): 0-dim fp32 tensors"""
        return self.terms(vertices, log_scales, logit_opacities).unbind(0)

    def scale_ratio_losses(self, vertices, scales, scale_ratio_th=5.0, scale_edge_ratio_th=1.0):
        """``scale_ratio_loss`` (below) over this mesh's cached face table -> (scale_ratio, scale_edge_ratio, scale_edge_ratio_var),
        0-dim fp32.  ``scales`` [F, 3] is the ``scales`` entry of ``render_vars``: through its graph the gradient reaches ``log_scales``."""
        v = self._verts(vertices, "verts")
        s = expect(scales, torch.float32, "scale", shape=(self.n_faces, 3))
        if s.device != v.device:
            raise RuntimeError("scale and verts must be on the same device")
        th = (float(scale_ratio_th), float(scale_edge_ratio_th))
        terms = _ScaleRatio.apply(v, s, self, th) if wants_grad(v, s) else _launch_scale_ratio(self, v, s, th)[:3]
        return terms.unbind(0)

    def _geometry(self, vertices, normals, areas):
        v = self._verts(vertices).detach()
        call("mpmhip_track_face_geometry", v.device, v.data_ptr(), v.shape[0], self.faces.data_ptr(), self.n_faces, ptr(normals), ptr(areas))

    def face_normals(self, vertices) -> torch.Tensor:
        """compute_face_normals -> [F, 3]; forward only"""
        out = _empty(self.faces.device, self.n_faces, 3)
        self._geometry(vertices, out, None)
        return out

    def face_areas(self, vertices) -> torch.Tensor:
        """compute_face_areas -> [F]; forward only"""
        out = _empty(self.faces.device, self.n_faces)
        self._geometry(vertices, None, out)
        return out


class VertexNormals(_Mesh):
    """compute_vertex_normals for one mesh: the unnormalised ``cross(v0 - v1, v2 - v1)`` of every incident face, summed per vertex in
    ascending face order (a gather, not an ``index_add_``: the same bits on every run) and normalised.  Forward only -- the body's
    normals take no gradient in the tracking loop (``collision_penalty``).  A vertex in no face gives NaN, as in the reference."""

    def __call__(self, verts: torch.Tensor) -> torch.Tensor:
        v = self._verts(verts, "verts").detach()
        start, items = self._table(v.shape[0])
        out = torch.empty_like(v)
        call("mpmhip_track_vertex_normals", v.device, v.data_ptr(), v.shape[0], self.faces.data_ptr(), self.n_faces, start.data_ptr(),
             items.data_ptr(), out.data_ptr())
        return out


def vertex_normals(verts: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
    """``compute_vertex_normals(vertices, faces)``; builds the vertex -> face table on every call (``VertexNormals`` keeps it)"""
    return VertexNormals(faces)(verts)


def _launch_collision(va, vb, nb, eps, mode):
    """-> (index int32 [n], distance [n] or None, value [1] or None)"""
    dev, n = va.device, va.shape[0]
    index = torch.empty(n, dtype=torch.int32, device=dev)
    dist = None if nb is None else _empty(dev, n)
    reduce = nb is not None and mode != _MODES["distance"]
    value = _empty(dev, 1) if reduce else None
    if n > 0:
        best = torch.empty(n, dtype=torch.int64, device=dev)
        scratch = torch.empty((n + _TPB - 1) // _TPB, dtype=torch.float64, device=dev) if reduce else None
        call("mpmhip_track_collision_forward", dev, va.data_ptr(), n, vb.data_ptr(), ptr(nb), vb.shape[0], eps, mode, best.data_ptr(),
             ptr(scratch), index.data_ptr(), ptr(dist), ptr(value))
    elif reduce:                                 # the reference's 0 / 0 and its empty sum
        value.fill_(float("nan") if mode == _MODES["average"] else 0.0)
    return index, dist, value


class _Collision(torch.autograd.Function):
    """va -> the distances or the penalty; the body is constant"""

    @staticmethod
    def forward(ctx, va, vb, nb, eps, mode):
        index, dist, value = _launch_collision(va, vb, nb, eps, mode)
        ctx.eps, ctx.mode = eps, mode
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(nb, index, dist)
        ctx.mark_non_differentiable(index)
        return (dist if value is None else value.reshape(())), index

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out, _g_index):
        nb, index, dist = ctx.saved_tensors
        n = index.shape[0]
        g = upstream(g_out, (n,) if ctx.mode == _MODES["distance"] else None)
        if g is None:
            return None, None, None, None, None
        d_va = _empty(nb.device, n, 3)
        if n > 0:
            call("mpmhip_track_collision_backward", nb.device, n, nb.data_ptr(), nb.shape[0], index.data_ptr(), dist.data_ptr(), ctx.eps,
                 ctx.mode, g.data_ptr(), d_va.data_ptr())
        return d_va, None, None, None, None


def _points(va, vb, nb=None):
    a = expect(va, torch.float32, "va", last=3)
    if a.dim() != 2:
        raise RuntimeError("va: expected an [n, 3] tensor")
    b = expect(vb, torch.float32, "vb", last=3, rows=True)
    if nb is not None:
        nb = expect(nb, torch.float32, "nb", shape=tuple(b.shape))
    for name, t in (("vb", b), ("nb", nb)):
        if t is not None and (t.device != a.device):
            raise RuntimeError(f"va and {name} must be on the same device")
        if t is not None and t.requires_grad and torch.is_grad_enabled():
            raise RuntimeError(f"{name} requires grad: the body takes no gradient here (the reference runs with --lr_smplx 0.0); "
                               f"pass {name}.detach()")
    L.load()
    return a, b, nb


def collision_penalty(va, vb, nb, eps=1e-3, return_average=True, return_distance=False):
    """``collision_penalty`` of preprocess/losses/physics.py: va [n, 3] the cloth vertices, vb [m, 3] and nb [m, 3] the body's vertices
    and vertex normals.  With j the nearest body vertex of va[i] and d_i = -nb[j] . (va[i] - vb[j]):

        return_distance                  -> the [n] signed distances d
        return_average (the default)     -> sum(max(eps - d, 0)) / n
        neither                          -> sum(max(eps - d, 0) ** 3)

    The nearest vertex is found without the [n, m] distance matrix, by the kernel of ``geo_metrics``' nearest-neighbour search: the
    lowest index of the exact minimum of the direct-form squared distance |a - b|^2.  The reference takes the argmin of the expanded
    form |a|^2 + |b|^2 - 2 a.b; where the two decide a near-tie differently, the expanded form is the less accurate of the two.
    The gradient goes to ``va`` alone: ``slope * nb[j] / n`` (slope 1 where eps - d > 0, 0 where < 0, exactly 1/2 where equal, as
    ``torch.maximum``), ``3 pen^2 nb[j]`` in the cubed mode, ``-g_i nb[j]`` in the distance mode.  A ``vb`` or ``nb`` that requires
    grad raises: pass ``.detach()``."""
    a, b, nrm = _points(va, vb, nb)
    mode = _MODES["distance"] if return_distance else _MODES["average"] if return_average else _MODES["cubed"]
    if wants_grad(a):
        return _Collision.apply(a, b, nrm, float(eps), mode)[0]
    _, dist, value = _launch_collision(a, b, nrm, float(eps), mode)
    return dist if value is None else value.reshape(())


def nearest_neighbour(A, B) -> torch.Tensor:
    """``NearestNeighbour()(A, B)`` of preprocess/losses/layers.py: the int32 [n] index of the nearest row of B [m, 3] for every row of
    A [n, 3] (the lowest index on an exact tie)."""
    a, b, _ = _points(A.detach() if isinstance(A, torch.Tensor) else A, B.detach() if isinstance(B, torch.Tensor) else B)
    return _launch_collision(a, b, None, 0.0, _MODES["distance"])[0]


# ---- the 4D-DRESS script's two further terms (train_mesh_lbs_4ddress.py:279-292, :361, :363; csrc/track4d.hip) -------------------------

def _launch_laplacian(lap, v, want_lv, want_value):
    """-> (Lv [V, 3] or None, value [1] or None)"""
    dev, n_v = v.device, v.shape[0]
    start, nbr = lap._adjacency(n_v)
    lv = _empty(dev, n_v, 3) if want_lv else None
    value = _empty(dev, 1) if want_value else None
    n_scratch = (n_v + _TPB - 1) // _TPB
    scratch = torch.empty(n_scratch, dtype=torch.float64, device=dev) if want_value else None
    call("mpmhip_track4d_laplacian_forward", dev, v.data_ptr(), n_v, start.data_ptr(), nbr.data_ptr(), nbr.shape[0], ptr(scratch), n_scratch,
         ptr(lv), ptr(value))
    return lv, value


class _Laplacian(torch.autograd.Function):
    """vertices -> mean_i |(Lv)_i|; the backward reads the saved Lv and the table, not the vertices"""

    @staticmethod
    def forward(ctx, v, lap):
        lv, value = _launch_laplacian(lap, v, True, True)
        ctx.lap = lap
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(lv)
        return value.reshape(())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_value):
        lv, = ctx.saved_tensors
        g = upstream(g_value, (1,))
        if g is None:
            return None, None
        n_v = lv.shape[0]
        start, nbr = ctx.lap._adjacency(n_v)
        d_v = torch.empty_like(lv)
        call("mpmhip_track4d_laplacian_backward", lv.device, lv.data_ptr(), n_v, start.data_ptr(), nbr.data_ptr(), nbr.shape[0], g.data_ptr(),
             d_v.data_ptr())
        return d_v, None


class MeshLaplacian(_Mesh):
    """``losses['laplacian']`` of train_mesh_lbs_4ddress.py:363 without the dense [V, V] ``laplacian_matrix`` of :212-214: the uniform
    Laplacian as a gather over the vertex adjacency.  With E the undirected edges of ``faces`` (each once, however many faces share
    it), N(i) the neighbours of i and deg(i) their number:

        (Lv)_i = (sum_{j in N(i)} v_j) / deg(i) - v_i        -v_i for a vertex in no face
        loss   = mean_i |(Lv)_i|                             over all V rows of ``vertices``

    The sum runs in ascending j and is divided by the degree, so neighbours that sum to exactly deg * v_i give exactly zero;
    pytorch3d stores 1 / deg in the matrix, a difference at rounding level.  Where |(Lv)_i| is zero the gradient through it is zero,
    as torch's ``norm``.  UNCONFIRMED against pytorch3d's ``laplacian_packed`` itself (not installed where the fixtures are made).
    A face that names one vertex twice raises: pytorch3d would put a self-edge into the matrix.  The adjacency (CSR, ascending within
    a row) is built with torch ops once per vertex count, at first use."""

    def __init__(self, faces: torch.Tensor):
        super().__init__(faces)
        f = self.faces
        if bool(((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 2] == f[:, 0])).any()):
            raise RuntimeError("faces: a face names one vertex twice")
        self._adj_key = self._adj_value = None

    def _adjacency(self, n_verts):
        if self._adj_key != n_verts:
            f = self.faces.long()
            e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
            e = torch.cat([e, e.flip(1)])                                        # both directions
            key = torch.unique(e[:, 0] * n_verts + e[:, 1])                      # sorted: by row, ascending within it; an edge counts once
            row = torch.div(key, n_verts, rounding_mode="floor")
            start = torch.zeros(n_verts + 1, dtype=torch.int32, device=f.device)
            start[1:] = torch.cumsum(torch.bincount(row, minlength=n_verts), 0)
            self._adj_key, self._adj_value = n_verts, (start, (key - row * n_verts).to(torch.int32))
        return self._adj_value

    def loss(self, vertices) -> torch.Tensor:
        """-> the 0-dim fp32 ``variables['laplacian_matrix'].mm(vertices).norm(dim=1).mean()``, with gradient to ``vertices``"""
        v = self._verts(vertices)
        return _Laplacian.apply(v, self) if wants_grad(v) else _launch_laplacian(self, v, False, True)[1].reshape(())

    def apply(self, vertices) -> torch.Tensor:
        """-> Lv [V, 3]; forward only"""
        return _launch_laplacian(self, self._verts(vertices).detach(), True, False)[0]


def _launch_scale_ratio(fg, v, s, th):
    dev = v.device
    terms = _empty(dev, 4)
    n_scratch = 4 * ((fg.n_faces + _TPB - 1) // _TPB)
    scratch = torch.empty(n_scratch, dtype=torch.float64, device=dev)
    call("mpmhip_track4d_scale_ratio_forward", dev, v.data_ptr(), v.shape[0], fg.faces.data_ptr(), fg.n_faces, s.data_ptr(), th[0], th[1],
         scratch.data_ptr(), n_scratch, terms.data_ptr())
    return terms


class _ScaleRatio(torch.autograd.Function):
    """(vertices, scales) -> [scale_ratio, scale_edge_ratio, scale_edge_ratio_var]"""

    @staticmethod
    def forward(ctx, v, s, fg, th):
        terms = _launch_scale_ratio(fg, v, s, th)
        ctx.fg, ctx.th = fg, th
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(v, s, terms)
        return terms[:3].clone()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_terms):
        v, s, terms = ctx.saved_tensors
        fg = ctx.fg
        g = upstream(g_terms)
        if g is None:
            return None, None, None, None
        d_v, d_s = [torch.empty_like(t) if want else None for want, t in zip(ctx.needs_input_grad[:2], (v, s))]
        start, items, stencil = None, None, None
        if d_v is not None:
            start, items = fg._table(v.shape[0])
            stencil = _empty(v.device, fg.n_faces, 3, 3)
        call("mpmhip_track4d_scale_ratio_backward", v.device, v.data_ptr(), v.shape[0], fg.faces.data_ptr(), fg.n_faces, s.data_ptr(),
             ctx.th[0], ctx.th[1], terms.data_ptr(), g.data_ptr(), ptr(start), ptr(items), ptr(stencil), ptr(d_v), ptr(d_s))
        return d_v, d_s, None, None


def scale_ratio_loss(verts, faces, scale, scale_ratio_th=5.0, scale_edge_ratio_th=1.0):
    """``scale_ratio_loss`` of train_mesh_lbs_4ddress.py:279-292 (name, argument order and defaults): per face, with m the longest
    edge, a = max(s0, s1), b = min(s0, s1), r = a / (b + 1e-8), q = a / (m + 1e-8),

        scale_ratio = mean(max(r, th_r) - th_r)    scale_edge_ratio = mean(max(q, th_e) - th_e)    scale_edge_ratio_var = var(q)

    (unbiased; NaN for a single face, as in the reference).  Gradients go to ``verts`` through m and to ``scale[:, :2]`` (column 2
    gets exact zeros); the decisions are held fixed as torch takes them on the CPU: the first of equal maxima and minima, clamp's
    slope 1 at x == th, no gradient through a longest edge of length zero.  Checks ``faces`` and builds the vertex -> corner table on
    every call; ``FaceGaussians.scale_ratio_losses`` keeps both."""
    return FaceGaussians(faces).scale_ratio_losses(verts, scale, scale_ratio_th, scale_edge_ratio_th)
