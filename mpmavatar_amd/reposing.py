"""Re-posing on the device: the k-nearest search and the linear-blend skinning that the reference's drivers do with ``SmplxDeformer``
(utils/smplx_deformer.py:164-337), pytorch3d's ``knn_points`` and open3d's KD-tree (csrc/repose.hip, csrc/knn_device.hpp,
csrc/repose_math.hpp):

    rp = Reposer(smplx_model.lbs_weights)                                         # [V, J], once
    t_v, _, lbs_w = rp.transform_to_t_pose(verts[None], smplx_out, trans, scale, lbs_w=lbs_w[None])       # train_material_params.py:335
    posed, _ = rp.transform_to_pose(t_v[0], lbs_w, test_smplx_out, test_trans, test_scale, with_T=False)  # :343, no repeat
    t_h, _, w = rp.transform_to_t_pose(human_v, smplx0, trans0, scale0)           # train_mesh_lbs_actorshq.py:511, 6-D k-NN, k = 10
    sq_dist, _ = knn_self(init_bary, 4)                                           # o3d_knn(init_bary, 4), :126
    nn = knn_points(a[None], b[None], K=1)                                        # lbs_weights_inpainting_*.py:60

``smplx_output`` is any object with ``.transform_mat [B, J, 4, 4]`` and ``.vertices [B, V, 3]``: what ``smplx_forward`` returns.  The
SMPL-X forward itself is not here.

k nearest neighbours: exact and brute force, fp32, D = 3 or 6, 1 <= K <= 16.  The distance is the direct form
``sum_d (q_d - t_d)^2``, accumulated in ascending d; results are ordered ascending by (distance, index), so equal distances go to the
lower index, whatever the number of slices the targets were cut into.  Non-finite input gives unspecified values but indices in range.
UNCONFIRMED (``simple_knn`` is not in the reference tree; from memory): ``distCUDA2(x)`` of scene/gaussian_model.py:190 is
``knn_self(x, 3)[0].mean(-1)``.

Skinning: ``T = sum_j W[p, j] A[b, j]`` with all 16 entries, in ascending j.  On the way to the T-pose ``T`` is inverted as a general
4 x 4 matrix (its last row is (0, 0, 0, sum_j w_j), and the reference's normalisation of ``lbs_w`` is commented out).  A singular ``T``
gives non-finite output; there is no synchronisation to raise on.  ``W`` may be ``[1, P, J]`` for any number of frames, and
``vertices`` ``[1, P, 3]`` or ``[P, 3]``: neither is repeated in memory.  The reference's ``pose_offsets_pnts`` is never used and not
computed.  One difference in shape rules: the reference's ``transform_to_t_pose`` divides ``[B, P, 3]`` by ``scale.unsqueeze(1)``,
which broadcasts a ``[B]`` scale only for B == 1 (or B == P); here a ``[B]`` scale is one factor per frame.

Nothing here is differentiable: the reference runs these under ``no_grad`` or at set-up.  Inputs are detached and outputs never carry a
graph.  Input errors are ``ValueError`` before any launch.  fp32, no atomics: the same inputs give the same bits.  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import torch

from . import _lib as L
from ._call import call, ptr

MAX_K = 16
MAX_JOINTS = 127      # MPMHIP_SKIN_MAX_JOINTS


class KNN(NamedTuple):
    """what pytorch3d's ``knn_points`` returns, as far as the reference reads it"""
    dists: torch.Tensor
    idx: torch.Tensor


def _f32(t, name, *, dim=None, last=None):
    """``t`` detached and contiguous if it is a float32 tensor on the GPU of the given rank and last dimension, else ValueError"""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda:
        raise ValueError(f"{name}: expected a float32 tensor on the GPU")
    if dim is not None and t.dim() not in (dim if isinstance(dim, tuple) else (dim,)):
        raise ValueError(f"{name}: expected {dim} dimensions, got shape {tuple(t.shape)}")
    if last is not None and (t.dim() < 1 or t.shape[-1] not in (last if isinstance(last, tuple) else (last,))):
        raise ValueError(f"{name}: last dimension must be {last}, got shape {tuple(t.shape)}")
    return t.detach().contiguous()


def _same_device(*named):
    dev = named[0][1].device
    for name, t in named[1:]:
        if t is not None and t.device != dev:
            raise ValueError(f"{named[0][0]} and {name} must be on the same device")


def _check_k(k, m, what="K"):
    if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= MAX_K:
        raise ValueError(f"{what}: expected an integer in [1, {MAX_K}], got {k!r}")
    if k > m:
        raise ValueError(f"{what} = {k} exceeds the number of targets {m}")


def _knn(q, t, k, slices=0):
    """q [N, D], t [M, D] checked -> (dists [N, k] fp32, idx [N, k] int32); one launch pair, nothing for N == 0"""
    n, d = q.shape
    m = t.shape[0]
    dists = torch.empty(n, k, dtype=torch.float32, device=q.device)
    idx = torch.empty(n, k, dtype=torch.int32, device=q.device)
    if n == 0:
        return dists, idx
    need = C.c_int64(0)
    rc = L.load().mpmhip_knn_scratch(n, m, d, k, slices, C.byref(need))
    if rc != L.OK:
        raise L.MPMHipError(rc, "mpmhip_knn_scratch failed")
    scratch = torch.empty(need.value, dtype=torch.int64, device=q.device)
    call("mpmhip_knn", q.device, q.data_ptr(), n, t.data_ptr(), m, d, k, slices, scratch.data_ptr(), need.value, dists.data_ptr(), idx.data_ptr())
    return dists, idx


def knn_points(p1: torch.Tensor, p2: torch.Tensor, K: int = 1, *, slices: int = 0) -> KNN:
    """pytorch3d's ``knn_points(p1, p2, K=K)`` as the reference uses it (utils/smplx_deformer.py:184-185): p1 [B, N, D], p2 [B, M, D]
    with D 3 or 6 -> ``.dists`` [B, N, K] squared distances ascending, ``.idx`` [B, N, K] int64.  One launch pair per batch entry.
    ``slices`` (0: chosen by the library) cuts the targets for the search; the result does not depend on it."""
    a = _f32(p1, "p1", dim=3, last=(3, 6))
    b = _f32(p2, "p2", dim=3, last=(3, 6))
    _same_device(("p1", a), ("p2", b))
    if a.shape[0] != b.shape[0] or a.shape[2] != b.shape[2]:
        raise ValueError(f"p1 {tuple(a.shape)} and p2 {tuple(b.shape)}: batch size and point dimension must agree")
    if b.shape[1] == 0:
        raise ValueError("p2: no targets")
    _check_k(K, b.shape[1])
    if not isinstance(slices, int) or slices < 0:
        raise ValueError("slices: expected a non-negative integer")
    L.load()
    out = [_knn(a[i], b[i], K, slices) for i in range(a.shape[0])]
    if not out:
        return KNN(a.new_empty(0, a.shape[1], K), torch.empty(0, a.shape[1], K, dtype=torch.int64, device=a.device))
    return KNN(torch.stack([d for d, _ in out]), torch.stack([i for _, i in out]).to(torch.int64))


def knn_self(pts: torch.Tensor, k: int):
    """``o3d_knn(pts, k)`` of preprocess/helpers.py:84-94 on a device tensor: the k + 1 nearest of pts [N, 3] to the set itself with the
    first (the point, or its lowest-indexed duplicate) dropped -> (sq_dists [N, k] fp32, idx [N, k] int64).  k + 1 <= min(N, 16)."""
    p = _f32(pts, "pts", dim=2, last=(3, 6))
    if not isinstance(k, int) or isinstance(k, bool) or k < 1:
        raise ValueError(f"k: expected a positive integer, got {k!r}")
    _check_k(k + 1, p.shape[0], "k + 1")
    L.load()
    d, i = _knn(p, p, k + 1)
    return d[:, 1:].contiguous(), i[:, 1:].to(torch.int64)


def _shepard(dists, idx, power, lbs):
    """dists [N, k], idx int32 [N, k] -> W [N, J] (lbs [V, J]) or the weights [N, k] (lbs None), one launch"""
    n, k = dists.shape
    cols = k if lbs is None else lbs.shape[1]
    out = torch.empty(n, cols, dtype=torch.float32, device=dists.device)
    if n > 0:
        call("mpmhip_shepard_weights", dists.device, dists.data_ptr(), ptr(idx), n, k, power, ptr(lbs), 0 if lbs is None else lbs.shape[0],
             cols, out.data_ptr())
    return out


class Reposer:
    """Stands where the reference uses ``SmplxDeformer`` for re-posing.  ``lbs_weights`` [V, J]: the body model's skinning weights."""

    def __init__(self, lbs_weights: torch.Tensor):
        self.lbs_weights = _f32(lbs_weights, "lbs_weights", dim=2)
        v, j = self.lbs_weights.shape
        if v == 0 or not 1 <= j <= MAX_JOINTS:
            raise ValueError(f"lbs_weights: expected [V, J] with V >= 1 and 1 <= J <= {MAX_JOINTS}, got {tuple(self.lbs_weights.shape)}")
        self.device = self.lbs_weights.device
        L.load()                                 # a missing library is reported here, not at the first launch

    # ---- the k-nearest half ----------------------------------------------------------------------------------------------------------

    def _search(self, points, verts, k, points_normals, verts_normals, normal_weight):
        """-> per batch entry (dists [N, k] fp32, idx int32 [N, k]) of the 3-D points, or of (x, normal_weight * n) when a normal is given"""
        a = _f32(points, "points", dim=3, last=3)
        b = _f32(verts, "verts", dim=3, last=3)
        _same_device(("points", a), ("verts", b))
        if a.shape[0] != b.shape[0]:
            raise ValueError(f"points {tuple(a.shape)} and verts {tuple(b.shape)}: batch sizes must agree")
        if b.shape[1] == 0:
            raise ValueError("verts: no targets")
        _check_k(k, b.shape[1], "k")
        if points_normals is not None or verts_normals is not None:
            pn = torch.zeros_like(a) if points_normals is None else _f32(points_normals, "points_normals", dim=3, last=3)
            vn = torch.zeros_like(b) if verts_normals is None else _f32(verts_normals, "verts_normals", dim=3, last=3)
            if pn.shape != a.shape or vn.shape != b.shape:
                raise ValueError("normals: expected the shapes of points and verts")
            _same_device(("points", a), ("points_normals", pn), ("verts_normals", vn))
            a = torch.cat([a, float(normal_weight) * pn], dim=-1)               # exactly the reference's six coordinates (:182-183)
            b = torch.cat([b, float(normal_weight) * vn], dim=-1)
        return [_knn(a[i], b[i], k) for i in range(a.shape[0])]

    def find_k_closest_verts(self, points, verts, k, points_normals=None, verts_normals=None, normal_weight=0.1):
        """:164-185 -> (dists [bs, n, k] squared distances, idxs [bs, n, k] int64).  Without normals the reference's three zero
        coordinates add exact zeros, so the 3-D search gives the same bits."""
        out = self._search(points, verts, k, points_normals, verts_normals, normal_weight)
        return torch.stack([d for d, _ in out]), torch.stack([i for _, i in out]).to(torch.int64)

    def weights_from_k_closest_verts(self, points, verts, k, points_normals=None, verts_normals=None, normal_weight=0.1, p=1):
        """:187-205, Shepard's method -> (weights [bs, n, k], point_verts_idx [bs, n, k] int64); ``p`` a non-negative integer"""
        if not isinstance(p, int) or isinstance(p, bool) or p < 0:
            raise ValueError(f"p: expected a non-negative integer, got {p!r}")
        out = self._search(points, verts, k, points_normals, verts_normals, normal_weight)
        return torch.stack([_shepard(d, None, p, None) for d, _ in out]), torch.stack([i for _, i in out]).to(torch.int64)

    # ---- the skinning half -----------------------------------------------------------------------------------------------------------

    def _frames(self, smplx_output):
        A = _f32(getattr(smplx_output, "transform_mat", None), "smplx_output.transform_mat", dim=4)
        if tuple(A.shape[1:]) != (self.lbs_weights.shape[1], 4, 4):
            raise ValueError(f"smplx_output.transform_mat: expected [B, {self.lbs_weights.shape[1]}, 4, 4], got {tuple(A.shape)}")
        _same_device(("lbs_weights", self.lbs_weights), ("smplx_output.transform_mat", A))
        return A

    def _skin_args(self, vertices, W, A, global_transl, scale):
        B, J = A.shape[0], A.shape[1]
        v = _f32(vertices, "vertices", dim=(2, 3), last=3)
        v = v[None] if v.dim() == 2 else v
        if W is not None:                        # None: the weights are still to be computed, one row per vertex
            W = _f32(W, "lbs_w", dim=3, last=J)
            if W.shape[0] not in (1, B):
                raise ValueError(f"lbs_w: expected [{B}, P, {J}] or [1, P, {J}], got {tuple(W.shape)}")
        P = v.shape[1] if W is None else W.shape[1]
        if v.shape[0] not in (1, B) or v.shape[1] != P:
            raise ValueError(f"vertices: expected [{B}, {P}, 3] or [1, {P}, 3], got {tuple(v.shape)}")
        tr = None
        if global_transl is not None:
            tr = _f32(global_transl, "global_transl", dim=(1, 2), last=3)
            tr = tr[None] if tr.dim() == 1 else tr
            if tr.shape[0] not in (1, B):
                raise ValueError(f"global_transl: expected [{B}, 3], got {tuple(tr.shape)}")
            tr = tr.expand(B, 3).contiguous()
        sc = None
        if scale is not None:
            sc = _f32(scale, "scale", dim=(0, 1))
            if sc.dim() == 1 and sc.shape[0] not in (1, B):
                raise ValueError(f"scale: expected a 0-dimensional tensor or [{B}], got {tuple(sc.shape)}")
        _same_device(("lbs_weights", self.lbs_weights), ("vertices", v), ("lbs_w", W), ("global_transl", tr), ("scale", sc))
        return v, W, tr, sc, B, P, J

    def _skin(self, name, v, W, A, tr, sc, B, P, J, with_T):
        dev = A.device
        pnts = torch.empty(1, B, P, 3, dtype=torch.float32, device=dev)
        T = torch.empty(1, B, P, 4, 4, dtype=torch.float32, device=dev) if with_T else None
        if B > 0 and P > 0:
            call(name, dev, v.data_ptr(), int(v.shape[0] == B and B > 1), W.data_ptr(), int(W.shape[0] == B and B > 1), A.data_ptr(), B, P, J, ptr(tr),
                 ptr(sc), int(sc is not None and sc.dim() == 1 and sc.shape[0] == B and B > 1), pnts.data_ptr(), ptr(T))
        return pnts, T

    def transform_to_t_pose(self, vertices, smplx_output, global_transl=None, scale=None, lbs_w=None, k=10, v_normals=None, smplx_normals=None,
                            normal_weight=0.1, with_T=True):
        """:207-288 -> (pnts [1, B, P, 3], T [1, B, P, 4, 4] the inverse blended transforms, W).  With ``lbs_w`` [B or 1, P, J] given,
        W is ``lbs_w`` and nothing is searched; otherwise W [B, P, J] are Shepard's weights (power 2) of the k nearest body vertices
        ``smplx_output.vertices`` over ``lbs_weights``, found in six dimensions when normals are given.  ``global_transl`` [B, 3] and
        ``scale`` (0-dimensional or [B]) are required, as in the reference.  ``with_T=False``: the T slot is None and nothing is written
        for it.  Not differentiable: no output carries a graph."""
        if global_transl is None or scale is None:
            raise ValueError("transform_to_t_pose: global_transl and scale are required (the reference fails on None)")
        A = self._frames(smplx_output)
        if lbs_w is None:
            body = _f32(getattr(smplx_output, "vertices", None), "smplx_output.vertices", dim=3, last=3)
            if body.shape[0] != A.shape[0] or body.shape[1] != self.lbs_weights.shape[0]:
                raise ValueError(f"smplx_output.vertices: expected [{A.shape[0]}, {self.lbs_weights.shape[0]}, 3], got {tuple(body.shape)}")
            self._skin_args(vertices, None, A, global_transl, scale)              # every check before the first launch
            out = self._search(vertices, body, k, v_normals, smplx_normals, normal_weight)
            W = torch.stack([_shepard(d, i, 2, self.lbs_weights) for d, i in out])
        else:
            W = lbs_w
        v, Wc, tr, sc, B, P, J = self._skin_args(vertices, W, A, global_transl, scale)
        pnts, T = self._skin("mpmhip_skin_to_tpose", v, Wc, A, tr, sc, B, P, J, with_T)
        return pnts, T, (Wc if lbs_w is None else lbs_w.detach())

    def transform_to_pose(self, vertices, lbs_weights_pnts, smplx_output, global_transl=None, scale=None, with_T=True):
        """:290-337 -> (pnts [1, B, P, 3], T [1, B, P, 4, 4]): ``(T (v, 1))[:3]``, then ``+ global_transl``, then ``* scale``, each only
        if given.  ``lbs_weights_pnts`` [B, P, J] or [1, P, J] and ``vertices`` [B, P, 3], [1, P, 3] or [P, 3]: the repeats of
        train_material_params.py:344-345 are not needed.  ``with_T=False``: the T slot is None and nothing is written for it.  Not
        differentiable: no output carries a graph."""
        A = self._frames(smplx_output)
        v, W, tr, sc, B, P, J = self._skin_args(vertices, lbs_weights_pnts, A, global_transl, scale)
        return self._skin("mpmhip_skin_to_pose", v, W, A, tr, sc, B, P, J, with_T)
