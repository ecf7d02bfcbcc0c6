"""Golden vectors for re-posing FROM THE REFERENCE'S OWN METHODS (tests/golden/repose.npz).

``find_k_closest_verts``, ``weights_from_k_closest_verts``, ``transform_to_t_pose`` and ``transform_to_pose`` are cut out of the
``SmplxDeformer`` class body of the reference's utils/smplx_deformer.py with ``ast`` at generation time and executed unchanged, as plain
functions whose ``self`` is a stand-in namespace (``device``, ``smplx_model.lbs_weights``, ``smplx_model.J_regressor``, of which only
``shape[0]`` is read); this script contains none of their text.  ``smplx_output`` is a namespace with ``transform_mat``, ``vertices``
and ``v_shaped`` (read for a value the reference never uses).

pytorch3d is not installed where this runs, so ``knn_points`` is bound to the float64 brute-force stand-in below: the direct-form
squared distance, a stable sort, the lowest index on ties.  The k-nearest search itself is therefore pinned by the twin
(tests/repose_twin_torch.py) and not by the reference, as ``matrix_to_quaternion`` was for the tracking step; what the reference pins
is everything built on it: the six-dimensional points, Shepard's weights, the gather, the blended transforms, their inverse, the
order of scale and translation, and the shapes.

Everything in float64 on the float32 inputs of tests/repose_cases.py.  The reference takes W and the vertices repeated per frame; the
cases' [1, P, J] weights are repeated here, in the generator only.  To stay within the size limit the [1, B, P, 4, 4] transforms and
the searched [B, P, J] weights are kept for every (P // 16)-th point (repose_cases.t_rows) with their full shapes on the side; the
points, which depend on all of them, are kept in full.  Data only: expected outputs.
    python tests/golden/make_golden_repose.py        (needs the reference checkout that make_golden_raster.py names)"""
import ast
import os
import sys
import types
from collections import namedtuple

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import repose_cases as rc  # noqa: E402
from make_golden_raster import REF  # noqa: E402

METHODS = ["find_k_closest_verts", "weights_from_k_closest_verts", "transform_to_t_pose", "transform_to_pose"]
KNN = namedtuple("KNN", "dists idx knn")


def knn_points(p1, p2, K=1):
    """the stand-in: [B, N, D] x [B, M, D] -> dists [B, N, K] ascending, idx [B, N, K] long, lowest index on ties"""
    d2 = ((p1[:, :, None, :] - p2[:, None, :, :]) ** 2).sum(-1)
    d, i = torch.sort(d2, dim=-1, stable=True)
    return KNN(d[..., :K], i[..., :K], None)


def cut_methods(path, cls, names, ns):
    """exec the methods `names` of the class `cls` of the reference file `path` into ns, as plain functions"""
    for node in ast.parse(open(path).read()).body:
        if isinstance(node, ast.ClassDef) and node.name == cls:
            for item in node.body:
                if isinstance(item, ast.FunctionDef) and item.name in names:
                    exec(compile(ast.Module(body=[item], type_ignores=[]), path, "exec"), ns)
    missing = [n for n in names if n not in ns]
    assert not missing, missing
    return ns


def d(a):
    return None if a is None else torch.tensor(np.asarray(a), dtype=torch.float64)


def deformer(ns, lbs):
    """the stand-in for self: the four methods bound to a namespace"""
    self = types.SimpleNamespace(device="cpu", smplx_model=types.SimpleNamespace(lbs_weights=lbs, J_regressor=torch.zeros(lbs.shape[1], 1)))
    for n in METHODS:
        setattr(self, n, types.MethodType(ns[n], self))
    return self


def main():
    ns = cut_methods(os.path.join(REF, "utils", "smplx_deformer.py"), "SmplxDeformer", METHODS, {"torch": torch, "knn_points": knn_points})
    out = {}
    plain = deformer(ns, torch.zeros(12, 3, dtype=torch.float64))
    for name in rc.ALL_KNN:
        c = rc.knn_case(name)
        p1, p2 = d(c["p1"])[None], d(c["p2"])[None]
        kw = dict(points_normals=p1[..., 3:], verts_normals=p2[..., 3:], normal_weight=1.0) if p1.shape[-1] == 6 else {}
        dists, idx = plain.find_k_closest_verts(p1[..., :3], p2[..., :3], c["K"], **kw)
        assert dists.shape == idx.shape == (1, p1.shape[1], c["K"]) and idx.dtype == torch.int64
        out[f"{name}_dists"], out[f"{name}_idx"] = dists[0].numpy(), idx[0].numpy().astype(np.int32)
    rng = np.random.default_rng(0)
    for name in rc.ALL_SKIN:
        c = rc.skin_case(name)
        B, P, J = c["A"].shape[0], c["verts"].shape[1], c["A"].shape[1]
        searched = c["W"] is None
        lbs = d(c["lbs"]) if searched else torch.zeros(12, J, dtype=torch.float64)
        body = d(c["body"]) if searched else d(rng.normal(0, 1, (B, 12, 3)))       # a given lbs_w still runs the (unused) search
        smplx = types.SimpleNamespace(transform_mat=d(c["A"]), vertices=body, v_shaped=torch.zeros_like(body))
        self = deformer(ns, lbs)
        W = None if searched else d(c["W"]).repeat(B // c["W"].shape[0], 1, 1)
        if c["direction"] == "pose":
            pnts, T = self.transform_to_pose(d(c["verts"]), W, smplx, d(c["transl"]), d(c["scale"]))
        else:
            pnts, T, W_out = self.transform_to_t_pose(d(c["verts"]), smplx, d(c["transl"]), d(c["scale"]), lbs_w=W, k=c.get("k", 10),
                                                      v_normals=d(c.get("normals")), smplx_normals=d(c.get("body_normals")),
                                                      normal_weight=rc.NORMAL_WEIGHT)
        assert pnts.shape == (1, B, P, 3) and T.shape == (1, B, P, 4, 4) and pnts.dtype == torch.float64
        rows = rc.t_rows(P)
        out[f"{name}_pnts"], out[f"{name}_T"], out[f"{name}_T_shape"] = pnts.numpy(), T[:, :, rows].numpy(), np.array(T.shape)
        if searched:
            _, idx = self.weights_from_k_closest_verts(d(c["verts"]), body, k=c["k"], p=2, points_normals=d(c["normals"]),
                                                       verts_normals=d(c["body_normals"]), normal_weight=rc.NORMAL_WEIGHT)
            assert W_out.shape == (B, P, J)
            out[f"{name}_idx"], out[f"{name}_W"], out[f"{name}_W_shape"] = idx.numpy().astype(np.int32), W_out[:, rows].numpy(), np.array(W_out.shape)
    path = os.path.join(HERE, "repose.npz")
    np.savez_compressed(path, **out)
    print("repose.npz: %d bytes" % os.path.getsize(path), {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
