"""Golden vectors for the mesh tracking step FROM THE REFERENCE'S OWN FUNCTIONS (tests/golden/track.npz).

``compute_face_normals``, ``compute_face_barycenters``, ``compute_face_areas``, ``compute_vertex_normals`` and ``compute_q_from_faces``
(preprocess/utils/geo_utils.py) and ``collision_penalty`` (preprocess/losses/physics.py, over ``NearestNeighbour`` and
``PairwiseDistance`` of preprocess/losses/layers.py) are cut out of the reference's files with ``ast`` at generation time and executed
unchanged; this script contains none of their text.  pytorch3d is not installed where this runs, so ``matrix_to_quaternion`` is bound
to a stand-in that returns its argument: the fixture pins the [F, 3, 3] rotation matrices by the reference's own code, and the
conversion behind them is pinned by nothing but tests/track_twin_torch.py (UNCONFIRMED).

Everything in float64 on the float32 inputs of the mesh cases sheet, closed, one and ties and of every collision case of
tests/track_cases.py: values, gradients to ``vertices`` and ``va`` (upstream weights w_* of the cases), and nearest indices.
Data only: expected outputs.
    python tests/golden/make_golden_track.py        (needs the reference checkout that make_golden_raster.py names)"""
import os
import sys
import warnings

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import track_cases as tc  # noqa: E402
from make_golden_raster import REF, cut  # noqa: E402


def main():
    warnings.simplefilter("ignore")                                               # torch.cross without dim, as the reference calls it
    geo = cut(os.path.join(REF, "preprocess", "utils", "geo_utils.py"),
              ["normalize", "compute_face_normals", "compute_face_barycenters", "compute_face_areas", "compute_vertex_normals",
               "compute_q_from_faces"], {"torch": torch, "matrix_to_quaternion": lambda m: m})
    layers = cut(os.path.join(REF, "preprocess", "losses", "layers.py"), ["PairwiseDistance", "NearestNeighbour"], {"torch": torch, "nn": nn})
    phys = cut(os.path.join(REF, "preprocess", "losses", "physics.py"), ["collision_penalty"], {"torch": torch, "NearestNeighbour": layers["NearestNeighbour"]})
    d = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    out = {}
    for name in tc.FIXTURE_MESHES:
        c = tc.mesh_case(name)
        assert c["faces"].shape[0] != 3                                           # torch.cross without dim would take the wrong axis
        faces, v = torch.from_numpy(c["faces"].astype(np.int64)), d(c["verts"]).requires_grad_(True)
        normals = geo["compute_face_normals"](v, faces)
        vals = {"means3D": geo["compute_face_barycenters"](v, faces), "matrices": geo["compute_q_from_faces"](v, faces, normals),
                "face_normals": normals, "face_areas": geo["compute_face_areas"](v, faces), "vertex_normals": geo["compute_vertex_normals"](v, faces)}
        assert vals["matrices"].shape == (faces.shape[0], 3, 3)
        out.update({f"{name}_{k}": t.detach().numpy() for k, t in vals.items()})
        for k, w in (("means3D", c["w_means3D"]), ("matrices", c["w_matrices"]), ("face_areas", c["w_opacities"][:, 0])):
            out[f"{name}_d_{k}"] = torch.autograd.grad((d(w) * vals[k]).sum(), v, retain_graph=True)[0].numpy()
    for name in tc.COLLISION_CASES:
        c = tc.collision_case(name)
        va, vb, nb = d(c["va"]).requires_grad_(True), d(c["vb"]), d(c["nb"])
        out[f"{name}_index"] = layers["NearestNeighbour"]()(va.detach(), vb).numpy()
        assert out[f"{name}_index"].dtype == np.int32
        for mode, kw in (("distance", dict(return_distance=True)), ("average", dict(return_average=True)), ("cubed", dict(return_average=False))):
            y = phys["collision_penalty"](va, vb, nb, eps=c["eps"], **kw)
            out[f"{name}_{mode}"] = y.detach().numpy()
            out[f"{name}_d_{mode}"] = torch.autograd.grad((d(c["w"]) * y).sum() if mode == "distance" else y, va)[0].numpy()
    path = os.path.join(HERE, "track.npz")
    np.savez_compressed(path, **out)
    print("track.npz: %d bytes" % os.path.getsize(path), {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
