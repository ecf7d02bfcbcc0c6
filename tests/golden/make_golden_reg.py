"""Golden vectors for the regularisation terms of the appearance loop FROM THE REFERENCE'S OWN FUNCTIONS (tests/golden/reg.npz).

What train_appearance.py:136-150 computes per iteration: ``find_adjacent_faces`` (utils/general_utils.py:286-316), the set-up lines of
``MeshGaussianModel.init_from_trained_model`` (scene/mesh_gaussian_model.py:88-98) and its methods ``normal_loss``, ``opacity_loss``, ``iso_loss`` and
``area_loss`` (:203-246) are cut out of the reference's files with ``ast`` at generation time and executed unchanged on a
``SimpleNamespace`` model; this script contains none of their text.  The xyz and scale terms exist only inline in the training loop
(train_appearance.py:147-148) and are evaluated here with torch.  Everything in float64 on the float32 inputs of the mesh cases
sheet, closed and one and of the Gaussian case main of tests/reg_cases.py: the neighbour arrays, neighbor_dist and neighbor_weight,
the terms, and the gradient of each term.  Data only: inputs and expected outputs.
    python tests/golden/make_golden_reg.py        (needs the reference checkout that make_golden_raster.py names)"""
import ast
import os
import sys
from collections import defaultdict
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import reg_cases as rc  # noqa: E402
from make_golden_raster import REF, cut  # noqa: E402


def class_body(path, cls):
    for node in ast.parse(open(path).read()).body:
        if isinstance(node, ast.ClassDef) and node.name == cls:
            return node.body
    raise KeyError(cls)


def cut_methods(path, cls, names, ns):
    """exec the methods called `names` of class `cls` of the reference file `path` into ns, as plain functions of self"""
    for node in class_body(path, cls):
        if isinstance(node, ast.FunctionDef) and node.name in names:
            exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    assert all(n in ns for n in names)
    return ns


def cut_statements(path, cls, method, first, last):
    """the statements of cls.method on lines first..last, compiled as they stand"""
    init = [n for n in class_body(path, cls) if isinstance(n, ast.FunctionDef) and n.name == method][0]
    body = [n for n in init.body if first <= n.lineno and n.end_lineno <= last]
    assert body and body[0].lineno == first and body[-1].end_lineno == last
    return compile(ast.Module(body=body, type_ignores=[]), path, "exec")


def main():
    model_py = os.path.join(REF, "scene", "mesh_gaussian_model.py")
    gu = cut(os.path.join(REF, "utils", "general_utils.py"), ["find_adjacent_faces"], {"np": np, "defaultdict": defaultdict})
    setup = cut_statements(model_py, "MeshGaussianModel", "init_from_trained_model", 88, 98)
    fn = cut_methods(model_py, "MeshGaussianModel", ["normal_loss", "opacity_loss", "iso_loss", "area_loss"], {"torch": torch})
    out = {}
    for name in ("sheet", "closed", "one"):
        c = rc.mesh_case(name)
        out.update({f"{name}_{k}": np.asarray(v) for k, v in c.items()})
        me = SimpleNamespace(faces=torch.from_numpy(c["faces"].astype(np.int64)), verts_orig=torch.tensor(c["verts0"], dtype=torch.float64)[None])
        exec(setup, {"torch": torch, "find_adjacent_faces": gu["find_adjacent_faces"], "self": me, "device": "cpu"})
        assert me.face_neighbors.dtype == torch.int32 and me.neighbor_dist.dtype == torch.float64
        out[f"{name}_face_neighbors"] = me.face_neighbors.numpy()
        out[f"{name}_neighbor_dist"], out[f"{name}_neighbor_weight"] = me.neighbor_dist.numpy(), me.neighbor_weight.numpy()
        me.verts = torch.tensor(c["verts"], dtype=torch.float64, requires_grad=True)
        terms = [fn["normal_loss"](me), fn["iso_loss"](me), fn["area_loss"](me)]
        out[f"{name}_terms"] = torch.stack(terms).detach().numpy()
        for k, t in zip(rc.MESH_GRADS, terms):
            out[f"{name}_{k}"] = torch.autograd.grad(t, me.verts)[0].numpy()
    c = rc.gauss_case("main")
    out.update({f"gauss_{k}": np.asarray(v) for k, v in c.items()})
    opa, xyz, scl = [torch.tensor(c[k], dtype=torch.float64, requires_grad=True) for k in rc.GAUSS_GRADS]
    vis = torch.from_numpy(c["radii"] > 0)                                                # render()'s visibility_filter = radii > 0
    t_xyz, t_scale = rc.THRESHOLDS
    me = SimpleNamespace(get_opacity=torch.sigmoid(opa))                                  # scene/gaussian_model.py:158
    terms = [fn["opacity_loss"](me), F.relu(xyz[vis].norm(dim=1) - t_xyz).mean(), F.relu(torch.exp(scl[vis]) - t_scale).norm(dim=1).mean()]
    out["gauss_terms"] = torch.stack(terms).detach().numpy()
    for k, leaf, t in zip(rc.GAUSS_GRADS, (opa, xyz, scl), terms):
        out[f"gauss_d{k}"] = torch.autograd.grad(t, leaf)[0].numpy()
    path = os.path.join(HERE, "reg.npz")
    np.savez_compressed(path, **out)
    print("reg.npz: %d bytes" % os.path.getsize(path), {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
