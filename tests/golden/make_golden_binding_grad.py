"""Golden gradients of the mesh binding FROM THE REFERENCE'S OWN CODE under torch autograd, in float64.

The reference's ``compute_face_orientation`` (utils/graphics_utils.py:88-107) and the ``GaussianModel`` getters ``get_xyz``,
``get_rotation``, ``get_scaling``, ``get_opacity`` (scene/gaussian_model.py:112-160) are imported UNCHANGED; the face frames are put
together as ``MeshGaussianModel.set_mesh_by_verts`` does (scene/mesh_gaussian_model.py:137-146).  roma is not in this image: its
``rotmat_to_unitquat``, ``quat_product``, ``quat_xyzw_to_wxyz`` and ``quat_wxyz_to_xyzw`` are the functions of
tests/binding_twin_torch.py (plyfile and simple_knn, which the getters do not touch, are empty stand-ins as in make_golden_render.py).
The reference's code preserves the dtype of what it is given, so the whole chain runs in float64 on the float32 inputs below.

The case: icosphere(2, 0.5, (1, 1, 1)) -- 162 vertices, 320 faces -- with N(0, 4e-3) vertex noise; n = 2 * 320 + 17 Gaussians bound at
random and unsorted, 300 of them forced onto one face, the last five faces left empty; random weights on all four outputs, so that
the loss is  sum(w_m * means3D) + sum(w_r * rotations) + sum(w_s * scales) + sum(w_o * opacities).  Data only: inputs, weights and the
gradients of that loss for verts, _xyz, _rotation, _scaling, _opacity.
    python tests/golden/make_golden_binding_grad.py        (build container: needs /root/reference)"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, "/root/reference")
import binding_twin_torch as tw  # noqa: E402


def _stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


_stub("plyfile", PlyData=object, PlyElement=object)
_stub("simple_knn")
_stub("simple_knn._C", distCUDA2=None)
_stub("roma", quat_product=tw.quat_product, quat_xyzw_to_wxyz=tw.quat_xyzw_to_wxyz, quat_wxyz_to_xyzw=tw.quat_wxyz_to_xyzw,
      rotmat_to_unitquat=tw.rotmat_to_unitquat)

import importlib.util  # noqa: E402
_spec = importlib.util.spec_from_file_location("ref_gaussian_model", "/root/reference/scene/gaussian_model.py")  # (not the package:
_mod = importlib.util.module_from_spec(_spec)       # scene/__init__.py pulls the dataset readers and their dependencies in)
_spec.loader.exec_module(_mod)
GaussianModel = _mod.GaussianModel  # the reference's class
from roma import quat_xyzw_to_wxyz, rotmat_to_unitquat  # noqa: E402  (the stand-in above, as mesh_gaussian_model.py imports them)
from utils.graphics_utils import compute_face_orientation  # noqa: E402  (the reference's function)
from mpmavatar_amd import garment  # noqa: E402

SEED, N_HOT, N_EMPTY = 7, 300, 5
NAMES = ("verts", "_xyz", "_rotation", "_scaling", "_opacity")


def main():
    rng = np.random.default_rng(SEED)
    verts, faces = garment.icosphere(2, 0.5, (1.0, 1.0, 1.0))
    verts = (verts + rng.normal(0, 4e-3, verts.shape)).astype(np.float32)
    n_f = faces.shape[0]
    n = 2 * n_f + 17
    binding = rng.integers(0, n_f - N_EMPTY, n)
    hot = int(rng.integers(0, n_f - N_EMPTY))
    binding[rng.permutation(n)[:N_HOT]] = hot
    inp = {"_xyz": rng.normal(0, 0.4, (n, 3)), "_rotation": rng.normal(size=(n, 4)), "_scaling": rng.normal(-1.0, 0.6, (n, 3)),
           "_opacity": rng.normal(0, 2, (n, 1))}
    inp = {k: v.astype(np.float32) for k, v in inp.items()}
    w = {"w_means3D": rng.normal(size=(n, 3)), "w_rotations": rng.normal(size=(n, 4)), "w_scales": rng.normal(size=(n, 3)),
         "w_opacities": rng.normal(size=(n, 1))}
    w = {k: v.astype(np.float32) for k, v in w.items()}

    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in dict(verts=verts, **inp).items()}
    tf = torch.from_numpy(faces.astype(np.int64))
    pc = GaussianModel(0)
    for k in inp:
        setattr(pc, k, t[k])
    pc.binding = torch.from_numpy(binding.astype(np.int64))
    pc.face_center = t["verts"][tf].mean(dim=-2)                                  # mesh_gaussian_model.py:137-146
    pc.face_orien_mat, pc.face_scaling = compute_face_orientation(t["verts"], tf, return_scale=True)
    pc.face_orien_quat = quat_xyzw_to_wxyz(rotmat_to_unitquat(pc.face_orien_mat))
    out = {"means3D": pc.get_xyz, "rotations": pc.get_rotation, "scales": pc.get_scaling, "opacities": pc.get_opacity}
    assert all(v.dtype == torch.float64 for v in out.values())
    loss = sum((torch.tensor(w["w_" + k], dtype=torch.float64) * v).sum() for k, v in out.items())
    grads = torch.autograd.grad(loss, [t[k] for k in NAMES])
    np.savez_compressed(os.path.join(HERE, "binding_grad.npz"), verts=verts, faces=faces.astype(np.int32), binding=binding.astype(np.int32),
                        hot_face=np.int32(hot), n_empty=np.int32(N_EMPTY), **inp, **w,
                        **{"d_" + k: g.numpy() for k, g in zip(NAMES, grads)})
    print("binding_grad.npz:", n, "Gaussians,", n_f, "faces, hot face", hot, "with", int((binding == hot).sum()))


if __name__ == "__main__":
    main()
