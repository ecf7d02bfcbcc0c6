"""Golden vectors for the optimiser set-up and the learning-rate schedules FROM THE REFERENCE'S OWN METHODS (tests/golden/optim.npz).

``get_expon_lr_func`` (utils/general_utils.py:31-64) and ``training_setup`` and ``update_learning_rate`` of ``GaussianModel``
(scene/gaussian_model.py:207-234) and of ``MeshGaussianModel`` (scene/mesh_gaussian_model.py:148-170) are cut out of the reference's
files with ``ast`` at generation time and executed unchanged; this script contains none of their text.  The method nodes of each
class are wrapped in a class node of the same name, the second deriving from the first, so that the reference's zero-argument
``super()`` works; the stand-in model is an instance of the second that was given what the methods read (the parameters,
``spatial_lr_scale``, ``get_xyz``, ``shadow_net``).  The optimiser is the real ``torch.optim.Adam`` the reference constructs.  The
methods name ``device="cuda"``; they run on the CPU behind the ``torch`` proxy of make_golden_densify.py.  Everything in float64 on
the float32 inputs of tests/adam_cases.py.  Data only: group names, order and parameter counts, eps and betas, the learning rate of
every group at the iterations of adam_cases.ITERATIONS for the reference's default arguments and for adam_cases.OPT, and
parameters and moments of the base case after 25 steps.
    python tests/golden/make_golden_optim.py        (needs the reference checkout that make_golden_raster.py names)"""
import ast
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import adam_cases as ac  # noqa: E402
from make_golden_densify import TorchOnCpu  # noqa: E402
from make_golden_raster import REF, cut  # noqa: E402
from make_golden_reg import class_body  # noqa: E402

METHODS = ("training_setup", "update_learning_rate")
K = 25


def cut_class(path, cls, bases, names, ns):
    """a class `cls` made of the methods `names` of the reference's class of that name, exec'd into ns"""
    body = [n for n in class_body(path, cls) if isinstance(n, ast.FunctionDef) and n.name in names]
    assert len(body) == len(names)
    node = ast.ClassDef(name=cls, bases=[ast.Name(id=b, ctx=ast.Load()) for b in bases], keywords=[], body=body, decorator_list=[], type_params=[])
    exec(compile(ast.fix_missing_locations(ast.Module(body=[node], type_ignores=[])), path, "exec"), ns)
    return ns[cls]


def model(cls, opt_args, scale):
    """-> (model after training_setup, {tensor name: Parameter})"""
    me = object.__new__(cls)
    leaves = {k: nn.Parameter(torch.tensor(v, dtype=torch.float64)) for k, v in ac.params().items()}
    for k in ac.GAUSS:
        setattr(me, k, leaves[k])
    me.verts_offset, me.cam_m, me.cam_c = leaves["verts_offset"], leaves["cam_m"], leaves["cam_c"]
    me.shadow_net = SimpleNamespace(parameters=lambda: iter([leaves[f"shadow{i}"] for i in range(4)]))
    me.spatial_lr_scale = scale
    me.training_setup(SimpleNamespace(percent_dense=0.01, **vars(opt_args)))
    return me, leaves


def main():
    proxy = TorchOnCpu()
    ns = {"torch": proxy, "nn": nn, "np": np}
    cut(os.path.join(REF, "utils", "general_utils.py"), ["get_expon_lr_func"], ns)
    base = cut_class(os.path.join(REF, "scene", "gaussian_model.py"), "GaussianModel", [], METHODS, ns)
    base.get_xyz = property(lambda self: self._xyz)
    cls = cut_class(os.path.join(REF, "scene", "mesh_gaussian_model.py"), "MeshGaussianModel", ["GaussianModel"], METHODS, ns)
    out = {}
    torch.set_default_dtype(torch.float64)
    try:
        for tag, args, scale in (("default", ac.DEFAULT_OPT, 1.0), ("other", ac.OPT, ac.SCALE)):
            me, leaves = model(cls, args, scale)
            groups = me.optimizer.param_groups
            assert isinstance(me.optimizer, torch.optim.Adam)
            out[f"{tag}_names"] = np.array([g["name"] for g in groups])
            out[f"{tag}_counts"] = np.array([len(g["params"]) for g in groups], np.int32)
            named = {id(p): k for k, p in leaves.items()}
            out[f"{tag}_members"] = np.array([",".join(named[id(p)] for p in g["params"]) for g in groups])
            out[f"{tag}_eps"] = np.array([g["eps"] for g in groups], np.float64)
            out[f"{tag}_betas"] = np.array([g["betas"] for g in groups], np.float64)
            out[f"{tag}_lr_setup"] = np.array([g["lr"] for g in groups], np.float64)
            lrs = []
            for it in ac.ITERATIONS:
                me.update_learning_rate(it)
                lrs.append([float(g["lr"]) for g in groups])
            out[f"{tag}_lr"] = np.array(lrs, np.float64)                                   # [iteration, group]
        # the trajectory of the base case: a fresh model, K steps at the iterations of the cases
        me, leaves = model(cls, ac.OPT, ac.SCALE)
        for k in range(1, K + 1):
            me.update_learning_rate(ac.iteration(k))
            for name, p in leaves.items():
                p.grad = torch.tensor(ac.grads(k)[name], dtype=torch.float64)
            me.optimizer.step()
        for name, p in leaves.items():
            st = me.optimizer.state[p]
            assert float(st["step"]) == K
            out["p_" + name], out["m_" + name], out["v_" + name] = p.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()
    finally:
        torch.set_default_dtype(torch.float32)
    path = os.path.join(HERE, "optim.npz")
    np.savez_compressed(path, **out)
    print("optim.npz: %d bytes" % os.path.getsize(path), out["other_names"], out["other_lr"][:2])


if __name__ == "__main__":
    main()
