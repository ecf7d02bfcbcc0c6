"""The optimiser step of the appearance loop on the device, and the reference's learning-rate schedules: the two lines of
train_appearance.py that were left to torch,

    gaussians.update_learning_rate(iteration)                  # train_appearance.py:112
    gaussians.optimizer.step(); optimizer.zero_grad(...)       # :260-261

over csrc/adam.hip:

    groups = appearance_param_groups(_xyz, _features_dc, _features_rest, _opacity, _scaling, _rotation, verts_offset,
                                     [cam_m, cam_c], shadow_net.parameters(), opt, spatial_lr_scale)
    optimizer = FusedAdam(groups, lr=0.0, eps=1e-15)           # for torch.optim.Adam(l, lr=0.0, eps=1e-15), scene/gaussian_model.py:222
    update_learning_rate(optimizer, iteration)                 # the xyz and verts schedules
    optimizer.step()                                           # ONE launch per 48 tensors, whatever the number of groups

``FusedAdam`` is Adam without amsgrad and without weight decay, which is all the reference uses.  Per element it does the operations
of torch's single-tensor implementation in their order (csrc/adam_math.hpp), in fp32 without contraction, with the scalars computed
here in Python doubles as torch computes them.  Its state has torch's keys and types (``step`` a float32 CPU scalar, ``exp_avg``,
``exp_avg_sq``), so ``densify.adam_moments``, ``DensifyResult.swap_into`` and ``densify.reset_opacity`` work on it unchanged and a
``state_dict`` goes to and from ``torch.optim.Adam``.  One difference: a group whose learning rate is exactly zero (``f_rest``, and
``verts`` with the default arguments) still moves its moments, but its parameters are neither read nor written -- torch would write
``p - 0 * (m / d)``, which is ``p`` unless ``m / d`` is not finite and NaN then.  No CPU fallback: parameters must live on an MI355X.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L
from ._call import call

ADAM_CHUNK, MAX_TENSORS = 4096, 48          # MPMHIP_ADAM_CHUNK, MPMHIP_ADAM_MAX_TENSORS
_UNSUPPORTED = ("amsgrad", "maximize", "capturable", "differentiable")
# the order and the names of the groups of the two training_setup methods (scene/gaussian_model.py:212-220,
# scene/mesh_gaussian_model.py:151-162)
GROUP_NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "verts", "cams", "shadow")


def expon_lr(step, lr_init, lr_final, lr_delay_steps=0, lr_delay_mult=1.0, max_steps=1000000):
    """The schedule of utils/general_utils.py:31-64 as a function of the step: log-linear from ``lr_init`` at 0 to ``lr_final`` at
    ``max_steps`` and constant behind it, times an eased-in factor that starts at ``lr_delay_mult`` while ``step <
    lr_delay_steps``.  0.0 for a negative step and where both rates are zero (the group is switched off)."""
    if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
        return 0.0
    ease = 1.0
    if lr_delay_steps > 0:
        ease = lr_delay_mult + (1 - lr_delay_mult) * np.sin(0.5 * np.pi * np.clip(step / lr_delay_steps, 0, 1))
    t = np.clip(step / max_steps, 0, 1)
    return ease * np.exp(np.log(lr_init) * (1 - t) + np.log(lr_final) * t)


def appearance_param_groups(_xyz, _features_dc, _features_rest, _opacity, _scaling, _rotation, verts_offset, cams, shadow, opt,
                            spatial_lr_scale):
    """-> the nine parameter groups of ``MeshGaussianModel.training_setup`` (GROUP_NAMES), in its order and with its rates.  ``cams``
    and ``shadow`` are iterables of parameters (``[cam_m, cam_c]``, ``shadow_net.parameters()``); ``opt`` carries the names of
    arguments/__init__.py:115-126.  The ``xyz`` and ``verts`` groups also carry ``"schedule"``, the arguments of ``expon_lr`` that
    ``update_learning_rate`` reads."""
    s = spatial_lr_scale
    schedule = lambda k: dict(lr_init=getattr(opt, k + "_lr_init") * s, lr_final=getattr(opt, k + "_lr_final") * s,
                              lr_delay_mult=getattr(opt, k + "_lr_delay_mult"), max_steps=getattr(opt, k + "_lr_max_steps"))
    return [{"params": [_xyz], "lr": opt.position_lr_init * s, "name": "xyz", "schedule": schedule("position")},
            {"params": [_features_dc], "lr": opt.feature_lr, "name": "f_dc"},
            {"params": [_features_rest], "lr": 0.0, "name": "f_rest"},
            {"params": [_opacity], "lr": opt.opacity_lr, "name": "opacity"},
            {"params": [_scaling], "lr": opt.scaling_lr, "name": "scaling"},
            {"params": [_rotation], "lr": opt.rotation_lr, "name": "rotation"},
            {"params": [verts_offset], "lr": opt.verts_lr_init * s, "name": "verts", "schedule": schedule("verts")},
            {"params": list(cams), "lr": 1e-4, "name": "cams"},
            {"params": list(shadow), "lr": 1e-4, "name": "shadow"}]


def update_learning_rate(optimizer, iteration):
    """``update_learning_rate`` of both models (scene/gaussian_model.py:228-234, scene/mesh_gaussian_model.py:164-170): every group
    that carries a ``"schedule"`` gets ``expon_lr(iteration, **schedule)`` as its ``lr``.  -> {group name: rate}"""
    out = {}
    for group in optimizer.param_groups:
        if "schedule" in group:
            group["lr"] = out[group.get("name")] = expon_lr(iteration, **group["schedule"])
    return out


def adam_scalars(lr, betas, eps, step):
    """-> (step_size, bc2_sqrt, w1, beta2, w2, eps) of csrc/adam_math.hpp for a parameter at its ``step``-th step, in Python doubles
    as torch's ``_single_tensor_adam`` computes them; they are rounded to fp32 once, where they are handed to the library"""
    beta1, beta2 = betas
    return (lr / (1 - beta1 ** step), (1 - beta2 ** step) ** 0.5, 1 - beta1, beta2, 1 - beta2, eps)


def pack(rows):
    """rows [(p, g, m, v, count, six scalars in double, update)] -> (the arguments of mpmhip_adam_step behind device and stream, the
    host arrays they point into, which must outlive the call)"""
    n = len(rows)
    ptrs = [(C.c_void_p * n)(*[row[k].data_ptr() for row in rows]) for k in range(4)]
    counts = (C.c_int64 * n)(*[row[4] for row in rows])
    scalars = np.ascontiguousarray(np.array([row[5] for row in rows], np.float64).reshape(n, 6).astype(np.float32).T)      # [6, n], rounded once
    update = (C.c_uint8 * n)(*[int(row[6]) for row in rows])
    args = [n] + [C.addressof(a) for a in ptrs] + [C.addressof(counts)] + [scalars[k].ctypes.data for k in range(6)] + [C.addressof(update)]
    return args, (ptrs, counts, scalars, update, rows)


class FusedAdam(torch.optim.Optimizer):
    """``torch.optim.Adam(params, lr, betas, eps)`` with the whole step in csrc/adam.hip.  ``step()`` reads ``group["lr"]`` when it
    is called (a float or a ``numpy.float64``), skips a parameter whose ``.grad`` is None (its ``step`` does not advance), makes one
    library call per device and never synchronises.  Not supported, and a ValueError: weight decay, amsgrad, maximize, capturable,
    differentiable, a closure, sparse gradients, parameters that are not contiguous fp32 tensors on the GPU."""

    def __init__(self, params, lr=0.0, betas=(0.9, 0.999), eps=1e-15, weight_decay=0.0, amsgrad=False, *, maximize=False,
                 capturable=False, differentiable=False):
        if isinstance(lr, torch.Tensor):
            raise ValueError("FusedAdam: lr must be a number (a tensor would have to be read back every step)")
        if not 0.0 <= lr or not 0.0 <= eps or not all(0.0 <= b < 1.0 for b in betas):
            raise ValueError(f"FusedAdam: invalid lr {lr}, eps {eps} or betas {betas}")
        # the keys of torch.optim.Adam's groups, so that a state_dict of either loads into the other
        defaults = dict(lr=lr, betas=tuple(float(b) for b in betas), eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                        foreach=None, capturable=capturable, differentiable=False, fused=None, decoupled_weight_decay=False)
        if differentiable:
            raise ValueError("FusedAdam does not support differentiable")
        super().__init__(params, defaults)
        for group in self.param_groups:
            self._check_group(group)

    @staticmethod
    def _check_group(group):
        if group["weight_decay"] != 0:
            raise ValueError("FusedAdam does not support weight_decay")
        for k in _UNSUPPORTED:
            if group.get(k):
                raise ValueError(f"FusedAdam does not support {k}")
        if isinstance(group["lr"], torch.Tensor):
            raise ValueError("FusedAdam: lr must be a number")

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._check_group(self.param_groups[-1])

    @staticmethod
    def _check_tensors(p):
        if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.layout == torch.strided):
            raise ValueError(f"FusedAdam: expected a contiguous float32 parameter on the GPU, got {p.dtype} {tuple(p.shape)} on {p.device}")
        g = p.grad
        if g.is_sparse:
            raise ValueError("FusedAdam does not support sparse gradients")
        if not (g.dtype == torch.float32 and g.device == p.device and g.shape == p.shape and g.layout == torch.strided):
            raise ValueError("FusedAdam: the gradient must be a float32 tensor of the parameter's shape on its device")

    def _rows(self):
        """every check, then the state of this step -> {device: [(p, g, m, v, count, six scalars, update)]}; ``step`` has advanced"""
        work = []                                                   # (group, parameter); nothing is touched before every check has passed
        for group in self.param_groups:
            self._check_group(group)
            for p in group["params"]:
                if p.grad is not None:
                    self._check_tensors(p)
                    work.append((group, p))
        rows = {}
        for group, p in work:
            state = self.state[p]
            if len(state) == 0:
                state["step"] = torch.tensor(0.0, dtype=torch.float32)
                state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            if state["step"].is_cuda:                               # a state_dict of torch's fused=True keeps it on the device
                state["step"] = state["step"].cpu()
            m, v = state["exp_avg"], state["exp_avg_sq"]
            for t, k in ((m, "exp_avg"), (v, "exp_avg_sq")):
                if not (t.dtype == torch.float32 and t.device == p.device and t.shape == p.shape and t.is_contiguous()):
                    raise ValueError(f"FusedAdam: {k} must be a contiguous float32 tensor of the parameter's shape on its device")
            state["step"] += 1
            step = float(state["step"])
            lr = float(group["lr"])
            g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
            rows.setdefault(p.device, []).append((p, g, m, v, p.numel(), adam_scalars(lr, group["betas"], group["eps"], step), lr != 0.0))
        return rows

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise ValueError("FusedAdam does not support a closure")
        L.load()
        for dev, rows in self._rows().items():
            args, _keep = pack(rows)
            call("mpmhip_adam_step", dev, *args)
        return None
