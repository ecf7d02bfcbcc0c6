"""Densification of the bound Gaussians on the device: the last block of the appearance loop (train_appearance.py:245-257), which
changes the set of Gaussians itself,

    gaussians.max_radii2D[visibility_filter] = torch.max(...)                     # train_appearance.py:248
    gaussians.add_densification_stats(viewspace_point_tensor, visibility_filter)  # scene/gaussian_model.py:524-526
    gaussians.densify_and_prune(max_grad, 0.005, scene_radius, size_threshold)    # :508-522 with :378-506
    gaussians.reset_opacity()                                                     # :284-287

over csrc/densify.hip:

    stats = DensifyStats(n, device)
    stats.add(means2D.grad, radii)                                                # every iteration: one launch, in place, no sync
    res = densify_and_prune(_xyz, _features_dc, _features_rest, _opacity, _scaling, _rotation, binding, n_faces, frames.face_scaling,
                            stats, max_grad, 0.005, extent, size_threshold, percent_dense, moments=adam_moments(optimizer))
    res.swap_into(optimizer)                                                      # cat_tensors_to_optimizer / _prune_optimizer
    new_opacity = reset_opacity(_opacity, optimizer)                              # replace_tensor_to_optimizer

The result is the result of the reference's three steps -- clone, split, prune -- run one after another, row for row and in the
reference's row order: [kept originals | clones | first children | second children], each block in source order.  One pass over the
originals decides everything (csrc/densify_math.hpp); the only host synchronisation of a densification is the read-back of the
counts that size the output, which also carries the error flag of a ``binding`` entry outside [0, n_faces).  fp32; integer atomics
only, so the same input gives the same bits.  The reference's screen-size test is dead (``densification_postfix`` zeroes
``max_radii2D`` before ``densify_and_prune`` reads it): ``max_screen_size`` only switches the world-size test on, here too.  The
reference draws ``torch.normal(0, std)`` per selected point; here child ``c`` of source ``i`` takes ``std * noise[i, c]`` from a
``noise [n, 2, 3]`` of standard normals, sized by ``n`` so that drawing it needs no synchronisation.  No CPU fallback: tensors must
live on an MI355X.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L
from ._call import call, expect

PARAMS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
# the reference's optimiser group of each parameter (scene/gaussian_model.py:433-439)
GROUPS = {"_xyz": "xyz", "_features_dc": "f_dc", "_features_rest": "f_rest", "_opacity": "opacity", "_scaling": "scaling",
          "_rotation": "rotation"}
_MODE = {"_xyz": 2, "_scaling": 3}               # MODE_XYZ, MODE_SCALING of densify_math.hpp; every other parameter is copied
_MOMENT = 1                                      # MODE_MOMENT
_N_COUNTS, _MAX_TENSORS = 8, 24                  # MPMHIP_DENSIFY_COUNTS, MPMHIP_DENSIFY_MAX_TENSORS


def _f32(x):
    return float(np.float32(x))


class DensifyStats:
    """``xyz_gradient_accum [n, 1]``, ``denom [n, 1]`` and ``max_radii2D [n]`` of the model, fp32, zero at the start and after
    every densification."""

    def __init__(self, n: int, device):
        self.device = torch.device(device)
        self.reset(n)

    def reset(self, n: int):
        self.xyz_gradient_accum = torch.zeros(n, 1, dtype=torch.float32, device=self.device)
        self.denom = torch.zeros(n, 1, dtype=torch.float32, device=self.device)
        self.max_radii2D = torch.zeros(n, dtype=torch.float32, device=self.device)

    @property
    def n(self):
        return self.max_radii2D.shape[0]

    def add(self, viewspace_grad: torch.Tensor, radii: torch.Tensor):
        """viewspace_grad [n, 3]: the gradient the rasteriser leaves on ``means2D``; radii: its int32 [n] (visible = radii > 0), or
        a bool [n], which counts as radius 1.  One launch, in place; nothing is allocated and nothing synchronises."""
        n = self.n
        grad = expect(viewspace_grad, torch.float32, "viewspace_grad", shape=(n, 3))
        if not (isinstance(radii, torch.Tensor) and radii.dtype in (torch.int32, torch.bool)):
            raise RuntimeError("radii: expected an int32 or bool tensor on the GPU")
        vis = expect(radii, radii.dtype, "radii", shape=(n,))
        if not (grad.device == vis.device == self.device):
            raise RuntimeError("DensifyStats.add: the tensors must be on the device of the statistics")
        L.load()
        if n == 0:                                   # an empty tensor has no pointer to tell radii from a mask by
            return
        ptrs = (None, vis.data_ptr()) if vis.dtype == torch.bool else (vis.data_ptr(), None)
        call("mpmhip_densify_stats_add", self.device, n, grad.data_ptr(), *ptrs, self.xyz_gradient_accum.data_ptr(), self.denom.data_ptr(),
             self.max_radii2D.data_ptr())


def adam_moments(optimizer, names=None):
    """-> {parameter name: (exp_avg, exp_avg_sq)} of the named groups of a torch.optim.Adam that hold state (none before its first
    step); names: {parameter name: group name}, by default the reference's"""
    names = GROUPS if names is None else names
    out = {}
    for group in optimizer.param_groups:
        for k, g in names.items():
            if group.get("name") == g and len(group["params"]) == 1:
                state = optimizer.state.get(group["params"][0])
                if state:
                    out[k] = (state["exp_avg"], state["exp_avg_sq"])
    return out


class DensifyResult:
    """The new tensors (``_xyz`` ... ``_rotation``, ``binding``, ``binding_counter``), ``moments`` {name: (exp_avg, exp_avg_sq)} of
    those that were given, ``src [n_out]`` int32 (the source row of every output row), ``kind [n_out]`` int32 (0 kept, 1 clone,
    2 split child) and the counts ``n_out``, ``n_cloned``, ``n_split`` (selected originals) and ``n_pruned`` (rows the last prune
    removed)."""

    def __init__(self, tensors, moments, binding, binding_counter, src, kind, counts):
        for k in PARAMS:
            setattr(self, k, tensors[k])
        self.moments = moments
        self.binding, self.binding_counter, self.src, self.kind = binding, binding_counter, src, kind
        self.n_out, self.n_cloned, self.n_split, self.n_pruned = counts

    def swap_into(self, optimizer, names=None):
        """What ``cat_tensors_to_optimizer`` and ``_prune_optimizer`` do to a torch.optim.Adam: each named group gets the new tensor
        as a new ``nn.Parameter`` and, where it held state, the new moments (copied for surviving originals, zero for new rows);
        ``step`` stays.  Groups that are not named (``verts``, ``cams``, ``shadow``) are left alone.  -> {parameter name: Parameter}"""
        names = GROUPS if names is None else names
        out = {}
        for group in optimizer.param_groups:
            for k, g in names.items():
                if group.get("name") != g:
                    continue
                if len(group["params"]) != 1:
                    raise RuntimeError(f"group {g}: expected one parameter")
                old = group["params"][0]
                new = torch.nn.Parameter(getattr(self, k).requires_grad_(True))
                state = optimizer.state.pop(old, None)
                if state:
                    if k not in self.moments:
                        raise RuntimeError(f"group {g} holds Adam moments that densify_and_prune was not given (moments=adam_moments(optimizer))")
                    state["exp_avg"], state["exp_avg_sq"] = self.moments[k]
                    optimizer.state[new] = state
                group["params"][0] = new
                setattr(self, k, new)
                out[k] = new
        return out


def densify_and_prune(_xyz, _features_dc, _features_rest, _opacity, _scaling, _rotation, binding, n_faces, face_scaling, stats, max_grad,
                      min_opacity, extent, max_screen_size, percent_dense, *, moments=None, noise=None, generator=None) -> DensifyResult:
    """scene/gaussian_model.py:508-522 for a bound model.  The raw parameters ``_xyz [n, 3]``, ``_features_dc [n, 1, 3]``,
    ``_features_rest [n, R, 3]`` (R >= 0), ``_opacity [n, 1]``, ``_scaling [n, 3]``, ``_rotation [n, 4]``; ``binding [n]`` int32,
    ``face_scaling [n_faces, 1]`` of the current mesh (``MeshFrames.face_scaling``); ``stats``: the DensifyStats, zero and of the new
    length afterwards; ``max_screen_size``: None or a number, which switches the world-size prune on; ``moments``: {parameter name:
    (exp_avg, exp_avg_sq)}, see ``adam_moments``; ``noise [n, 2, 3]``: standard normals, drawn with ``torch.randn`` from
    ``generator`` when not given.  One host synchronisation."""
    xyz = expect(_xyz.detach(), torch.float32, "_xyz", last=3)
    if xyz.dim() != 2:
        raise RuntimeError("_xyz: expected an [n, 3] tensor")
    n, dev = xyz.shape[0], xyz.device
    rest = expect(_features_rest.detach(), torch.float32, "_features_rest", last=3)
    if rest.dim() != 3 or rest.shape[0] != n:
        raise RuntimeError(f"_features_rest: expected shape ({n}, R, 3), got {tuple(rest.shape)}")
    tensors = {"_xyz": xyz, "_features_dc": expect(_features_dc.detach(), torch.float32, "_features_dc", shape=(n, 1, 3)), "_features_rest": rest,
               "_opacity": expect(_opacity.detach(), torch.float32, "_opacity", shape=(n, 1)),
               "_scaling": expect(_scaling.detach(), torch.float32, "_scaling", shape=(n, 3)),
               "_rotation": expect(_rotation.detach(), torch.float32, "_rotation", shape=(n, 4))}
    bind = expect(binding, torch.int32, "binding", shape=(n,))
    n_faces = int(n_faces)
    fs = expect(face_scaling.detach(), torch.float32, "face_scaling")
    if tuple(fs.shape) not in ((n_faces, 1), (n_faces,)):
        raise RuntimeError(f"face_scaling: expected shape {(n_faces, 1)}, got {tuple(fs.shape)}")
    if not isinstance(stats, DensifyStats) or stats.n != n:
        raise RuntimeError(f"stats: expected the DensifyStats of {n} Gaussians")
    moments = dict(moments or {})
    for k, pair in moments.items():
        if k not in tensors or len(pair) != 2:
            raise RuntimeError(f"moments: {k!r} is not a parameter with an (exp_avg, exp_avg_sq) pair")
        moments[k] = tuple(expect(m.detach(), torch.float32, f"moments[{k}]", shape=tensors[k].shape) for m in pair)
    if noise is None:
        noise = torch.randn(n, 2, 3, dtype=torch.float32, device=dev, generator=generator)
    noise = expect(noise, torch.float32, "noise", shape=(n, 2, 3))
    everything = list(tensors.values()) + [bind, fs, noise, stats.max_radii2D] + [m for pair in moments.values() for m in pair]
    if any(t.device != dev for t in everything):
        raise RuntimeError("densify_and_prune: the tensors must be on the same device")
    if 3 * n + 1 > 2 ** 31 - 1:
        raise RuntimeError(f"densify_and_prune: {n} Gaussians are more than the scan can index")
    lib = L.load()
    index = dev.index if dev.index is not None else torch.cuda.current_device()
    nbytes = C.c_int64(0)
    rc = lib.mpmhip_densify_scratch_bytes(index, n, n_faces, C.byref(nbytes))
    if rc != L.OK:
        raise L.MPMHipError(rc, "mpmhip_densify_scratch_bytes failed")
    scratch = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    counts = torch.empty(_N_COUNTS, dtype=torch.int32, device=dev)
    prune_big = 1 if max_screen_size else 0
    call("mpmhip_densify_plan", dev, n, n_faces, tensors["_scaling"].data_ptr(), tensors["_opacity"].data_ptr(), bind.data_ptr(), fs.data_ptr(),
         stats.xyz_gradient_accum.data_ptr(), stats.denom.data_ptr(), _f32(max_grad), _f32(float(percent_dense) * float(extent)),
         _f32(min_opacity), _f32(0.1 * float(extent)), prune_big, scratch.data_ptr(), nbytes.value, counts.data_ptr())
    n_out, n_cloned, n_split, n_pruned, error = counts.cpu().tolist()[:5]              # the one synchronisation
    if error:
        raise RuntimeError(f"binding: index out of range [0, {n_faces})")
    out = {k: torch.empty((n_out,) + tuple(t.shape[1:]), dtype=torch.float32, device=dev) for k, t in tensors.items()}
    out_moments = {k: tuple(torch.empty_like(out[k]) for _ in pair) for k, pair in moments.items()}
    src, kind, out_binding = (torch.empty(n_out, dtype=torch.int32, device=dev) for _ in range(3))
    counter = torch.empty(n_faces, dtype=torch.int32, device=dev)
    table = []                                                                          # (in, out, floats per row, mode)
    for k, t in tensors.items():
        width = int(np.prod(t.shape[1:]))
        if width == 0 or n_out == 0:                                                    # R = 0: rows of nothing; n = 0: no rows
            continue
        table.append((t, out[k], width, _MODE.get(k, 0)))
        table += [(m, o, width, _MOMENT) for m, o in zip(moments.get(k, ()), out_moments.get(k, ()))]
    assert len(table) <= _MAX_TENSORS
    k = len(table)
    ins, outs = (C.c_void_p * k)(*[t[0].data_ptr() for t in table]), (C.c_void_p * k)(*[t[1].data_ptr() for t in table])
    widths, modes = (C.c_int32 * k)(*[t[2] for t in table]), (C.c_int32 * k)(*[t[3] for t in table])
    call("mpmhip_densify_emit", dev, n, n_faces, n_out, xyz.data_ptr(), tensors["_scaling"].data_ptr(), tensors["_rotation"].data_ptr(),
         bind.data_ptr(), fs.data_ptr(), noise.data_ptr(), scratch.data_ptr(), nbytes.value, k, C.addressof(ins), C.addressof(outs),
         C.addressof(widths), C.addressof(modes), src.data_ptr(), kind.data_ptr(), out_binding.data_ptr(), counter.data_ptr())
    stats.reset(n_out)
    return DensifyResult(out, out_moments, out_binding, counter, src, kind, (n_out, n_cloned, n_split, n_pruned))


def reset_opacity(_opacity, optimizer=None, name="opacity"):
    """scene/gaussian_model.py:284-287 in one launch: log(x / (1 - x)) with x = min(sigmoid(_opacity), 0.01).  With an optimiser,
    ``replace_tensor_to_optimizer`` too: the group called ``name`` gets the result as a new ``nn.Parameter``, its moments are zeroed
    and ``step`` stays.  -> the new tensor (the new Parameter with an optimiser)"""
    opa = expect(_opacity.detach(), torch.float32, "_opacity")
    out = torch.empty_like(opa)
    call("mpmhip_reset_opacity", opa.device, opa.numel(), opa.data_ptr(), out.data_ptr())
    if optimizer is None:
        return out
    for group in optimizer.param_groups:
        if group.get("name") == name:
            new = torch.nn.Parameter(out.requires_grad_(True))
            state = optimizer.state.pop(group["params"][0], None)
            if state:
                state["exp_avg"], state["exp_avg_sq"] = torch.zeros_like(out), torch.zeros_like(out)
                optimizer.state[new] = state
            group["params"][0] = new
            return new
    raise RuntimeError(f"reset_opacity: the optimiser has no group called {name!r}")
