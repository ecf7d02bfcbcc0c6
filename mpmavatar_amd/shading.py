"""The colours handed to the render call of the appearance loop, on the device (train_appearance.py:120-123):

    shadow_map = shadow_net(ao_map)["shadow_map"]                                  # [1, 1, H, W], the caller's network
    shadow     = F.grid_sample(shadow_map, uv_coord, 'bilinear', align_corners=False).squeeze()[..., None][binding]
    colors     = shadow * convert_SH(get_features, cam, gaussians, get_xyz)        # clamp_min(eval_sh(...) + 0.5, 0)

as one launch forward (``mpmhip_shade_colors``) and one call backward (``mpmhip_shade_colors_backward``, csrc/shade.hip):

    sampler = ShadowSampler(gaussians.uv_coord, 256, 256)                          # once per mesh
    colors  = shaded_colors(_features_dc, _features_rest, active_sh_degree, means3D, campos,
                            binding=binding, shadow_map=shadow_map, sampler=sampler)
    render(..., override_color=colors)

With grad mode on the result carries a graph back to whichever of ``features_dc``, ``features_rest``, ``means3D`` and ``shadow_map``
require grad; ``uv_coord`` and ``campos`` are constants, as in the reference.  The backward is the exact derivative with every
discrete decision held fixed (the bilinear cell, a tap outside the map, the SH clamp with zero slope where it binds), fp32, no
atomics: the same input gives the same bits.  There is no double backward.  With grad mode off, or with nothing requiring grad,
the output carries no ``grad_fn``.  No CPU fallback: tensors must live on an MI355X.
"""
from __future__ import annotations

import torch

from . import _lib as L
from ._call import call, csr, expect, ptr, upstream, wants_grad
from .mesh_frames import _GaussianTable


def texel_table(uv, height, width):
    """uv [F, 2] float32 -> (texel_start [H * W + 1], texel_items) int32: the taps (4 * face + corner) inside the map that land on each
    texel, ascending within a texel.  The cell is shadow_taps' of csrc/shade_math.hpp: the same fp32 operations in the same order
    (that function is compiled without FMA contraction), here as torch ops."""
    n_f = uv.shape[0]
    W, H = float(width), float(height)
    ix, iy = ((uv[:, 0] + 1.0) * W - 1.0) / 2.0, ((uv[:, 1] + 1.0) * H - 1.0) / 2.0
    x0, y0 = torch.floor(ix), torch.floor(iy)
    xs, ys = torch.stack([x0, x0 + 1.0, x0, x0 + 1.0], 1), torch.stack([y0, y0, y0 + 1.0, y0 + 1.0], 1)      # nw ne sw se
    inside = (xs >= 0) & (xs <= W - 1) & (ys >= 0) & (ys <= H - 1)
    texel = (ys.clamp(0, H - 1).long() * width + xs.clamp(0, W - 1).long())[inside]     # row-major over (face, corner): ascending taps
    taps = torch.arange(4 * n_f, device=uv.device).reshape(n_f, 4)[inside]
    start, order = csr(texel, height * width, "texel")
    return start, taps[order.long()].to(torch.int32).contiguous()


class ShadowSampler:
    """Where each face samples the shadow map: the reference's ``uv_coord`` ([1, 1, F, 2] or [F, 2], in [-1, 1] with v flipped,
    scene/mesh_gaussian_model.py:109-111) for a map of ``height`` x ``width``, and the texel -> tap table of the backward pass
    (taps outside the map are dropped), built here once."""

    def __init__(self, uv_coord: torch.Tensor, height: int, width: int):
        uv = expect(uv_coord.reshape(-1, 2).contiguous(), torch.float32, "uv_coord", last=2)
        if height <= 0 or width <= 0 or height * width >= 2 ** 31 - 1:
            raise RuntimeError(f"ShadowSampler: bad map size {height} x {width}")
        if not bool(torch.isfinite(uv).all()):
            raise RuntimeError("ShadowSampler: uv_coord must be finite")
        L.load()                                 # a missing library is reported here, not at the first launch
        self.face_uv, self.height, self.width, self.n_faces = uv, int(height), int(width), uv.shape[0]
        self.texel_start, self.texel_items = texel_table(uv, self.height, self.width)


def _launch_forward(dc, rest, deg, means3D, campos, binding, smap, sampler, n):
    dev = means3D.device if means3D is not None else smap.device
    out = torch.empty(n, 3, dtype=torch.float32, device=dev)
    if n == 0:                                   # an empty tensor has no pointer to tell "no features" from "no Gaussians" by
        return out
    k = 0 if dc is None else 1 + rest.shape[1]
    call("mpmhip_shade_colors", dev, n, 0 if sampler is None else sampler.n_faces, ptr(binding), ptr(means3D), ptr(campos), deg, k, ptr(dc),
         ptr(rest) if k > 1 else None, ptr(smap), 0 if smap is None else sampler.height, 0 if smap is None else sampler.width,
         None if smap is None else sampler.face_uv.data_ptr(), out.data_ptr())
    return out


class _Shade(torch.autograd.Function):
    """(features_dc, features_rest, means3D, shadow_map [H, W]) -> colors [n, 3]: the forward launch with a backward.  ``table`` is the
    caller's face -> Gaussian table (_GaussianTable) and ``key`` the caller's binding tensor it is keyed on."""

    @staticmethod
    def forward(ctx, dc, rest, means3D, smap, campos, deg, binding, sampler, table, key, n):
        out = _launch_forward(dc, rest, deg, means3D, campos, binding, smap, sampler, n)
        ctx.deg, ctx.sampler, ctx.table, ctx.n = deg, sampler, table, n
        ctx.key = None if key is None else (key, key.data_ptr(), key._version)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(dc, rest, means3D, smap, campos, binding)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_colors):
        dc, rest, means3D, smap, campos, binding = ctx.saved_tensors
        g = upstream(g_colors)
        if g is None:
            return (None,) * 11
        n, sampler = ctx.n, ctx.sampler
        dev = g.device
        want_dc, want_rest, want_mean, want_map = ctx.needs_input_grad[:4]
        k = 0 if dc is None else 1 + rest.shape[1]
        d_dc = torch.empty_like(dc) if want_dc else None
        d_rest = torch.empty_like(rest) if want_rest else None
        d_mean = torch.empty_like(means3D) if want_mean else None
        d_map = scratch = start = items = None
        if n == 0 and not want_map:
            return (d_dc, d_rest, d_mean, None) + (None,) * 7
        if want_map:
            start, items = ctx.table.get(ctx.key, binding, sampler.n_faces)
            d_map = torch.empty_like(smap)
            scratch = torch.empty(n + sampler.n_faces, dtype=torch.float32, device=dev)
        call("mpmhip_shade_colors_backward", dev, n, 0 if sampler is None else sampler.n_faces, ptr(binding), ptr(means3D), ptr(campos),
             ctx.deg, k, ptr(dc), ptr(rest) if k > 1 else None, ptr(smap), 0 if smap is None else sampler.height,
             0 if smap is None else sampler.width, None if smap is None else sampler.face_uv.data_ptr(), g.data_ptr(), ptr(d_dc),
             ptr(d_rest) if k > 1 else None, ptr(d_mean), ptr(start), ptr(items),
             None if not want_map else sampler.texel_start.data_ptr(), None if not want_map else sampler.texel_items.data_ptr(),
             ptr(d_map), ptr(scratch))
        return (d_dc, d_rest, d_mean, d_map) + (None,) * 7


def shaded_colors(features_dc, features_rest, active_sh_degree, means3D, campos, *, binding=None, shadow_map=None, sampler=None,
                  gtable=None):
    """-> colors [n, 3] = shadow[binding] * clamp_min(eval_sh(active_sh_degree, features, normalize(means3D - campos)) + 0.5, 0).

    features_dc [n, 1, 3], features_rest [n, K - 1, 3]: the model's two tensors; both None gives the shadow alone on three channels
    (train_appearance.py:215-226).  shadow_map [H, W], [1, H, W] or [1, 1, H, W] with the ``sampler`` (ShadowSampler) of that size and
    ``binding`` [n]; None gives plain convert_SH (train_appearance.py:31-47).  ``gtable``: a _GaussianTable kept by the caller, so that
    the face -> Gaussian table of the backward pass is built once per binding."""
    if features_dc is None and shadow_map is None:
        raise RuntimeError("shaded_colors: give features, a shadow map, or both")
    dc = rest = mean = cam = smap = b = None
    deg = int(active_sh_degree)
    if features_dc is not None:
        dc = expect(features_dc, torch.float32, "features_dc", last=3)
        n = dc.shape[0]
        if features_rest is None:
            features_rest = dc.new_zeros(n, 0, 3)
        rest = expect(features_rest, torch.float32, "features_rest", last=3)
        if dc.dim() != 3 or dc.shape[1] != 1 or rest.dim() != 3 or rest.shape[0] != n:
            raise RuntimeError("shaded_colors: features_dc must be [n, 1, 3] and features_rest [n, K - 1, 3]")
        if not 0 <= deg <= 3 or 1 + rest.shape[1] < (deg + 1) ** 2:
            raise RuntimeError(f"shaded_colors: degree {deg} needs {(deg + 1) ** 2} coefficients, got {1 + rest.shape[1]}")
        mean = expect(means3D, torch.float32, "means3D", shape=(n, 3))
        cam = campos.detach().to(device=dc.device, dtype=torch.float32).reshape(3).contiguous()
    if shadow_map is not None:
        if sampler is None or binding is None:
            raise RuntimeError("shaded_colors: a shadow map needs its sampler and the binding")
        b = expect(binding.to(torch.int32).contiguous(), torch.int32, "binding")
        if features_dc is None:
            n = b.numel()
        if b.numel() != n:
            raise RuntimeError("shaded_colors: binding must have one entry per Gaussian")
        if sampler.face_uv.device != b.device:
            raise RuntimeError("shaded_colors: the sampler and the binding must be on the same device")
        if shadow_map.dim() not in (2, 3, 4) or tuple(shadow_map.shape[-2:]) != (sampler.height, sampler.width) or \
                shadow_map.numel() != sampler.height * sampler.width:
            raise RuntimeError(f"shaded_colors: shadow_map must be [{sampler.height}, {sampler.width}] with leading ones")
        smap = expect(shadow_map.reshape(sampler.height, sampler.width), torch.float32, "shadow_map")
    else:
        sampler = None
    if wants_grad(dc, rest, mean, smap):
        table = gtable if gtable is not None else _GaussianTable()
        return _Shade.apply(dc, rest, mean, smap, cam, deg, b, sampler, table, binding, n)
    return _launch_forward(dc, rest, deg, mean, cam, b, smap, sampler, n)
