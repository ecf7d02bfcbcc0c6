"""Gaussian rasteriser on the GPU, forward and backward, behind the names of the reference's ``diff_gauss`` extension
(/root/reference/gaussian_renderer/__init__.py:14,36-103): the last step of the chain solver -> ``MeshFrames`` ->
``BoundGaussians.render_inputs`` -> image,

    settings = GaussianRasterizationSettings(image_height=h, image_width=w, tanfovx=..., tanfovy=..., bg=bg_color,
                                             scale_modifier=1.0, viewmatrix=cam.world_view_transform,
                                             projmatrix=cam.full_proj_transform, sh_degree=pc.active_sh_degree,
                                             campos=cam.camera_center, prefiltered=False, debug=False)
    image, _, _, mask, radii, _ = GaussianRasterizer(raster_settings=settings)(**gaussians.render_inputs(frames, ...))

over the HIP pipelines of ``csrc/raster.hip`` (forward) and ``csrc/raster_backward.hip`` (backward).  With
``mpmavatar_amd/compat`` on PYTHONPATH the reference's ``from diff_gauss import GaussianRasterizationSettings,
GaussianRasterizer`` resolves to these two names.

FORWARD AND BACKWARD.  With grad mode on and at least one of ``means3D``, ``opacities``, ``shs``, ``colors_precomp``,
``scales``, ``rotations``, ``cov3Ds_precomp`` requiring grad, ``image`` and ``alpha`` carry a graph, and ``loss.backward()``
-- the render call and loss of ``train_appearance.py`` (:123-155: image * mask, L1 + SSIM + LPIPS) -- fills the gradients of
those inputs and of ``means2D`` (``viewspace_point_tensor.grad`` of train_appearance.py:245-253; the published convention:
dL/dpx * W/2, dL/dpy * H/2, 0 -- the gradient with respect to an additive NDC offset of the pixel centre; the tensor's value
stays ignored).  ``means2D`` requiring grad ALONE builds no graph: that is how the eval loop
(train_material_params.py:857-872) and the demo (run_demo.py:540-604) call it, and they get exactly the forward-only call:
same kernels, nothing more allocated.  ``radii`` is non-differentiable; the camera tensors, ``bg`` and ``scale_modifier``
get no gradient; there is no double backward.

The gradient is the exact derivative of the forward function as computed here (``csrc/raster_grad_math.hpp``), every
discrete decision held fixed: culling, radius and tile rectangle, depth order, power > 0, alpha < 1/255, the T < 1e-4
finish.  The clamps differentiate as clamps, zero slope where they bind: alpha = min(0.99, .), the +-1.3 tanfov clamp inside
the Jacobian, max(0, sh + 0.5).  ONE DEVIATION, unconfirmed: the CUDA original is remembered to let the gradient through a
bound 0.99 alpha clamp; its source is not at hand to check.  Here a bound clamp returns zero to the opacity and the
geometry, because that is the derivative of what the forward pass computes.  No floating-point atomics: two backward
passes over the same inputs return the same bits.

A frame that will be differentiated keeps its own copy of the pipeline's state (packed records, sorted indices, tile ranges,
per-pixel T and stopping position) in a tensor held by the autograd node: the scratch is shared by every rasteriser on a
device and stream, and the next forward overwrites it.  What is NOT differentiable: ``BoundGaussians.render_inputs`` is a
forward-only launch, so gradients stop at its outputs; densification itself is the caller's.

EXTRA ATTRIBUTE CHANNELS.  ``extra_attrs`` [N, E] (contiguous float32 on the same device, 1 <= E <= 8) is the table the 4D-DRESS
tracking script hands over (preprocess/train_mesh_lbs_4ddress.py:260-277: ``variables['cloth_mask']``, upper and lower garment); the
sixth value of the result is then [E, H, W], ``extra_e = sum_k a_ke alpha_k T_k`` with the alpha, T and finishing rule of the colour
and NO background term (:299 reads it, :306 compares it with the data's garment mask).  UNCONFIRMED against the CUDA original, whose
source is not at hand.  It is one more walk over the tile lists that the colour pass has sorted (``csrc/raster_extra.hip``), up to
where each pixel's colour walk stopped, so such a frame always runs the training flavour of the colour pass; its state is saved only
when a graph is built.  A graph is built when ``extra_attrs`` or any input other than ``means2D`` requires grad; the extras' share
of the geometry and opacity gradients adds to that of image and alpha, and the table gets ``dL/da_ke = g_e alpha_k T_k``.  When slot
5 is not used by the loss its gradient arrives as None and the backward pass is exactly that of a call without extras, bit for bit.
Without ``extra_attrs`` nothing changes: the same kernels and entry points, ``None`` in slot 5.

Each call blocks the host once (the pipeline reads one count back to size its sort, csrc/raster.hip).  The three floats of
``bg`` are read from the device the first time a given tensor is seen and kept until it is modified in place or freed, so
a loop that renders against one background tensor, as the reference's does, adds no second wait.  No CPU fallback: tensors
must live on an MI355X.
"""
from __future__ import annotations

import ctypes as C
import math
import weakref
from typing import NamedTuple

import torch

from . import _lib as L
from ._call import call_handle, expect, ptr, upstream


class GaussianRasterizationSettings(NamedTuple):  # fields and order of gaussian_renderer/__init__.py:36-49
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


class _Handle:
    """One mpmhip_raster per (device, stream): the scratch is reused from frame to frame.  The handle keeps the
    torch.cuda.Stream object it was made for: torch's own streams come from a pool that is never destroyed, and for an
    ExternalStream the wrapper does not own the hipStream_t -- whoever destroys such a stream must not render on a new one
    at the same address (``GaussianRasterizer(..., private_scratch=True)`` is the way out)."""

    def __init__(self, device_index, stream):
        self.lib = L.load()
        self.ptr = L.vp()
        self.stream = stream
        self.last_user = None     # weak reference to the rasteriser whose frame the handle's counts describe
        call_handle("mpmhip_raster_create", device_index, stream.cuda_stream, C.byref(self.ptr))
        weakref.finalize(self, self.lib.mpmhip_raster_destroy, self.ptr)


MAX_EXTRA_ATTRS = 8   # channels of extra_attrs in one call (rast::EXTRA_MAX of csrc/raster_extra_math.hpp)
_SHARED = {}
_BG = {}    # id(bg tensor) -> (weak reference, version counter, three floats)


def _bg_floats(bg):
    """The background colour as three host floats; one device-to-host copy per tensor and version, not per frame."""
    hit = _BG.get(id(bg))
    if hit is not None and hit[0]() is bg and hit[1] == bg._version:
        return hit[2]
    vals = tuple(float(v) for v in bg.detach().reshape(3).tolist())
    key = id(bg)
    _BG[key] = (weakref.ref(bg, lambda _, key=key: _BG.pop(key, None)), bg._version, vals)
    return vals


def look_at_camera(eye, target, fov_deg, device, znear=0.01, zfar=100.0):
    """(world_view_transform, full_proj_transform, camera_center, tan(fov / 2)) of a square-pixel camera at `eye` looking
    at `target`, world +y up, in the reference's layout (scene/cameras.py:26-39: transposed, row vectors from the left;
    +z forward, +y down in the image).  For the example and the benchmark, which have no dataset camera."""
    import numpy as np
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(fwd, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    R = np.stack([right, down, fwd])                    # world -> camera
    w2c = np.eye(4)
    w2c[:3, :3], w2c[:3, 3] = R, -R @ eye
    t = math.tan(math.radians(fov_deg) / 2)
    P = np.zeros((4, 4))
    P[0, 0] = P[1, 1] = 1.0 / t
    P[2, 2], P[2, 3], P[3, 2] = zfar / (zfar - znear), -(zfar * znear) / (zfar - znear), 1.0
    f32 = lambda a: torch.tensor(np.asarray(a, np.float32), device=device)
    return f32(w2c.T), f32(w2c.T @ P.T), f32(eye), t


class _Frame:
    """What one differentiable call keeps besides its input tensors: the settings struct with the camera tensors it points
    to, the handle, and the saved state of the pipeline (a uint8 tensor this frame owns)."""
    __slots__ = ("cs", "keep", "hd", "n", "n_sh", "saved", "n_entries", "h", "w")


def _ptr(t):
    """the rasteriser's own rule on top of ptr: an empty tensor goes down as NULL too"""
    return None if t is not None and t.numel() == 0 else ptr(t)


def _launch_forward(hd, cs, n, n_sh, tensors, grad):
    """One frame: allocates image [3, H, W], alpha [1, H, W] and radii [n] and runs mpmhip_raster_forward, or with ``grad``
    mpmhip_raster_forward_grad.  tensors = (means3D, shs, colors_precomp, opacities, scales, rotations, cov3Ds_precomp)."""
    dev, h, w = tensors[0].device, cs.image_height, cs.image_width
    image = torch.empty(3, h, w, dtype=torch.float32, device=dev)
    alpha = torch.empty(1, h, w, dtype=torch.float32, device=dev)
    radii = torch.empty(n, dtype=torch.int32, device=dev)
    means3D, shs, colors_precomp, opacities, scales, rotations, cov3Ds_precomp = map(_ptr, tensors)
    call_handle("mpmhip_raster_forward_grad" if grad else "mpmhip_raster_forward", hd.ptr, C.byref(cs), n, means3D, shs, n_sh,
                colors_precomp, opacities, scales, rotations, cov3Ds_precomp, image.data_ptr(), alpha.data_ptr(), _ptr(radii))
    return image, alpha, radii


def _launch_extra(hd, cs, n, extra):
    """The extras of the frame that _launch_forward(..., grad=True) has just rendered on ``hd``: mpmhip_raster_extra_forward
    -> [E, H, W].  It reads the frame's sorted lists and stopping positions out of the handle, so nothing may render in between."""
    out = torch.empty(extra.shape[1], cs.image_height, cs.image_width, dtype=torch.float32, device=extra.device)
    call_handle("mpmhip_raster_extra_forward", hd.ptr, C.byref(cs), n, _ptr(extra), extra.shape[1], out.data_ptr())
    return out


def _save_frame(fr, dev):
    """copy the state of the handle's newest frame into a tensor that ``fr`` owns"""
    size, entries = C.c_int64(), C.c_int64()
    call_handle("mpmhip_raster_saved_bytes", fr.hd.ptr, C.byref(size), C.byref(entries))
    fr.saved = torch.empty(size.value, dtype=torch.uint8, device=dev)
    fr.n_entries = entries.value
    call_handle("mpmhip_raster_save", fr.hd.ptr, fr.saved.data_ptr(), size.value)


def _launch_backward(ctx, g_image, g_alpha, extra=None, g_extra=None):
    """mpmhip_raster_backward over the frame of ``ctx``, or with ``g_extra`` mpmhip_raster_backward_extra -> the gradients in the
    order of the autograd inputs behind ``fr``, and d_extra (None without ``g_extra``)"""
    fr = ctx.fr
    means3D, opacities, shs, colors_precomp, scales, rotations, cov3Ds_precomp = ctx.saved_tensors[:7]
    hd, dev, n = fr.hd, means3D.device, fr.n
    g_image, g_alpha = upstream(g_image, (3, fr.h, fr.w)), upstream(g_alpha, (1, fr.h, fr.w))
    like = lambda t: None if t is None else torch.empty_like(t)
    d_means3D, d_means2D, d_opac = torch.empty_like(means3D), torch.empty(n, 3, dtype=torch.float32, device=dev), torch.empty_like(opacities)
    d_shs, d_col, d_scales, d_rots, d_cov = like(shs), like(colors_precomp), like(scales), like(rotations), like(cov3Ds_precomp)
    p = _ptr
    args = (hd.ptr, C.byref(fr.cs), n, p(means3D), p(shs), fr.n_sh, p(colors_precomp), p(opacities), p(scales), p(rotations),
            p(cov3Ds_precomp), fr.saved.data_ptr(), fr.saved.numel(), fr.n_entries, p(g_image), p(g_alpha), p(d_means3D), p(d_means2D),
            p(d_shs), p(d_col), p(d_opac), p(d_scales), p(d_rots), p(d_cov))
    d_extra = None
    if g_extra is None:
        call_handle("mpmhip_raster_backward", *args)
    else:
        g_extra, d_extra = upstream(g_extra, (extra.shape[1], fr.h, fr.w)), torch.empty_like(extra)
        call_handle("mpmhip_raster_backward_extra", *args, p(extra), extra.shape[1], p(g_extra), p(d_extra))
    if ctx.means2D_shape is None or not ctx.needs_input_grad[2]:
        d_means2D = None
    elif ctx.means2D_shape != (n, 3):
        raise RuntimeError(f"means2D: expected shape {(n, 3)} to receive its gradient, got {ctx.means2D_shape}")
    return (None, d_means3D, d_means2D, d_opac, d_shs, d_col, d_scales, d_rots, d_cov), d_extra


class _Rasterize(torch.autograd.Function):
    """forward: mpmhip_raster_forward_grad + mpmhip_raster_save; backward: mpmhip_raster_backward"""

    @staticmethod
    def forward(ctx, fr, means3D, means2D, opacities, shs, colors_precomp, scales, rotations, cov3Ds_precomp):
        hd, tensors = fr.hd, (means3D, shs, colors_precomp, opacities, scales, rotations, cov3Ds_precomp)
        image, alpha, radii = _launch_forward(hd, fr.cs, fr.n, fr.n_sh, tensors, True)
        _save_frame(fr, means3D.device)
        ctx.fr = fr
        ctx.means2D_shape = None if means2D is None else tuple(means2D.shape)
        ctx.save_for_backward(means3D, opacities, shs, colors_precomp, scales, rotations, cov3Ds_precomp)
        ctx.mark_non_differentiable(radii)
        ctx.set_materialize_grads(False)       # an unused output's gradient arrives as None and goes down as NULL = zeros
        return image, alpha, radii

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_image, g_alpha, _g_radii):
        return _launch_backward(ctx, g_image, g_alpha)[0]


class _RasterizeExtra(torch.autograd.Function):
    """_Rasterize with ``extra_attrs``: forward adds mpmhip_raster_extra_forward between the render and the save; backward is
    mpmhip_raster_backward_extra, or, when the extras' gradient arrives as None (slot 5 unused), exactly _Rasterize's."""

    @staticmethod
    def forward(ctx, fr, means3D, means2D, opacities, shs, colors_precomp, scales, rotations, cov3Ds_precomp, extra_attrs):
        hd, tensors = fr.hd, (means3D, shs, colors_precomp, opacities, scales, rotations, cov3Ds_precomp)
        image, alpha, radii = _launch_forward(hd, fr.cs, fr.n, fr.n_sh, tensors, True)
        extra = _launch_extra(hd, fr.cs, fr.n, extra_attrs)
        _save_frame(fr, means3D.device)
        ctx.fr = fr
        ctx.means2D_shape = None if means2D is None else tuple(means2D.shape)
        ctx.save_for_backward(means3D, opacities, shs, colors_precomp, scales, rotations, cov3Ds_precomp, extra_attrs)
        ctx.mark_non_differentiable(radii)
        ctx.set_materialize_grads(False)
        return image, alpha, radii, extra

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_image, g_alpha, _g_radii, g_extra):
        grads, d_extra = _launch_backward(ctx, g_image, g_alpha, ctx.saved_tensors[7], g_extra)
        return grads + (d_extra,)


class GaussianRasterizer:
    """``GaussianRasterizer(raster_settings)(means3D=, means2D=, shs=, colors_precomp=, opacities=, scales=, rotations=,
    cov3Ds_precomp=, extra_attrs=)`` -> ``(image [3, H, W], None, None, alpha [1, H, W], radii [N] int32, extra [E, H, W] or None)``:
    the 6-tuple of the reference's call, of which it reads slots 0, 3 and 4 (gaussian_renderer/__init__.py:95) and the 4D-DRESS
    tracking script slot 5 as well (train_mesh_lbs_4ddress.py:299).  image, alpha and extra carry a graph when an input other than
    means2D requires grad (module docstring)."""

    def __init__(self, raster_settings: GaussianRasterizationSettings, private_scratch: bool = False):
        """The reference builds a new rasteriser for every frame (gaussian_renderer/__init__.py:51), so the scratch is shared
        by all instances (one handle per device and stream).  private_scratch=True gives this instance handles of its own."""
        self.raster_settings = raster_settings
        self._handles = {} if private_scratch else _SHARED
        self._last = None

    def _handle(self, dev):
        index = dev.index if dev.index is not None else torch.cuda.current_device()
        stream = torch.cuda.current_stream(index)
        key = (index, stream.cuda_stream)
        if key not in self._handles:
            self._handles[key] = _Handle(index, stream)
        return self._handles[key]

    def stats(self):
        """{"n_entries", "max_tile_entries", "n_visible", "scratch_bytes"} of this instance's newest call (synchronises).
        The counts live in the handle, which other instances share: asking after another instance has rendered on the same
        device and stream raises instead of reporting that one's frame."""
        if self._last is None:
            raise RuntimeError("nothing has been rendered yet")
        if self._last.last_user is None or self._last.last_user() is not self:
            raise RuntimeError("another rasteriser has rendered on this device and stream since: its counts replaced these")
        st = L.RasterStats()
        call_handle("mpmhip_raster_stats", self._last.ptr, C.byref(st))
        return {k: int(getattr(st, k)) for k, _ in L.RasterStats._fields_}

    def forward(self, means3D, means2D=None, opacities=None, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3Ds_precomp=None, extra_attrs=None):
        s = self.raster_settings
        if (shs is None) == (colors_precomp is None):
            raise RuntimeError("Please provide exactly one of either SHs or precomputed colors!")
        if (scales is None) != (rotations is None) or (scales is None) == (cov3Ds_precomp is None):
            raise RuntimeError("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")
        if opacities is None:
            raise RuntimeError("opacities: expected a tensor")
        h, w = int(s.image_height), int(s.image_width)
        if h <= 0 or w <= 0:
            raise RuntimeError("image_height and image_width must be positive")
        for name, t in (("means3D", means3D), ("opacities", opacities), ("shs", shs), ("colors_precomp", colors_precomp),
                        ("scales", scales), ("rotations", rotations), ("cov3Ds_precomp", cov3Ds_precomp)):
            if t is not None and not isinstance(t, torch.Tensor):
                raise RuntimeError(f"{name}: expected a tensor")
        given = dict(means3D=means3D, opacities=opacities, shs=shs, colors_precomp=colors_precomp, scales=scales, rotations=rotations,
                     cov3Ds_precomp=cov3Ds_precomp)
        # means2D requiring grad alone builds no graph: the eval loop passes it so and reads no gradient
        graph = torch.is_grad_enabled() and (any(t is not None and t.requires_grad for t in given.values())
                                             or (isinstance(extra_attrs, torch.Tensor) and extra_attrs.requires_grad))
        with torch.no_grad():
            m = expect(means3D.detach(), torch.float32, "means3D")
            if m.dim() != 2 or m.shape[1] != 3:
                raise RuntimeError(f"means3D: expected shape (n, 3), got {tuple(m.shape)}")
            n, dev = m.shape[0], m.device
            same = lambda t, name, shape: expect(t.detach() if isinstance(t, torch.Tensor) else t, torch.float32, name, shape=shape)
            op = same(opacities, "opacities", (n, 1)) if opacities.dim() == 2 else same(opacities, "opacities", (n,))
            n_sh, deg = 0, int(s.sh_degree)
            if shs is not None:
                if not 0 <= deg <= 3:
                    raise RuntimeError("sh_degree must be 0, 1, 2 or 3")
                if shs.dim() != 3 or shs.shape[1] < (deg + 1) ** 2:
                    raise RuntimeError(f"shs: expected shape (n, >= {(deg + 1) ** 2}, 3) for sh_degree {deg}")
                n_sh = shs.shape[1]
                shs = same(shs, "shs", (n, n_sh, 3))
            else:
                colors_precomp = same(colors_precomp, "colors_precomp", (n, 3))
            if scales is not None:
                scales, rotations = same(scales, "scales", (n, 3)), same(rotations, "rotations", (n, 4))
            else:
                cov3Ds_precomp = same(cov3Ds_precomp, "cov3Ds_precomp", (n, 6))
            # the reference's world_view_transform is a transposed view (scene/cameras.py:26): the three small camera
            # tensors are made contiguous here instead of being refused
            small = lambda t, name, shape: same(t.contiguous() if isinstance(t, torch.Tensor) else t, name, shape)
            view, proj = small(s.viewmatrix, "viewmatrix", (4, 4)), small(s.projmatrix, "projmatrix", (4, 4))
            campos, bg = small(s.campos, "campos", (3,)), s.bg
            if not (isinstance(bg, torch.Tensor) and bg.numel() == 3):
                raise RuntimeError("bg: expected a tensor of 3 values")
            extra = None
            if extra_attrs is not None:
                extra = expect(extra_attrs.detach() if isinstance(extra_attrs, torch.Tensor) else extra_attrs, torch.float32, "extra_attrs")
                if extra.dim() != 2 or extra.shape[0] != n or not 1 <= extra.shape[1] <= MAX_EXTRA_ATTRS:
                    raise RuntimeError(f"extra_attrs: expected shape ({n}, E) with 1 <= E <= {MAX_EXTRA_ATTRS}, got {tuple(extra.shape)}")
            for name, t in (("opacities", op), ("shs", shs), ("colors_precomp", colors_precomp), ("scales", scales),
                            ("rotations", rotations), ("cov3Ds_precomp", cov3Ds_precomp), ("extra_attrs", extra), ("viewmatrix", view),
                            ("projmatrix", proj), ("campos", campos)):
                if t is not None and t.device != dev:
                    raise RuntimeError(f"{name}: expected a tensor on {dev}")
            bg3 = _bg_floats(bg)
            cs = L.RasterSettings(h, w, float(s.tanfovx), float(s.tanfovy), L.f3(*bg3), float(s.scale_modifier), deg,
                                  view.data_ptr(), proj.data_ptr(), campos.data_ptr())
            hd = self._handle(dev)
            if not graph:
                # a frame with extras records where every pixel stopped (the training flavour): the extra walk ends there
                image, alpha, radii = _launch_forward(hd, cs, n, n_sh, (m, shs, colors_precomp, op, scales, rotations, cov3Ds_precomp),
                                                      extra is not None)
                blended = None if extra is None else _launch_extra(hd, cs, n, extra)
                self._last, hd.last_user = hd, weakref.ref(self)
                return image, None, None, alpha, radii, blended
        # the validated values above are detached views of these: the same memory, now with the graph's leaves attached
        fr = _Frame()
        fr.cs, fr.keep, fr.hd, fr.n, fr.n_sh, fr.h, fr.w = cs, (view, proj, campos), hd, n, n_sh, h, w
        m2 = means2D if isinstance(means2D, torch.Tensor) and means2D.requires_grad else None
        leaves = (fr, given["means3D"], m2, given["opacities"], given["shs"], given["colors_precomp"], given["scales"], given["rotations"],
                  given["cov3Ds_precomp"])
        if extra_attrs is None:
            (image, alpha, radii), blended = _Rasterize.apply(*leaves), None
        else:
            image, alpha, radii, blended = _RasterizeExtra.apply(*leaves, extra_attrs)
        self._last, hd.last_user = hd, weakref.ref(self)
        return image, None, None, alpha, radii, blended

    __call__ = forward
