"""The torch side of a call into libmpmhip.so, said once for the appearance chain (mesh_frames, render_inputs, geo_metrics,
image_loss, rasterizer) and the solver's one stateless launch: which device and stream a launch goes to, what a non-zero
return becomes, what a tensor argument must be, what an upstream gradient is turned into.  ``_lib.py`` stays free of torch.
"""
from __future__ import annotations

import torch

from . import _lib as L


def call_handle(name, *args):
    """``name(*args)`` of the library; a non-zero return raises.  For the mpmhip_raster_* functions, whose handle holds the
    device and stream."""
    rc = getattr(L.load(), name)(*args)
    if rc != L.OK:
        raise L.MPMHipError(rc, f"{name} failed")


def call(name, dev, *args):
    """``name(device, stream, *args)`` of a stateless entry point: the index of ``dev`` (the current
    device where it has none) and the current torch stream of that device."""
    index = dev.index if dev.index is not None else torch.cuda.current_device()
    call_handle(name, index, torch.cuda.current_stream(index).cuda_stream, *args)


def ptr(t):
    """None -> NULL.  An empty tensor keeps its pointer: the entry points accept a zero count with pointers set."""
    return None if t is None else t.data_ptr()


def expect(t, dtype, name, *, shape=None, last=None, rows=False, contiguous=True):
    """``t`` if it is a (contiguous) ``dtype`` tensor on the GPU of the given shape, else RuntimeError.  shape: the exact
    shape; last: the size of the last dimension; rows with last: a non-empty [n, last] matrix."""
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and (t.is_contiguous() or not contiguous)):
        raise RuntimeError(f"{name}: expected a {'contiguous ' if contiguous else ''}{dtype} tensor on the GPU")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    if last is not None and rows and (t.dim() != 2 or t.shape[-1] != last or t.shape[0] == 0):
        raise RuntimeError(f"{name}: expected a non-empty [n, {last}] tensor")
    if last is not None and (t.dim() < 1 or t.shape[-1] != last):
        raise RuntimeError(f"{name}: last dimension must be {last}")
    return t


def csr(keys, n_keys, what):
    """key -> items table on the device: (start [n_keys + 1] int32, items int32 in ascending item index within a key).  Plumbing for
    the serial reductions of the backward passes, built with torch ops; the bounds of ``keys`` are checked here, once."""
    k = keys.reshape(-1).long()
    counts = torch.bincount(k, minlength=n_keys)          # raises on a negative key
    if counts.numel() != n_keys:
        raise RuntimeError(f"{what}: index {counts.numel() - 1} out of range [0, {n_keys})")
    start = torch.zeros(n_keys + 1, dtype=torch.int32, device=keys.device)
    start[1:] = torch.cumsum(counts, 0)
    return start, torch.sort(k, stable=True).indices.to(torch.int32)


def wants_grad(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def upstream(g, shape=None):
    """An upstream gradient as a backward launch reads it: None stays None (NULL = zeros), otherwise fp32, expanded to
    ``shape`` if given, contiguous."""
    if g is None:
        return None
    g = g.to(torch.float32)
    return (g if shape is None else g.expand(shape)).contiguous()
