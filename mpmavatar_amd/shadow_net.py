"""The shadow network of the appearance loop on the device (scene/shadow.py:14-181; train_appearance.py:120 and :201):

    shadow_net = ShadowUNet(ao_mean=ao_mean, interp_mode="bilinear", biases=False, uv_size=256, shadow_size=256, n_dims=4)
    shadow_map = shadow_net(ao_map)["shadow_map"]                                   # [N, 1, U, U]

with the reference's constructor arguments, parameter names, shapes and ``named_parameters()`` order (per convolution ``bias``,
``weight_g``, ``weight_v``; ``enc_layers.{i}.0``, ``dec_layers.{j}.0``, ``shadow_pred``; the buffer ``ao_mean``), so that a state dict
moves between the two classes in either direction and ``shadow_net.parameters()`` goes into ``appearance_param_groups`` unchanged.
The forward pass is ``mpmhip_shadow_forward`` (10 launches, 11 where uv_size != shadow_size), the backward pass
``mpmhip_shadow_backward`` (12 launches, csrc/shadow.hip): fp32, no atomics, the same input gives the same bits.  There is no double
backward.  With grad mode off, or with nothing requiring grad, the outputs carry no ``grad_fn`` and nothing is kept.  ``ao_map`` and
``ao_mean`` are constants, as in the reference.  No CPU fallback: tensors must live on an MI355X.

Supported: n_dims 4 or 8, shadow_size >= 8, any uv_size and batch, biases True and False, interp_mode "bilinear", trainable_mean False.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib as L
from ._call import call, expect, upstream, wants_grad

LAYERS = 9


def _channels(c, layer):
    """(cin, cout) of layer 0..3 encoder, 4..7 decoder, 8 head"""
    return (1 if layer == 0 else 2 * c if 5 <= layer <= 7 else c), (1 if layer == 8 else c)


def _sizes(shadow_size, uv_size, n_dims, n=1, in_h=1, in_w=1):
    d = L.ShadowDesc()
    d.n, d.in_h, d.in_w, d.shadow_size, d.uv_size, d.n_dims = n, in_h, in_w, shadow_size, uv_size, n_dims
    return d


def resample_tables(in_h, in_w, shadow_size, uv_size, n_dims=4):
    """-> (the table blob of csrc/shadow_math.hpp as int32 words, workspace bytes for a batch of one).  Host arithmetic of the
    library: needs no device."""
    lib, d = L.load(), _sizes(shadow_size, uv_size, n_dims, 1, in_h, in_w)
    ws, tb = C.c_int64(0), C.c_int64(0)
    rc = lib.mpmhip_shadow_workspace_bytes(0, None, C.byref(d), C.byref(ws), C.byref(tb), None)
    if rc not in (L.OK, L.ERR_NO_DEVICE):
        raise L.MPMHipError(rc, "mpmhip_shadow_workspace_bytes failed")
    words = np.zeros(tb.value // 4, np.int32)
    lib.mpmhip_shadow_workspace_bytes(0, None, C.byref(d), C.byref(ws), C.byref(tb), words.ctypes.data_as(C.c_void_p))
    return words, ws.value


class _ConvWN(torch.nn.Module):
    """The parameters of one weight-normalised convolution, registered in the reference's order: bias, weight_g, weight_v."""

    def __init__(self, cin, cout, bias_shape):
        super().__init__()
        v = torch.empty(cout, cin, 3, 3)
        torch.nn.init.kaiming_uniform_(v, a=math.sqrt(5))        # what the reference's weight_v holds after its constructor
        self.bias = torch.nn.Parameter(torch.zeros(bias_shape))
        self.weight_g = torch.nn.Parameter(v.norm().reshape(1, 1, 1, 1).repeat(cout, 1, 1, 1))
        self.weight_v = torch.nn.Parameter(v)

    def forward(self, x):
        raise RuntimeError("ShadowUNet runs as one fused call; its layers are not callable on their own")


class _Shadow(torch.autograd.Function):
    """(ao [N, h, w], the 27 parameters) -> (shadow_map, shadow_map_lowres); ``ao_out`` is filled on the way where given."""

    @staticmethod
    def forward(ctx, net, ao, ao_out, *params):
        smap, low, ws = net._launch(ao, ao_out, params)
        ctx.net, ctx.ws = net, ws
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(ao, low, *params)
        return smap, low

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_map, g_low):
        ao, low, *params = ctx.saved_tensors
        g_map, g_low = upstream(g_map), upstream(g_low)
        wanted = ctx.needs_input_grad[3:]
        if (g_map is None and g_low is None) or not any(wanted):
            return (None,) * (3 + len(params))
        grads = [torch.empty_like(p) if w else None for p, w in zip(params, wanted)]
        net = ctx.net
        d = net._desc(ao, params, grads)
        call("mpmhip_shadow_backward", ao.device, C.byref(d), ao.data_ptr(), low.data_ptr(), None if g_map is None else g_map.data_ptr(),
             None if g_low is None else g_low.data_ptr(), ctx.ws.data_ptr(), ctx.ws.numel() * 4)
        return (None, None, None) + tuple(grads)


class ShadowUNet(torch.nn.Module):
    def __init__(self, uv_size, ao_mean, shadow_size, lrelu_slope=0.2, beta=1.0, n_dims=64, interp_mode="bilinear", biases=True,
                 trainable_mean=False):
        super().__init__()
        if n_dims not in (4, 8):
            raise ValueError(f"ShadowUNet: n_dims must be 4 or 8, got {n_dims}")
        if int(shadow_size) != shadow_size or not 8 <= shadow_size <= 8192:
            raise ValueError(f"ShadowUNet: shadow_size must be an integer in 8 .. 8192, got {shadow_size}")
        if int(uv_size) != uv_size or not 1 <= uv_size <= 8192:
            raise ValueError(f"ShadowUNet: uv_size must be an integer in 1 .. 8192, got {uv_size}")
        if interp_mode != "bilinear":
            raise ValueError(f"ShadowUNet: interp_mode must be 'bilinear', got {interp_mode!r}")
        if trainable_mean:
            raise ValueError("ShadowUNet: trainable_mean must be False (ao_mean is a constant here)")
        if not (math.isfinite(lrelu_slope) and lrelu_slope >= 0 and math.isfinite(beta)):
            raise ValueError(f"ShadowUNet: lrelu_slope must be finite and >= 0 and beta finite, got {lrelu_slope}, {beta}")
        self.uv_size, self.shadow_size, self.n_dims, self.biases = int(uv_size), int(shadow_size), int(n_dims), bool(biases)
        self.lrelu_slope, self.beta, self.interp_mode = float(lrelu_slope), float(beta), interp_mode
        s = self.shadow_size
        mean = torch.as_tensor(ao_mean, dtype=torch.float32)
        if mean.dim() != 3 or mean.shape[0] != 1:
            raise ValueError(f"ShadowUNet: ao_mean must be [1, h, w], got {tuple(mean.shape)}")
        self.register_buffer("ao_mean", F.interpolate(mean[None], size=(s, s))[0].contiguous())
        self.sizes = [s // 2 ** i for i in range(4)]
        self.enc_layers, self.dec_layers = torch.nn.ModuleList(), torch.nn.ModuleList()
        for layer in range(8):
            cin, cout = _channels(self.n_dims, layer)
            size = self.sizes[layer] if layer < 4 else self.sizes[7 - layer]
            (self.enc_layers if layer < 4 else self.dec_layers).append(torch.nn.Sequential(_ConvWN(cin, cout, (cout, size, size))))
        self.shadow_pred = _ConvWN(self.n_dims, 1, (1, s, s) if self.biases else (1,))
        L.load()                                 # a missing library is reported here, not at the first launch
        self._tables, self._ws_bytes = {}, {}

    # ---- the launches ------------------------------------------------------------------------------------------------------------

    def _params(self):
        convs = [seq[0] for seq in self.enc_layers] + [seq[0] for seq in self.dec_layers] + [self.shadow_pred]
        return [p for conv in convs for p in (conv.bias, conv.weight_g, conv.weight_v)]

    def _table(self, in_h, in_w, dev):
        key = (in_h, in_w, str(dev))
        if key not in self._tables:
            words, _ = resample_tables(in_h, in_w, self.shadow_size, self.uv_size, self.n_dims)
            self._tables[key] = torch.from_numpy(words).to(dev)
        return self._tables[key]

    def _workspace(self, n, dev):
        if n not in self._ws_bytes:
            d = _sizes(self.shadow_size, self.uv_size, self.n_dims, n)
            ws, tb = C.c_int64(0), C.c_int64(0)
            call("mpmhip_shadow_workspace_bytes", dev, C.byref(d), C.byref(ws), C.byref(tb), None)
            self._ws_bytes[n] = ws.value
        return torch.empty(self._ws_bytes[n] // 4, dtype=torch.float32, device=dev)

    def _desc(self, ao, params, grads=None):
        n, in_h, in_w = ao.shape
        d = _sizes(self.shadow_size, self.uv_size, self.n_dims, n, in_h, in_w)
        d.untied_head_bias, d.lrelu_slope, d.beta = int(self.biases), self.lrelu_slope, self.beta
        d.ao_mean, d.tables = self.ao_mean.data_ptr(), self._table(in_h, in_w, ao.device).data_ptr()
        for layer in range(LAYERS):
            d.bias[layer], d.weight_g[layer], d.weight_v[layer] = (p.data_ptr() for p in params[3 * layer:3 * layer + 3])
            if grads is not None:
                d.d_bias[layer], d.d_weight_g[layer], d.d_weight_v[layer] = (None if g is None else g.data_ptr()
                                                                            for g in grads[3 * layer:3 * layer + 3])
        return d

    def _launch(self, ao, ao_out, params):
        n, dev, s, u = ao.shape[0], ao.device, self.shadow_size, self.uv_size
        ws = self._workspace(n, dev)
        low = torch.empty(n, 1, s, s, dtype=torch.float32, device=dev)
        smap = torch.empty(n, 1, u, u, dtype=torch.float32, device=dev)
        d = self._desc(ao, params)
        call("mpmhip_shadow_forward", dev, C.byref(d), ao.data_ptr(), ws.data_ptr(), ws.numel() * 4,
             None if ao_out is None else ao_out.data_ptr(), low.data_ptr(), smap.data_ptr())
        return smap, low, ws

    def forward(self, ao_map):
        """ao_map [N, 1, h, w], [1, h, w] or [h, w] -> {"shadow_map" [N, 1, U, U], "shadow_map_lowres" [N, 1, S, S], "ao_map": the
        input at S x S (the input itself where it has that size)}"""
        if not isinstance(ao_map, torch.Tensor) or ao_map.dim() not in (2, 3, 4) or ao_map.numel() == 0 or \
                (ao_map.dim() == 3 and ao_map.shape[0] != 1) or (ao_map.dim() == 4 and ao_map.shape[1] != 1):
            raise RuntimeError("ShadowUNet: ao_map must be [N, 1, h, w], [1, h, w] or [h, w]")
        if ao_map.requires_grad:
            raise RuntimeError("ShadowUNet: ao_map must not require grad: it is a constant here and its gradient would be dropped")
        h, w = ao_map.shape[-2:]
        if h > 8192 or w > 8192 or ao_map.numel() // (h * w) > 65535:
            raise RuntimeError("ShadowUNet: ao_map is too large")
        ao = expect(ao_map.reshape(-1, h, w), torch.float32, "ao_map")
        params = self._params()
        for p in params:
            expect(p, torch.float32, "ShadowUNet parameter")
        if self.ao_mean.device != ao.device or any(p.device != ao.device for p in params):
            raise RuntimeError("ShadowUNet: ao_map and the module must be on the same device")
        s = self.shadow_size
        resized = (h, w) != (s, s)
        ao_out = torch.empty(ao.shape[0], 1, s, s, dtype=torch.float32, device=ao.device) if resized else None
        if wants_grad(*params):
            smap, low = _Shadow.apply(self, ao, ao_out, *params)
        else:
            smap, low, _ = self._launch(ao, ao_out, params)
        return {"shadow_map": smap, "ao_map": ao_out if resized else ao_map, "shadow_map_lowres": low}
