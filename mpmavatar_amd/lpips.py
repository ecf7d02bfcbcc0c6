"""LPIPS on the device (lpipsPyTorch/modules/{lpips,networks,utils}.py, net_type 'vgg', version 0.1; train_appearance.py:78 and :133,
eval.py:59):

    lpips_net = LPIPS.from_checkpoints("vgg16-397923af.pth", "vgg.pth").cuda()
    lpips_loss = lpips_net(image.unsqueeze(0), gt_image.unsqueeze(0))                  # [1, 1, 1, 1]

with the reference's 33 ``state_dict()`` keys, shapes and order (``net.mean``, ``net.std``, ``net.layers.{0,2,..,28}.{weight,bias}``,
``lin.{0..4}.1.weight``), every parameter frozen, so that a state dict moves between the two classes in either direction.  Nothing is
downloaded, ever: the weights are the caller's two files (torchvision's VGG16 state dict and the upstream ``vgg.pth``), and a module
without weights raises when called.

The forward pass is ``mpmhip_lpips_forward`` (19 launches: thirteen convolutions on the f32-input MFMA with x and y in the same
launch, five distance heads, one sum), the backward pass ``mpmhip_lpips_backward`` (18 launches), csrc/lpips.hip: fp32, no atomics,
the same input gives the same bits.  The result is the sum over the five taps AND over the N images, as in the reference (it
concatenates the taps along the batch and sums over it), not their mean.  The only gradient is d out / d x; ``y`` must not require
grad (its gradient would be dropped).  There is no double backward.  With grad mode off, or with an ``x`` that needs no grad, the
output carries no ``grad_fn`` and nothing is kept.

One stated deviation: where a tap pixel's feature vector of x is all zero, the reference's gradient is NaN (0 / 0 through sqrt); here
that pixel's contribution is left out.

Memory: with a gradient the workspace keeps the thirteen post-ReLU maps of x (1.1 GB at 1024 x 1024), the five tap maps of y (0.5 GB),
the five tap gradients (0.5 GB) and four alternating buffers of 64 h w floats (1.1 GB), until backward has run; without one, the taps
of both images and four alternating buffers, released on return.  No CPU fallback: tensors must live on an MI355X.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _lib as L
from ._call import call, expect, upstream, wants_grad

CONV_AT = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)       # the convolutions of torchvision's vgg16().features[0:30]
CHANNELS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
            (512, 512), (512, 512), (512, 512))
TAP_CHANNELS = (64, 128, 256, 512, 512)
ENV_VGG16, ENV_LIN = "MPMHIP_LPIPS_VGG16", "MPMHIP_LPIPS_LIN"


class _Frozen(torch.nn.Module):
    """A holder of frozen parameters under the reference's names; never called."""

    def forward(self, *args):
        raise RuntimeError("LPIPS runs as one fused call; its layers are not callable on their own")


def _frozen(shape):
    return torch.nn.Parameter(torch.zeros(shape), requires_grad=False)


class _Net(_Frozen):
    def __init__(self):
        super().__init__()
        self.register_buffer("mean", torch.tensor([-.030, -.088, -.188])[None, :, None, None])
        self.register_buffer("std", torch.tensor([.458, .448, .450])[None, :, None, None])
        self.layers = _Frozen()
        for at, (cin, cout) in zip(CONV_AT, CHANNELS):
            conv = _Frozen()
            conv.weight, conv.bias = _frozen((cout, cin, 3, 3)), _frozen((cout,))
            self.layers.add_module(str(at), conv)


class _Lpips(torch.autograd.Function):
    """(x [N, 3, H, W]) -> out [1, 1, 1, 1]; the workspace of the forward pass is kept for backward"""

    @staticmethod
    def forward(ctx, net, x, y):
        out, ws = net._launch(x, y, keep=1)
        ctx.net, ctx.ws, ctx.shape = net, ws, x.shape
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        g, net, ws = upstream(g_out, (1, 1, 1, 1)), ctx.net, ctx.ws
        ctx.ws = None
        dx = torch.empty(ctx.shape, dtype=torch.float32, device=g.device)
        d = net._desc(*ctx.shape[:1], *ctx.shape[2:])
        call("mpmhip_lpips_backward", g.device, C.byref(d), g.data_ptr(), ws.data_ptr(), ws.numel() * 4, dx.data_ptr())
        return None, dx, None


def _check_kind(net_type, version):
    if net_type != "vgg":
        raise NotImplementedError(f"LPIPS: net_type must be 'vgg' (the appearance loop's), got net_type={net_type!r}")
    if version != "0.1":
        raise NotImplementedError(f"LPIPS: version must be '0.1', got version={version!r}")


class LPIPS(torch.nn.Module):
    def __init__(self, net_type: str = "vgg", version: str = "0.1"):
        super().__init__()
        _check_kind(net_type, version)
        self.net = _Net()
        self.lin = _Frozen()
        for i, c in enumerate(TAP_CHANNELS):
            pair = _Frozen()
            pair.add_module("1", _Frozen())
            getattr(pair, "1").weight = _frozen((1, c, 1, 1))
            self.lin.add_module(str(i), pair)
        self._loaded = False
        self._backward_weights, self._backward_key = None, None
        self.register_load_state_dict_post_hook(lambda module, incompatible: setattr(module, "_loaded", not incompatible.missing_keys))
        L.load()                                 # a missing library is reported here, not at the first launch

    # ---- weights -------------------------------------------------------------------------------------------------------------------

    @classmethod
    def from_checkpoints(cls, vgg16_path, lin_path, net_type: str = "vgg", version: str = "0.1"):
        """The two files a user of the reference already has: torchvision's VGG16 state dict (``features.N.*`` is used,
        ``classifier.*`` ignored) and the upstream ``vgg.pth`` (``lin{i}.model.1.weight``, renamed as the reference renames them)."""
        net = cls(net_type, version)
        vgg = torch.load(vgg16_path, map_location="cpu", weights_only=True)
        lin = torch.load(lin_path, map_location="cpu", weights_only=True)
        state = {"net.mean": net.net.mean, "net.std": net.net.std}
        for at in CONV_AT:
            for kind in ("weight", "bias"):
                if f"features.{at}.{kind}" not in vgg:
                    raise KeyError(f"LPIPS.from_checkpoints: {vgg16_path} has no 'features.{at}.{kind}'")
                state[f"net.layers.{at}.{kind}"] = vgg[f"features.{at}.{kind}"]
        for key, val in lin.items():
            state["lin." + key.replace("lin", "").replace("model.", "")] = val
        net.load_state_dict(state)
        return net

    @classmethod
    def from_environment(cls, net_type: str = "vgg", version: str = "0.1"):
        _check_kind(net_type, version)
        paths = os.environ.get(ENV_VGG16), os.environ.get(ENV_LIN)
        if not all(paths):
            raise RuntimeError(f"LPIPS: set {ENV_VGG16} (torchvision's VGG16 state dict) and {ENV_LIN} (the upstream vgg.pth) to the "
                               "paths of the weight files; nothing is downloaded")
        return cls.from_checkpoints(*paths, net_type=net_type, version=version)

    def _convs(self):
        return [getattr(self.net.layers, str(at)) for at in CONV_AT]

    def _taps(self):
        return [getattr(getattr(self.lin, str(i)), "1").weight for i in range(5)]

    def _backward_layouts(self, dev):
        """the flipped, transposed weights, rebuilt when a weight's version or storage changes"""
        weights = [c.weight for c in self._convs()]
        key = tuple((w.data_ptr(), w._version) for w in weights) + (str(dev),)
        if key != self._backward_key:
            self._backward_weights = [torch.empty(w.numel(), dtype=torch.float32, device=dev) for w in weights]
            self._backward_key = key
            call("mpmhip_lpips_prepare_weights", dev, C.byref(self._desc(0, 16, 16)))
        return self._backward_weights

    # ---- the launches ------------------------------------------------------------------------------------------------------------

    def _desc(self, n, h, w):
        d = L.LpipsDesc()
        d.n, d.h, d.w = n, h, w
        for i, conv in enumerate(self._convs()):
            d.weight[i], d.bias[i] = conv.weight.data_ptr(), conv.bias.data_ptr()
            d.weight_bwd[i] = None if self._backward_weights is None else self._backward_weights[i].data_ptr()
        for i, tap in enumerate(self._taps()):
            d.tap_weight[i] = tap.data_ptr()
        mean, std = self.net.mean.flatten().tolist(), self.net.std.flatten().tolist()
        for c in range(3):
            d.mean[c], d.std[c] = mean[c], std[c]
        return d

    def _launch(self, x, y, keep):
        n, _, h, w = x.shape
        dev = x.device
        if keep:
            self._backward_layouts(dev)
        d, nbytes = self._desc(n, h, w), C.c_int64(0)
        call("mpmhip_lpips_workspace_bytes", dev, C.byref(d), keep, C.byref(nbytes))
        ws = torch.empty(nbytes.value // 4, dtype=torch.float32, device=dev)
        out = torch.empty(1, 1, 1, 1, dtype=torch.float32, device=dev)
        call("mpmhip_lpips_forward", dev, C.byref(d), x.data_ptr(), y.data_ptr(), keep, ws.data_ptr(), ws.numel() * 4, out.data_ptr())
        return out, ws

    def forward(self, x, y):
        """x, y [N, 3, H, W] or [3, H, W] (N = 1), H, W >= 16 -> [1, 1, 1, 1]: the sum over the five taps and the N images"""
        if not self._loaded:
            raise RuntimeError("LPIPS: no weights loaded: use LPIPS.from_checkpoints(vgg16_path, lin_path) or load_state_dict")
        for name, t in (("x", x), ("y", y)):
            if not isinstance(t, torch.Tensor) or t.dim() not in (3, 4) or t.shape[-3] != 3:
                raise RuntimeError(f"LPIPS: {name} must be [N, 3, H, W] or [3, H, W]")
        if y.requires_grad:
            raise RuntimeError("LPIPS: y must not require grad: the only gradient is d out / d x, and y's would be dropped")
        x4, y4 = x.reshape(-1, *x.shape[-3:]), y.reshape(-1, *y.shape[-3:])
        if x4.shape != y4.shape:
            raise RuntimeError(f"LPIPS: x and y must have the same shape, got {tuple(x.shape)} and {tuple(y.shape)}")
        n, _, h, w = x4.shape
        if n < 1 or n > 1024 or not (16 <= h <= 8192 and 16 <= w <= 8192):
            raise RuntimeError(f"LPIPS: need 1 <= N <= 1024 and 16 <= H, W <= 8192 (four poolings must leave 1 x 1), got {tuple(x4.shape)}")
        x4, y4 = expect(x4.contiguous(), torch.float32, "x"), expect(y4.contiguous(), torch.float32, "y")
        params = [p for conv in self._convs() for p in (conv.weight, conv.bias)] + self._taps()
        for p in params:
            expect(p, torch.float32, "LPIPS parameter")
        if any(p.device != x4.device for p in params) or y4.device != x4.device:
            raise RuntimeError("LPIPS: x, y and the module must be on the same device")
        if wants_grad(x4):
            return _Lpips.apply(self, x4, y4)
        return self._launch(x4, y4, keep=0)[0]


def lpips(x, y, net_type: str = "vgg", version: str = "0.1"):
    """The functional form of lpipsPyTorch/__init__.py; the weights come from the files MPMHIP_LPIPS_VGG16 and MPMHIP_LPIPS_LIN name."""
    return LPIPS.from_environment(net_type, version).to(x.device)(x, y)
