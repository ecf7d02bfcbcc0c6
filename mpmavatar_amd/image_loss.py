"""Image loss and image metrics on the GPU: what stands between the render call and ``loss.backward()`` in the appearance loop
(/root/reference/train_appearance.py:132-134) and what every run's evaluation ends with (eval.py:59-98).  The reference's
import lines

    from utils.loss_utils import l1_loss, ssim
    from utils.image_utils import psnr

become ``from mpmavatar_amd.image_loss import l1_loss, ssim, psnr`` with the same signatures, over the two HIP entry points
``mpmhip_image_loss_forward`` and ``mpmhip_image_loss_backward`` (csrc/image_loss.hip).  The loss expression of the loop,

    Ll1 = l1_loss(image, gt)
    loss = (1.0 - lambda_dssim) * Ll1 + lambda_dssim * (1.0 - ssim(image, gt))

is ``loss, Ll1, ssim_value = image_loss(image, gt, lambda_dssim)``: ONE forward launch and, in ``loss.backward()``, one
backward launch (the two separate calls above cost two of each and give the same numbers).  The evaluation loop is

    ev = AppEval()
    for frame in frames:
        ev.add_frame(img_pred, img_gt, mask)                   # nothing leaves the device, nothing synchronises
    ev.save(output_path)                                       # app_metric.npz, keys "PSNR" and "SSIM"

LPIPS (train_appearance.py:133, eval.py:89) is ``mpmavatar_amd/lpips.py`` (its weights are the caller's files): the caller adds
``lambda_lpips * lpips_net(image[None], gt[None])`` to ``image_loss``'s result, and ``AppEval(lpips=lpips_net)`` adds the "LPIPS" key
of ``app_metric.npz``.

All four functions share one ``torch.autograd.Function`` whose outputs are the per-plane means (a plane is one (batch,
channel) image) of |d|, d^2 and the SSIM map as three ``[planes]`` tensors; the means over planes, ``1 - ssim``, the lambda
mix and ``log10`` are ordinary torch operations on those tiny tensors, so autograd hands the per-plane upstream gradients to
the backward launch on the device and no value passes through the host.  The gradient goes to the FIRST argument only.
Under ``torch.no_grad()``, or when the first argument does not require grad, the three partial-derivative maps the
backward pass needs are not stored and not allocated; the values are the same bits either way.  Inputs are fp32 tensors on
the GPU, ``[C, H, W]`` or ``[N, C, H, W]``; the kernels run on the current torch stream; there is no double backward.  No
CPU fallback: tensors must live on an MI355X.

The variances are formed as E[x^2] - mu^2 in fp32, as the reference forms them: on nearly constant images that difference
cancels and the reference's own fp32 result is off in the fifth decimal.  That behaviour is kept.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from ._call import call, expect, ptr, upstream

WINDOW_SIZE = 11


def _chk(t, name):
    expect(t, torch.float32, name, contiguous=False)
    if t.dim() not in (3, 4) or t.numel() == 0:
        raise RuntimeError(f"{name}: expected a non-empty [C, H, W] or [N, C, H, W] tensor, got {tuple(t.shape)}")
    return t


def scratch_doubles(planes, H, W):
    """MPMHIP_IMAGE_LOSS_SCRATCH of include/mpmhip.h: one triple of doubles per 16 x 16 tile."""
    return planes * ((H + 15) // 16) * ((W + 15) // 16) * 3


class _PlaneMeans(torch.autograd.Function):
    """(img, gt) [planes, H, W] -> (mean |d|, mean d^2, mean SSIM map), each [planes].  want_grad: whether a graph is being
    built for img (the caller's grad mode and img.requires_grad; ctx.needs_input_grad ignores the grad mode)."""

    @staticmethod
    def forward(ctx, img, gt, want_grad):
        planes, H, W = img.shape
        dev = img.device
        maps = torch.empty((planes, 3, H, W), dtype=torch.float32, device=dev) if want_grad else None
        scratch = torch.empty(scratch_doubles(planes, H, W), dtype=torch.float64, device=dev)
        out = torch.empty((planes, 3), dtype=torch.float32, device=dev)
        call("mpmhip_image_loss_forward", dev, img.data_ptr(), gt.data_ptr(), planes, H, W,
             ptr(maps), scratch.data_ptr(), out.data_ptr())
        if want_grad:
            ctx.save_for_backward(img, gt, maps)
        return out[:, 0].contiguous(), out[:, 1].contiguous(), out[:, 2].contiguous()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_l1, g_mse, g_ssim):
        img, gt, maps = ctx.saved_tensors
        planes, H, W = img.shape
        g = [torch.zeros(planes, dtype=torch.float32, device=img.device) if t is None else upstream(t) for t in (g_l1, g_mse, g_ssim)]
        d_img = torch.empty_like(img)
        call("mpmhip_image_loss_backward", img.device, img.data_ptr(), gt.data_ptr(), planes, H, W, maps.data_ptr(),
             g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(), d_img.data_ptr())
        return d_img, None, None


def plane_means(img1, img2):
    """The three per-plane means behind every function here: (mean |img1 - img2|, mean (img1 - img2)^2, mean SSIM map),
    each of shape ``img1.shape[:-2]``, from one launch."""
    a, b = _chk(img1, "img1"), _chk(img2, "img2")
    if a.shape != b.shape or a.device != b.device:
        raise RuntimeError(f"img1 and img2 must have one shape and one device, got {tuple(a.shape)} and {tuple(b.shape)}")
    if b.requires_grad and torch.is_grad_enabled():
        raise RuntimeError("img2 requires grad: the image loss differentiates with respect to its first argument only")
    if a.numel() > 2 ** 31 - 1:
        raise RuntimeError("more than 2^31 - 1 pixels")
    H, W = a.shape[-2:]
    lead = a.shape[:-2]
    out = _PlaneMeans.apply(a.contiguous().view(-1, H, W), b.detach().contiguous().view(-1, H, W),
                            a.requires_grad and torch.is_grad_enabled())
    return tuple(t.view(lead) for t in out)


def l1_loss(network_output, gt):
    """utils/loss_utils.py:18-19: torch.abs(network_output - gt).mean(), a 0-d tensor."""
    return plane_means(network_output, gt)[0].mean()


def _ssim_from(m, size_average):
    if size_average:
        return m.mean()
    if m.dim() != 2:
        raise IndexError("ssim(size_average=False) needs a 4-D input, as the reference's .mean(1).mean(1).mean(1) does")
    return m.mean(1)


def ssim(img1, img2, window_size=11, size_average=True):
    """utils/loss_utils.py:34-64.  0-d tensor, or [N] with size_average=False on a 4-D input (a 3-D input raises there, as in
    the reference).  Only the window of 11 exists, the one every caller uses."""
    if window_size != WINDOW_SIZE:
        raise ValueError(f"window_size must be {WINDOW_SIZE}, got {window_size}")
    return _ssim_from(plane_means(img1, img2)[2], size_average)


def _psnr_from(mse, ndim):
    per_first = mse if ndim == 3 else mse.mean(1)       # image_utils.py:18: .view(img1.shape[0], -1).mean(1, keepdim=True)
    return (20 * torch.log10(1.0 / torch.sqrt(per_first))).unsqueeze(1)


def psnr(img1, img2):
    """utils/image_utils.py:17-19: [img1.shape[0], 1]; the mean squared error is taken per FIRST dimension -- per channel for
    a 3-D image, per batch item for a 4-D one."""
    return _psnr_from(plane_means(img1, img2)[1], img1.dim())


def image_loss(image, gt, lambda_dssim=0.2):
    """train_appearance.py:132,134 without its LPIPS term: (loss, Ll1, ssim_value), all 0-d, from one forward launch; the
    driver logs Ll1 (train_appearance.py:172)."""
    l1, _, m = plane_means(image, gt)
    Ll1, s = l1.mean(), m.mean()
    return (1.0 - lambda_dssim) * Ll1 + lambda_dssim * (1.0 - s), Ll1, s


class AppEval:
    """The appearance loop of eval.py:59-98 with the metrics on the device: one (PSNR, SSIM) pair per frame, kept as device
    scalars.  The mask erosion and white-pixel removal of eval.py:71-83 are ``eval_mask`` and ``eval_inputs`` of
    mpmavatar_amd/image_head.py, whose pair goes straight into ``add_frame``.  With
    ``lpips`` (a module of mpmavatar_amd/lpips.py with its weights loaded) every frame also gets the LPIPS of the masked pair
    (eval.py:89) and app_metric.npz its "LPIPS" key; without it LPIPS is not computed and the file has no such key."""

    def __init__(self, lpips=None):
        self.psnrs, self.ssims, self.lpips, self.lpipss = [], [], lpips, []

    def add_frame(self, img_pred, img_gt, mask=None):
        """eval.py:86-91: both images times the mask if given, a [C, H, W] image made a batch of one as there (so that the
        PSNR is that of the whole image, not the mean over its channels), then psnr(...) and ssim(...).  Returns the pair
        (PSNR, SSIM), or the triple (PSNR, SSIM, LPIPS) where the evaluation has an LPIPS module."""
        with torch.no_grad():
            if mask is not None:
                img_pred, img_gt = img_pred * mask, img_gt * mask
            if img_pred.dim() == 3:
                img_pred, img_gt = img_pred.unsqueeze(0), img_gt.unsqueeze(0)
            _, mse, m = plane_means(img_pred, img_gt)
            pair = _psnr_from(mse, img_pred.dim()).mean(), m.mean()
            if self.lpips is not None:
                pair = pair + (self.lpips(img_pred, img_gt).reshape(()),)
        self.psnrs.append(pair[0])
        self.ssims.append(pair[1])
        if self.lpips is not None:
            self.lpipss.append(pair[2])
        return pair

    def results(self):
        """{"PSNR": [...], "SSIM": [...]} per frame on the host (the one synchronisation): the fp32 device values as float64,
        what the reference's lists of .item() become in np.savez; with an LPIPS module also "LPIPS", first as in eval.py:59."""
        rows = ([self.lpipss] if self.lpips is not None else []) + [self.psnrs, self.ssims]
        keys = (["LPIPS"] if self.lpips is not None else []) + ["PSNR", "SSIM"]
        if not self.psnrs:
            return {k: np.zeros(0, np.float64) for k in keys}
        r = torch.stack([torch.stack(row) for row in rows]).cpu().numpy().astype(np.float64)
        return {k: r[i].copy() for i, k in enumerate(keys)}

    def means(self):
        """(mean PSNR, mean SSIM) over the frames, as eval.py:93-95 prints them."""
        r = self.results()
        return float(r["PSNR"].mean()), float(r["SSIM"].mean())

    def save(self, directory):
        """app_metric.npz as eval.py:98 writes it ("LPIPS" only with an LPIPS module); plain arrays, loads without pickle."""
        r = self.results()
        os.makedirs(directory, exist_ok=True)
        path = os.path.join(directory, "app_metric.npz")
        np.savez(path, **r)
        return path
