#!/usr/bin/env python
"""Time the image loss (csrc/image_loss.hip through mpmavatar_amd.image_loss.image_loss) at the frame of tools/raster_bench.py,
3 x 1024 x 1024: the forward pass alone (under torch.no_grad(): no maps), the forward pass that stores its maps, and forward +
backward, each between two HIP events on torch's current stream after a warm-up.  Beside it the same expression written in
plain torch on the same device (five depthwise 11 x 11 conv2d calls and the elementwise operations around them, as
utils/loss_utils.py composes it), so that both numbers come from one run.

    python tools/image_loss_bench.py [--size 1024] [--channels 3] [--warmup 20] [--reps 200] [--out file.json]

Reported per variant: milliseconds per call and the achieved GB/s against the ALGORITHMIC bytes -- forward: two images in
(and three maps out when a gradient is wanted); backward: three maps and two images in, one image out; 4 bytes each.  The
plain-torch statement moves far more than that; the same byte count is used for it, so its figure is a rate of useful bytes,
not of traffic.  The first call of each variant is timed on its own: for the torch statement it includes the library's
choice of a convolution kernel for a new shape."""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from mpmavatar_amd import image_loss as il

LAMBDA = 0.2


def torch_window(channels, device):
    g = torch.tensor([math.exp(-(i - 5) ** 2 / (2 * 1.5 ** 2)) for i in range(11)], dtype=torch.float32, device=device)
    g = g / g.sum()
    return (g[:, None] * g[None, :]).expand(channels, 1, 11, 11).contiguous()


def torch_loss(image, gt, window, lam=LAMBDA):
    """(1 - lam) * mean |image - gt| + lam * (1 - ssim(image, gt)) in plain torch"""
    ch = image.shape[-3]
    conv = lambda t: F.conv2d(t, window, padding=5, groups=ch)
    mu1, mu2 = conv(image), conv(gt)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = conv(image * image) - mu1_sq, conv(gt * gt) - mu2_sq, conv(image * gt) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    ssim = (((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))).mean()
    return (1.0 - lam) * (image - gt).abs().mean() + lam * (1.0 - ssim)


def events_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def first_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("image_loss_bench.py measures on the GPU; there is none")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    shape = (a.channels, a.size, a.size)
    gt = torch.rand(shape, device=dev, generator=g)
    image = (gt + 0.1 * torch.randn(shape, device=dev, generator=g)).clip(0, 1).requires_grad_(True)
    window = torch_window(a.channels, dev)
    plane_bytes = 4 * a.channels * a.size * a.size
    bytes_of = {"forward_no_grad": 2 * plane_bytes, "forward": 5 * plane_bytes, "forward_backward": 5 * plane_bytes + 6 * plane_bytes}

    def ours_forward_no_grad():
        with torch.no_grad():
            il.image_loss(image, gt, LAMBDA)

    def ours_forward():
        il.image_loss(image, gt, LAMBDA)

    def ours_forward_backward():
        image.grad = None
        il.image_loss(image, gt, LAMBDA)[0].backward()

    def torch_forward_no_grad():
        with torch.no_grad():
            torch_loss(image, gt, window)

    def torch_forward():
        torch_loss(image, gt, window)

    def torch_forward_backward():
        image.grad = None
        torch_loss(image, gt, window).backward()

    variants = {"ours": (ours_forward_no_grad, ours_forward, ours_forward_backward),
                "torch": (torch_forward_no_grad, torch_forward, torch_forward_backward)}
    res = {"image": list(shape), "warmup": a.warmup, "reps": a.reps, "lambda_dssim": LAMBDA, "algorithmic_bytes": bytes_of}
    for who, fns in variants.items():
        for key, fn in zip(bytes_of, fns):
            first = first_ms(fn)
            for _ in range(a.warmup):
                fn()
            ms = events_ms(fn, a.reps)
            res[f"{who}_{key}"] = {"ms": ms, "first_call_ms": first, "GBps_algorithmic": bytes_of[key] / (ms * 1e-3) / 1e9}
    # the two statements agree, and the gradient too
    ours_forward_backward()
    g_ours, l_ours = image.grad.clone(), float(il.image_loss(image, gt, LAMBDA)[0])
    torch_forward_backward()
    g_torch, l_torch = image.grad.clone(), float(torch_loss(image, gt, window))
    res["loss_ours"], res["loss_torch"] = l_ours, l_torch
    res["grad_rel_diff"] = float((g_ours - g_torch).abs().max() / g_torch.abs().max())
    res["speedup_forward_backward"] = res["torch_forward_backward"]["ms"] / res["ours_forward_backward"]["ms"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
