#!/usr/bin/env python
"""Time the image head (train_appearance.py:126-127: the per-camera affine, the product with the rasteriser's alpha and the clip)
forward and forward + backward at 1024 x 1024, the size of the reference's training images.  Two statements of the same function
on the same device in one run, alternating:

  ours    mpmavatar_amd.image_head.camera_image under autograd (csrc/image_head.hip: one launch forward, two backward)
  torch   the reference's two lines as float32 torch operations under torch's own autograd, which is what a user had to run before
          these kernels existed

    python tools/image_head_bench.py [--size 1024] [--cams 160] [--warmup 20] [--reps 200] [--out file.json]

Each repetition is timed between two HIP events on torch's current stream; reported are the minimum, the median and the maximum per
statement for the forward pass alone under torch.no_grad() and for forward + backward of sum(w * image), the first call, the
device kernels each statement issues (counted by torch.profiler in a pass of its own, after the timing), the agreement of image and
gradients, and the algorithmic bytes of our launches (28 per pixel forward, 44 backward) with the rate they give.  "faster" is
claimed only where our maximum is below torch's minimum."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from mpmavatar_amd.image_head import camera_image


def torch_image(render, mask, cam_m, cam_c, camera_idx):
    image = render * torch.exp(cam_m[camera_idx])[:, None, None] + cam_c[camera_idx][:, None, None]
    return (image * mask).clip(0., 1.)


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def device_kernels(fn):
    """the number of device kernels one call of fn issues, or None where the profiler gives no device events"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
        return n or None
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--cams", type=int, default=160)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("image_head_bench.py measures on the GPU; there is none")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    H = W = a.size
    cam = a.cams // 3
    leaves = {"render": torch.rand((3, H, W), device=dev, generator=g) * 1.3 - 0.1, "mask": torch.rand((1, H, W), device=dev, generator=g),
              "cam_m": 0.2 * torch.randn((a.cams, 3), device=dev, generator=g), "cam_c": 0.05 * torch.randn((a.cams, 3), device=dev, generator=g)}
    leaves["mask"][:, : H // 4] = 0.0                       # the background of a rendered frame
    for t in leaves.values():
        t.requires_grad_(True)
    w = torch.randn((3, H, W), device=dev, generator=g)
    args = lambda: (leaves["render"], leaves["mask"], leaves["cam_m"], leaves["cam_c"], cam)
    variants = {"ours": lambda: camera_image(*args()), "torch": lambda: torch_image(*args())}

    def step(forward):
        for t in leaves.values():
            t.grad = None
        (w * forward()).sum().backward()

    def quiet(forward):
        with torch.no_grad():
            forward()

    first = {}
    for who, fwd in variants.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step(fwd)
        torch.cuda.synchronize()
        first[who] = (time.perf_counter() - t0) * 1e3
    for _ in range(a.warmup):
        for fwd in variants.values():
            step(fwd)
            quiet(fwd)
    times = {f"{who}_{what}": [] for who in variants for what in ("forward_backward", "forward_no_grad")}
    for _ in range(a.reps):                      # the two statements alternate, so that both see the same machine
        for who, fwd in variants.items():
            times[f"{who}_forward_backward"].append(event_ms(lambda: step(fwd)))
            times[f"{who}_forward_no_grad"].append(event_ms(lambda: quiet(fwd)))
    fwd_bytes, bwd_bytes = 28 * H * W, 44 * H * W
    res = {"size": [H, W], "cams": a.cams, "warmup": a.warmup, "reps": a.reps, "first_call_ms": first,
           "algorithmic_bytes": {"forward": fwd_bytes, "backward": bwd_bytes},
           "note": "forward_backward includes the w * image product, its sum and their backward, the same torch launches for both statements"}
    for k, ts in times.items():
        res[k] = {"min_ms": min(ts), "median_ms": statistics.median(ts), "max_ms": max(ts)}
    res["ours_forward_no_grad"]["GBps_algorithmic"] = fwd_bytes / (res["ours_forward_no_grad"]["median_ms"] * 1e-3) / 1e9
    for what in ("forward_backward", "forward_no_grad"):
        res[f"speedup_{what}"] = res[f"torch_{what}"]["median_ms"] / res[f"ours_{what}"]["median_ms"]
        res[f"faster_{what}"] = res[f"ours_{what}"]["max_ms"] < res[f"torch_{what}"]["min_ms"]      # our worst against torch's best
    # the head's own launches: the backward pass alone, fed a ready upstream gradient
    for who, fwd in variants.items():
        image = fwd()
        ts = [event_ms(lambda: torch.autograd.grad(image, list(leaves.values()), w, retain_graph=True)) for _ in range(a.warmup + a.reps)][a.warmup:]
        res[f"{who}_backward_alone"] = {"min_ms": min(ts), "median_ms": statistics.median(ts), "max_ms": max(ts)}
        res[f"{who}_kernels"] = {"forward": device_kernels(lambda: quiet(fwd)),
                                 "backward": device_kernels(lambda: torch.autograd.grad(image, list(leaves.values()), w, retain_graph=True))}
    res["ours_backward_alone"]["GBps_algorithmic"] = bwd_bytes / (res["ours_backward_alone"]["median_ms"] * 1e-3) / 1e9
    step(variants["ours"])
    g_ours = {k: t.grad.clone() for k, t in leaves.items()}
    i_ours = variants["ours"]().detach()
    step(variants["ours"])
    res["ours_same_bits_twice"] = all(torch.equal(g_ours[k], t.grad) for k, t in leaves.items())
    step(variants["torch"])
    res["image_rel_diff"] = float((i_ours - variants["torch"]().detach()).abs().max() / i_ours.abs().max())
    res["grad_rel_diff"] = {k: float((g_ours[k] - t.grad).abs().max() / t.grad.abs().max()) for k, t in leaves.items()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
