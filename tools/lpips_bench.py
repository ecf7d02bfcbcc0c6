#!/usr/bin/env python
"""Time LPIPS (lpipsPyTorch, net_type 'vgg') at N = 1 and a square size (the appearance loop renders 1024 x 1024): forward alone
under torch.no_grad(), and forward + backward of `out` to the image.  Two statements of the same function on the same device in one
run, alternating:

  ours    mpmavatar_amd.lpips.LPIPS (csrc/lpips.hip: 19 launches forward, 18 backward, the f32-input MFMA)
  torch   the same function as float32 torch operations under torch's own autograd over the same weights (F.conv2d through MIOpen,
          F.relu, F.max_pool2d, the distance head) -- which is what a user had to run before these kernels existed; the warm-up lets
          MIOpen finish its search before anything is timed, and the first call is reported on its own

    python tools/lpips_bench.py [--size 1024] [--warmup 5] [--reps 20] [--out file.json]

Weights are seeded stand-ins of the real shapes (convolutions ~ N(0, 2 / (9 cin))): the time does not depend on their values.  Each
repetition is timed between two HIP events on torch's current stream; reported are the median, the minimum and the maximum per
statement, the first call, the agreement of `out` and the gradient, and the achieved TFLOP/s of ours from the convolution FLOPs counted
below against the 157.3 TFLOP/s f32 matrix peak.  "faster" is claimed only where our maximum is below torch's minimum."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.nn.functional as F

from mpmavatar_amd.lpips import CHANNELS, CONV_AT, LPIPS, TAP_CHANNELS

PEAK_TFLOPS = 157.3
POOL_AT, TAP_AFTER = (4, 9, 16, 23), (3, 8, 15, 22, 29)


def torch_lpips(p, x, y):
    """the function over a state dict with the reference's keys, as torch ops"""
    def features(v):
        v, taps = (v - p["net.mean"]) / p["net.std"], []
        for at in range(30):
            if at in CONV_AT:
                v = F.conv2d(v, p[f"net.layers.{at}.weight"], p[f"net.layers.{at}.bias"], padding=1)
            elif at in POOL_AT:
                v = F.max_pool2d(v, 2, 2)
            else:
                v = F.relu(v)
            if at in TAP_AFTER:
                taps.append(v / (torch.sqrt(torch.sum(v ** 2, dim=1, keepdim=True)) + 1e-10))
        return taps
    res = [F.conv2d((fx - fy) ** 2, p[f"lin.{i}.1.weight"]).mean((2, 3), True) for i, (fx, fy) in enumerate(zip(features(x), features(y)))]
    return torch.sum(torch.cat(res, 0), 0, True)


def conv_flops(h, w):
    """2 * cout * 9 cin * pixels per convolution of one image at its level -> (one forward pass, one backward-data pass); the
    backward pass of layer 0 produces no gradient further down but is the same product transposed"""
    level = (0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4)
    return sum(2 * cout * 9 * cin * (h >> lv) * (w >> lv) for (cin, cout), lv in zip(CHANNELS, level))


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lpips_bench.py measures on the GPU; there is none")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    f32 = lambda v: torch.tensor(np.asarray(v, np.float32))
    net = LPIPS()
    state = {"net.mean": net.net.mean, "net.std": net.net.std}
    for at, (cin, cout) in zip(CONV_AT, CHANNELS):
        state[f"net.layers.{at}.weight"] = f32(rng.normal(size=(cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin)))
        state[f"net.layers.{at}.bias"] = f32(0.05 + 0.05 * rng.normal(size=cout))
    for i, c in enumerate(TAP_CHANNELS):
        state[f"lin.{i}.1.weight"] = f32(rng.uniform(0, 2.0 / c, (1, c, 1, 1)))
    net.load_state_dict(state)
    net = net.to(dev)
    p = dict(net.state_dict())
    s = a.size
    x0 = f32(rng.uniform(0, 1, (1, 3, s, s))).to(dev)
    y = torch.clamp(x0 + 0.15 * torch.randn(x0.shape, device=dev, generator=torch.Generator(dev).manual_seed(1)), 0, 1)
    variants = {"ours": net, "torch": lambda u, v: torch_lpips(p, u, v)}
    last = {}

    def step(who):
        x = x0.clone().requires_grad_(True)
        out = variants[who](x, y)
        out.sum().backward()
        last[who] = (out.detach(), x.grad)

    def quiet(who):
        with torch.no_grad():
            variants[who](x0, y)

    first = {}
    for who in variants:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step(who)
        torch.cuda.synchronize()
        first[who] = (time.perf_counter() - t0) * 1e3
    for _ in range(a.warmup):
        for who in variants:
            step(who)
            quiet(who)
    times = {f"{who}_{what}": [] for who in variants for what in ("forward_backward", "forward_no_grad")}
    for _ in range(a.reps):                      # the two statements alternate, so that both see the same machine
        for who in variants:
            times[f"{who}_forward_backward"].append(event_ms(lambda: step(who)))
            times[f"{who}_forward_no_grad"].append(event_ms(lambda: quiet(who)))
    flops = conv_flops(s, s)
    res = {"size": s, "batch": 1, "warmup": a.warmup, "reps": a.reps, "first_call_ms": first,
           "conv_flops": {"forward_no_grad": 2 * flops, "forward_backward": 3 * flops}, "peak_tflops_f32_matrix": PEAK_TFLOPS,
           "launches_by_construction": {"ours_forward": 19, "ours_backward": 18}}
    for k, ts in times.items():
        res[k] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}
    for what, passes in (("forward_no_grad", 2), ("forward_backward", 3)):
        tf = passes * flops / (res[f"ours_{what}"]["median_ms"] * 1e-3) / 1e12
        res[f"ours_{what}"]["tflops"] = tf
        res[f"ours_{what}"]["fraction_of_peak"] = tf / PEAK_TFLOPS
        res[f"speedup_{what}"] = res[f"torch_{what}"]["median_ms"] / res[f"ours_{what}"]["median_ms"]
        res[f"faster_{what}"] = res[f"ours_{what}"]["max_ms"] < res[f"torch_{what}"]["min_ms"]      # our worst against torch's best
        res[f"slower_{what}"] = res[f"ours_{what}"]["min_ms"] > res[f"torch_{what}"]["max_ms"]
    step("ours")
    kept = last["ours"]
    step("ours")
    res["ours_same_bits_twice"] = bool(torch.equal(kept[0], last["ours"][0]) and torch.equal(kept[1], last["ours"][1]))
    step("torch")
    res["out_rel_diff"] = float((kept[0] - last["torch"][0]).abs().max() / last["torch"][0].abs().max())
    res["dx_rel_diff"] = float((kept[1] - last["torch"][1]).abs().max() / last["torch"][1].abs().max())
    res["peak_memory_GB"] = torch.cuda.max_memory_allocated() / 1e9
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
