#!/usr/bin/env python
"""Time the shadow network (scene/shadow.py:14-181) at the reference's construction -- ShadowUNet(uv_size=256, shadow_size=256,
n_dims=4, biases=False, interp_mode="bilinear"), one 256 x 256 ambient-occlusion map (scene/mesh_gaussian_model.py:113-120) --
forward alone under torch.no_grad() and forward + backward of a weighted sum of the shadow map.  Two statements of the same
network on the same device in one run, alternating:

  ours    mpmavatar_amd.shadow_net.ShadowUNet (csrc/shadow.hip: 10 launches forward, 12 backward)
  torch   the same network as a float32 torch.nn.Module under torch's own autograd, restated below: weight norm with one norm over
          the whole of weight_v, F.conv2d, untied biases, F.leaky_relu, F.interpolate, torch.cat -- which is what a user had to run
          before these kernels existed; the warm-up lets MIOpen finish its search before anything is timed

    python tools/shadow_bench.py [--size 256] [--uv 256] [--dims 4] [--batch 1] [--warmup 20] [--reps 100] [--out file.json]

Each repetition is timed between two HIP events on torch's current stream; reported are the median, the minimum and the maximum per
statement, the first call, the agreement of outputs and gradients, the device launches of one step of either statement as torch's
profiler counts them (--count-launches, in a pass of its own after the timing), and the algorithmic bytes of the activations with
the rate they give.  "faster" is claimed only where our maximum is below torch's minimum."""
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

from mpmavatar_amd.shadow_net import ShadowUNet


class TorchShadowUNet(torch.nn.Module):
    """the network over the parameters of a ShadowUNet (shared, not copied), as torch ops"""

    def __init__(self, net):
        super().__init__()
        self.net = net

    @staticmethod
    def conv(layer, x):
        w = layer.weight_v * (layer.weight_g / torch.linalg.vector_norm(layer.weight_v))
        b = layer.bias
        return F.conv2d(x, w, None, 1, 1) + (b.reshape(1, 1, 1, 1) if b.dim() == 1 else b[None])

    def forward(self, ao_map):
        net = self.net
        s = net.shadow_size
        if tuple(ao_map.shape[-2:]) != (s, s):
            ao_map = F.interpolate(ao_map, size=(s, s))
        x = ao_map - net.ao_mean
        skips = []
        for i, seq in enumerate(net.enc_layers):
            x = F.leaky_relu(self.conv(seq[0], x), net.lrelu_slope)
            skips.append(x)
            if i < 3:
                x = F.interpolate(x, scale_factor=0.5, mode="bilinear", recompute_scale_factor=True, align_corners=True)
        for j, seq in enumerate(net.dec_layers):
            if j > 0:
                skip = skips[3 - j]
                x = torch.cat([F.interpolate(x, size=skip.shape[2:4], mode="bilinear", align_corners=True), skip], dim=1)
            x = F.leaky_relu(self.conv(seq[0], x), net.lrelu_slope)
        low = torch.sigmoid(self.conv(net.shadow_pred, x) + net.beta)
        return {"shadow_map": F.interpolate(low, (net.uv_size, net.uv_size), mode="bilinear", align_corners=False), "shadow_map_lowres": low}


def activation_bytes(n, s, u, c):
    """algorithmic bytes of the activations and untied biases: every tensor a pass must read or write, once.  forward: per layer
    its sources at their own size, its bias and its output; the final resize.  backward: per layer the saved output, the input
    gradients of its readers, its sources again (for dW), its own input gradient and its bias gradient; the head's three maps."""
    size = lambda layer: (s >> layer) if layer < 4 else (s >> (7 - layer)) if layer < 8 else s
    cin = lambda layer: 1 if layer == 0 else 2 * c if 5 <= layer <= 7 else c
    cout = lambda layer: 1 if layer == 8 else c
    fwd = bwd = 0
    for layer in range(9):
        q = size(layer) ** 2
        if layer == 0:
            src = n * q + q                                                            # the map and ao_mean
        elif layer in (4, 8):
            src = n * c * q
        else:
            src = n * c * size(layer - 1) ** 2 + (n * c * q if layer > 4 else 0)       # resampled source, and the skip
        bias = 1 if layer == 8 else cout(layer) * q
        fwd += 4 * (src + bias + n * cout(layer) * q)
        readers = n * cout(layer) * q if layer == 8 else n * c * size(layer + 1) ** 2 + (n * c * q if layer < 3 else 0)
        bwd += 4 * (n * cout(layer) * q + readers + src + (n * cin(layer) * q if layer else 0) + bias)
    fwd += 4 * n * u * u if u != s else 0
    bwd += 4 * (n * u * u + 2 * n * s * s)
    return fwd, bwd


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def count_launches(fn):
    """device kernels of one call, as torch's profiler sees them"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--uv", type=int, default=256)
    ap.add_argument("--dims", type=int, default=4)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--count-launches", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("shadow_bench.py measures on the GPU; there is none")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    f32 = lambda x: torch.tensor(x.astype(np.float32), device=dev)
    s, u, n = a.size, a.uv, a.batch
    net = ShadowUNet(uv_size=u, ao_mean=torch.tensor(rng.uniform(0.3, 0.7, (1, s, s)).astype(np.float32)), shadow_size=s, n_dims=a.dims,
                     interp_mode="bilinear", biases=False)
    with torch.no_grad():                        # seeded values: at the constructor's own the map is flat
        for k, p in net.named_parameters():
            p.copy_(torch.tensor((rng.normal(size=p.shape) if k.endswith("weight_v") else rng.uniform(0.5, 2.5, p.shape)
                                  if k.endswith("weight_g") else 0.3 * rng.normal(size=p.shape)).astype(np.float32)))
    net = net.to(dev)
    twin = TorchShadowUNet(net)
    ao, w = f32(rng.uniform(0, 1, (n, 1, s, s))), f32(rng.normal(size=(n, 1, u, u)))
    params = list(net.parameters())
    variants = {"ours": net, "torch": twin}

    def step(module):
        for p in params:
            p.grad = None
        (w * module(ao)["shadow_map"]).sum().backward()

    def quiet(module):
        with torch.no_grad():
            module(ao)

    first = {}
    for who, module in variants.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step(module)
        torch.cuda.synchronize()
        first[who] = (time.perf_counter() - t0) * 1e3
    for _ in range(a.warmup):
        for module in variants.values():
            step(module)
            quiet(module)
    times = {f"{who}_{what}": [] for who in variants for what in ("forward_backward", "forward_no_grad")}
    for _ in range(a.reps):                      # the two statements alternate, so that both see the same machine
        for who, module in variants.items():
            times[f"{who}_forward_backward"].append(event_ms(lambda: step(module)))
            times[f"{who}_forward_no_grad"].append(event_ms(lambda: quiet(module)))
    fwd_bytes, bwd_bytes = activation_bytes(n, s, u, a.dims)
    res = {"shadow_size": s, "uv_size": u, "n_dims": a.dims, "batch": n, "parameters": sum(p.numel() for p in params), "warmup": a.warmup,
           "reps": a.reps, "first_call_ms": first, "algorithmic_bytes": {"forward": fwd_bytes, "backward": bwd_bytes},
           "launches_by_construction": {"ours_forward": 10 + (u != s), "ours_backward": 12}}
    for k, ts in times.items():
        res[k] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}
    res["ours_forward_backward"]["GBps_algorithmic"] = (fwd_bytes + bwd_bytes) / (res["ours_forward_backward"]["median_ms"] * 1e-3) / 1e9
    res["ours_forward_no_grad"]["GBps_algorithmic"] = fwd_bytes / (res["ours_forward_no_grad"]["median_ms"] * 1e-3) / 1e9
    for what in ("forward_backward", "forward_no_grad"):
        res[f"speedup_{what}"] = res[f"torch_{what}"]["median_ms"] / res[f"ours_{what}"]["median_ms"]
        res[f"faster_{what}"] = res[f"ours_{what}"]["max_ms"] < res[f"torch_{what}"]["min_ms"]      # our worst against torch's best
    step(net)
    g_ours = [p.grad.clone() for p in params]
    m_ours = net(ao)["shadow_map"].detach()
    step(net)
    res["ours_same_bits_twice"] = all(torch.equal(g, p.grad) for g, p in zip(g_ours, params))
    step(twin)
    res["shadow_map_rel_diff"] = float((m_ours - twin(ao)["shadow_map"].detach()).abs().max() / m_ours.abs().max())
    res["grad_rel_diff_worst"] = max(float((g - p.grad).abs().max() / p.grad.abs().max()) for g, p in zip(g_ours, params))
    if a.count_launches:
        res["launches_profiled"] = {f"{who}_{what}": count_launches((lambda m=module: step(m)) if what == "forward_backward" else
                                                                   (lambda m=module: quiet(m)))
                                    for who, module in variants.items() for what in ("forward_backward", "forward_no_grad")}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
