#!/usr/bin/env python
"""Time forward + backward of the colours handed to the render call (train_appearance.py:120-123) -- SH features, positions and a
shadow map -> colors [n, 3] -> a weighted sum -> backward() -- at the size of tools/raster_bench.py and tools/binding_bench.py:
200,000 Gaussians on about 80,000 faces (the 200 x 200 cylinder), a 256 x 256 shadow map, SH degree 3.  Two statements of the same
function on the same device in one run, alternating:

  ours    mpmavatar_amd.shading.shaded_colors under autograd (csrc/shade.hip: one launch forward, three backward)
  torch   the float32 torch expression of the reference under torch's own autograd -- F.grid_sample, the index by the binding, the
          transpose / view / normalise / eval_sh / clamp_min chain of convert_SH, restated below -- which is what a user had to run
          before these kernels existed

    python tools/shade_bench.py [--gaussians 200000] [--warmup 10] [--reps 50] [--out file.json]

Each repetition is timed between two HIP events on torch's current stream; reported are the median, the minimum and the maximum per
statement, the forward pass alone under torch.no_grad(), the first call, the agreement of the gradients, and the algorithmic bytes of
our four launches (csrc/shade.hip has the per-item figures) with the rate they give.  "faster" is claimed only where our maximum is
below torch's minimum."""
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

from mpmavatar_amd import garment
from mpmavatar_amd.mesh_frames import _GaussianTable
from mpmavatar_amd.shading import ShadowSampler, shaded_colors

C0, C1 = 0.28209479177387814, 0.4886025119029199
C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
      -0.5900435899266435)


def torch_colors(dc, rest, means, campos, smap, uv_coord, binding64):
    """degree 3, float32: the launches of train_appearance.py:120-123 with convert_SH and the real spherical harmonics written out"""
    shadow = F.grid_sample(smap[None, None], uv_coord, mode="bilinear", align_corners=False).squeeze()[..., None][binding64]
    sh = torch.cat((dc, rest), dim=1).transpose(1, 2).view(-1, 3, 16)
    d = means - campos.repeat(sh.shape[0], 1)
    d = d / d.norm(dim=1, keepdim=True)
    x, y, z = d[..., 0:1], d[..., 1:2], d[..., 2:3]
    r = C0 * sh[..., 0]
    r = r - C1 * y * sh[..., 1] + C1 * z * sh[..., 2] - C1 * x * sh[..., 3]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    r = (r + C2[0] * xy * sh[..., 4] + C2[1] * yz * sh[..., 5] + C2[2] * (2.0 * zz - xx - yy) * sh[..., 6] + C2[3] * xz * sh[..., 7]
         + C2[4] * (xx - yy) * sh[..., 8])
    r = (r + C3[0] * y * (3 * xx - yy) * sh[..., 9] + C3[1] * xy * z * sh[..., 10] + C3[2] * y * (4 * zz - xx - yy) * sh[..., 11]
         + C3[3] * z * (2 * zz - 3 * xx - 3 * yy) * sh[..., 12] + C3[4] * x * (4 * zz - xx - yy) * sh[..., 13]
         + C3[5] * z * (xx - yy) * sh[..., 14] + C3[6] * x * (xx - 3 * yy) * sh[..., 15])
    return shadow * torch.clamp_min(r + 0.5, 0.0)


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=200000)
    ap.add_argument("--map", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("shade_bench.py measures on the GPU; there is none")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    n_f = garment.cylinder(200, 200, 0.25, 0.8, (1.0, 1.0, 1.0))[1].shape[0]
    n, size = a.gaussians, a.map
    f32 = lambda x: torch.tensor(x.astype(np.float32), device=dev)
    uv_coord = f32(rng.uniform(-1.0, 1.0, (n_f, 2)))[None, None]                      # one sample location per face, as uv_coord
    binding = torch.tensor(rng.integers(0, n_f, n).astype(np.int32), device=dev)      # unsorted, as after densification
    binding64 = binding.long()
    leaves = {"features_dc": f32(rng.normal(0, 0.5, (n, 1, 3))), "features_rest": f32(rng.normal(0, 0.3, (n, 15, 3))),
              "means3D": f32(rng.normal(0, 1.0, (n, 3))), "shadow_map": f32(rng.uniform(0.2, 1.0, (1, 1, size, size)))}
    for t in leaves.values():
        t.requires_grad_(True)
    campos, w = f32(np.array([0.2, -0.1, 4.0])), f32(rng.normal(size=(n, 3)))
    sampler, table = ShadowSampler(uv_coord, size, size), _GaussianTable()
    n_taps = int(sampler.texel_items.numel())

    def ours_forward():
        return shaded_colors(leaves["features_dc"], leaves["features_rest"], 3, leaves["means3D"], campos, binding=binding,
                             shadow_map=leaves["shadow_map"], sampler=sampler, gtable=table)

    def torch_forward():
        return torch_colors(leaves["features_dc"], leaves["features_rest"], leaves["means3D"], campos, leaves["shadow_map"][0, 0], uv_coord,
                            binding64)

    def step(forward):
        for t in leaves.values():
            t.grad = None
        (w * forward()).sum().backward()

    def quiet(forward):
        with torch.no_grad():
            forward()

    variants = {"ours": ours_forward, "torch": torch_forward}
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
    # algorithmic bytes of our launches: forward; backward stage 1 (per Gaussian), 2 (per face), 3 (per texel)
    fwd_bytes = n * 244
    bwd_bytes = n * 452 + (n * 8 + n_f * 8) + (size * size * 8 + n_taps * 16)
    res = {"gaussians": n, "faces": n_f, "map": [size, size], "taps_inside": n_taps, "sh_degree": 3, "warmup": a.warmup, "reps": a.reps,
           "first_call_ms": first, "algorithmic_bytes": {"forward": fwd_bytes, "backward": bwd_bytes}}
    for k, ts in times.items():
        res[k] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}
    res["ours_forward_backward"]["GBps_algorithmic"] = (fwd_bytes + bwd_bytes) / (res["ours_forward_backward"]["median_ms"] * 1e-3) / 1e9
    res["ours_forward_no_grad"]["GBps_algorithmic"] = fwd_bytes / (res["ours_forward_no_grad"]["median_ms"] * 1e-3) / 1e9
    for what in ("forward_backward", "forward_no_grad"):
        res[f"speedup_{what}"] = res[f"torch_{what}"]["median_ms"] / res[f"ours_{what}"]["median_ms"]
        res[f"faster_{what}"] = res[f"ours_{what}"]["max_ms"] < res[f"torch_{what}"]["min_ms"]      # our worst against torch's best
    step(ours_forward)
    g_ours = {k: t.grad.clone() for k, t in leaves.items()}
    c_ours = ours_forward().detach()
    step(ours_forward)
    res["ours_same_bits_twice"] = all(torch.equal(g_ours[k], t.grad) for k, t in leaves.items())
    step(torch_forward)
    res["colors_rel_diff"] = float((c_ours - torch_forward().detach()).abs().max() / c_ours.abs().max())
    res["grad_rel_diff"] = {k: float((g_ours[k] - t.grad).abs().max() / t.grad.abs().max()) for k, t in leaves.items()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
