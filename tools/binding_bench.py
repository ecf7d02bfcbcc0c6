#!/usr/bin/env python
"""Time forward + backward of the mesh binding -- vertices and raw parameters -> face frames -> the rasteriser's argument lists ->
a weighted sum -> backward() -- at the size of tools/raster_bench.py: 200,000 Gaussians on the reference-sized garment (the
200 x 200 cylinder, about 80,000 faces).  Two statements of the same function on the same device in one run, alternating:

  ours    MeshFrames.set_mesh_by_verts + BoundGaussians.render_inputs under autograd (csrc/frames.hip, csrc/frames_backward.hip)
  torch   tests/binding_twin_torch.py in float32 under torch's own autograd: what a user had to write before these kernels had
          a backward pass

    python tools/binding_bench.py [--gaussians 200000] [--warmup 10] [--reps 50] [--out file.json]

Each repetition is timed between two HIP events on torch's current stream; reported are the median, the minimum and the maximum per
statement, the forward pass alone under torch.no_grad(), the first call, the agreement of the two gradients, and the algorithmic
bytes of our six launches (forward 2, backward 4; DESIGN.md has the per-item figures) with the rate they give."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import binding_twin_torch as tw
from mpmavatar_amd import garment
from mpmavatar_amd.mesh_frames import MeshFrames
from mpmavatar_amd.render_inputs import BoundGaussians

OUTS = ("means3D", "rotations", "scales", "opacities")


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
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("binding_bench.py measures on the GPU; there is none")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    v, f = garment.cylinder(200, 200, 0.25, 0.8, (1.0, 1.0, 1.0))
    n_v, n_f, n = v.shape[0], f.shape[0], a.gaussians
    verts = torch.tensor((v + rng.normal(0, 1e-4, v.shape)).astype(np.float32), device=dev).requires_grad_(True)
    faces = torch.tensor(f.astype(np.int32), device=dev)
    binding = torch.tensor(rng.integers(0, n_f, n).astype(np.int32), device=dev)      # unsorted, as after densification
    leaf = lambda x: torch.tensor(x.astype(np.float32), device=dev).requires_grad_(True)
    p = {"_xyz": leaf(rng.normal(0, 0.4, (n, 3))), "_rotation": leaf(rng.normal(size=(n, 4))), "_scaling": leaf(rng.normal(-1, 0.6, (n, 3))),
         "_opacity": leaf(rng.normal(0, 2, (n, 1)))}
    w = {k: torch.tensor(rng.normal(size=(n, c)).astype(np.float32), device=dev) for k, c in zip(OUTS, (3, 4, 3, 1))}
    leaves = [verts] + list(p.values())
    frames = MeshFrames(faces)
    bound = BoundGaussians(p["_xyz"], p["_rotation"], p["_scaling"], p["_opacity"], torch.zeros(n, 1, 3, device=dev),
                           torch.zeros(n, 0, 3, device=dev), binding)
    faces64, binding64 = faces.long(), binding.long()

    def ours_forward():
        frames.set_mesh_by_verts(verts)
        return bound.render_inputs(frames)

    def torch_forward():
        return tw.render_inputs(verts, faces64, binding64, p["_xyz"], p["_rotation"], p["_scaling"], p["_opacity"])

    def step(forward):
        for t in leaves:
            t.grad = None
        out = forward()
        sum((w[k] * out[k]).sum() for k in OUTS).backward()

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
    # algorithmic bytes of our launches (4-byte items): forward frames + render_inputs, backward kernels 1 to 4
    fwd_bytes = n_f * (24 + 68 + 36 - 12) + n * (4 + 48 + 56 + 56)
    bwd_bytes = n * (36 + 44 + 56 + 44) + (n * (44 + 40) + n_f * (8 + 56 + 68)) + n_f * (12 + 36 + 52 + 68 + 36) + (3 * n_f * (4 + 12) + n_v * (8 + 12))
    res = {"gaussians": n, "faces": n_f, "vertices": n_v, "warmup": a.warmup, "reps": a.reps, "first_call_ms": first,
           "algorithmic_bytes": {"forward": fwd_bytes, "backward": bwd_bytes}}
    for k, ts in times.items():
        res[k] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}
    res["ours_forward_backward"]["GBps_algorithmic"] = (fwd_bytes + bwd_bytes) / (res["ours_forward_backward"]["median_ms"] * 1e-3) / 1e9
    res["speedup_forward_backward"] = res["torch_forward_backward"]["median_ms"] / res["ours_forward_backward"]["median_ms"]
    res["speedup_forward_no_grad"] = res["torch_forward_no_grad"]["median_ms"] / res["ours_forward_no_grad"]["median_ms"]
    step(ours_forward)
    g_ours = [t.grad.clone() for t in leaves]
    step(torch_forward)
    res["grad_rel_diff"] = {k: float((a_ - b_.grad).abs().max() / b_.grad.abs().max())
                            for k, a_, b_ in zip(("verts",) + tuple(p), g_ours, leaves)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
