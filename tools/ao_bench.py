#!/usr/bin/env python
"""Time the AO bake (mpmavatar_amd.ao_bake, csrc/ao.hip) per frame and per stage at the size of the garment:
the 200 x 200 cylinder of scenes.garment_cylinder (79,600 faces), wrinkled so that it shades itself, with a generated atlas (the
cylinder unrolled, one seam), a 256 x 256 map and 256 rays per texel -- the reference's --ao_res and this project's default S.

    python tools/ao_bench.py [--map 256] [--samples 256] [--warmup 5] [--reps 30] [--out file.json]

Each repetition is timed between two HIP events on torch's current stream: the whole bake, and its three stages one at a time
(grid: records + box + count / scan / fill; trace; margin).  Reported are the median, the minimum and the maximum, the one-time
costs (constructor, first bake), the sizes, and that two bakes gave the same bits.  There is no second implementation to compare
with: Blender's bake cannot run here.  The figure to hold the result against is the simulation of the frame it shades, 400
substeps of the garment."""
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

from mpmavatar_amd import garment
from mpmavatar_amd.ao_bake import AOBaker


def wrinkled_cylinder(n_theta=200, n_h=200):
    """the garment cylinder with radial wrinkles, and its atlas: u along theta (a seam column of its own), v along the height"""
    verts, faces = garment.cylinder(n_theta, n_h, 0.25, 0.8, (1.0, 1.0, 1.0))
    v = verts.astype(np.float64) - 1.0
    theta, y = np.arctan2(v[:, 2], v[:, 0]), v[:, 1]
    r = 0.25 * (1.0 + 0.10 * np.sin(9 * theta) * np.sin(25 * y) + 0.04 * np.sin(31 * theta + 40 * y))
    verts = (np.stack([r * np.cos(theta), y, r * np.sin(theta)], -1) + 1.0).astype(np.float32)
    row, t = np.meshgrid(np.arange(n_h), np.arange(n_theta + 1), indexing="ij")
    vt = np.stack([0.01 + 0.98 * t / n_theta, 0.99 - 0.98 * row / (n_h - 1)], -1).reshape(-1, 2).astype(np.float32)
    rr, tt = np.meshgrid(np.arange(n_h - 1), np.arange(n_theta), indexing="ij")
    a = (rr * (n_theta + 1) + tt).reshape(-1)
    b, c, d = a + 1, a + n_theta + 1, a + n_theta + 2
    ft = np.stack([np.stack([a, b, c], -1), np.stack([b, d, c], -1)], 1).reshape(-1, 3).astype(np.int32)      # garment.cylinder's face order
    return verts, faces, vt, ft


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map", type=int, default=256)
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ao_bench.py measures on the GPU; there is none")
    dev = torch.device("cuda:0")
    verts_h, faces, vt, ft = wrinkled_cylinder()
    verts = torch.as_tensor(verts_h, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    baker = AOBaker(torch.as_tensor(faces, device=dev), vt, ft, height=a.map, width=a.map, samples=a.samples)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    out = torch.empty(a.map, a.map, device=dev)
    first = baker.bake(verts, out=out).clone()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    stages = {"bake": lambda: baker.bake(verts, out=out), "grid": lambda: baker.build_grid(verts), "trace": lambda: baker.trace(verts),
              "margin": lambda: baker.add_margin(out)}
    for _ in range(a.warmup):
        for fn in stages.values():
            fn()
    times = {k: [] for k in stages}
    for _ in range(a.reps):
        for k, fn in stages.items():
            times[k].append(event_ms(fn))
    again = baker.bake(verts)
    covered = baker.coverage[0] >= 0
    res = {"faces": int(faces.shape[0]), "map": [a.map, a.map], "samples": a.samples, "covered_texels": int(baker.n_covered),
           "rays": int(baker.n_covered) * a.samples, "margin_pixels": baker.margin, "cap_cells": baker.cap_cells, "cap_entries": baker.cap_entries,
           "scratch_bytes": int(baker._scratch.numel()), "warmup": a.warmup, "reps": a.reps,
           "constructor_ms": (t1 - t0) * 1e3, "first_bake_ms": (t2 - t1) * 1e3,
           "mean_ao": float(first[covered].mean()), "fully_open_texels": float((first[covered] == 1.0).float().mean()),
           "finite": bool(torch.isfinite(first).all()), "same_bits_twice": bool(torch.equal(first, again))}
    for k, ts in times.items():
        res[k] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}
    res["rays_per_second"] = res["rays"] / (res["trace"]["median_ms"] * 1e-3)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
