#!/usr/bin/env python
"""Time the densification block of the appearance loop (train_appearance.py:245-257) at the size of tools/reg_bench.py: 200,000
Gaussians bound to 79,600 faces, SH degree 3 (R = 15), Adam moments for all six parameters.  Two statements of the same procedure on
the same device in one run, alternating:

  ours    mpmavatar_amd.densify (csrc/densify.hip): DensifyStats.add, one launch; densify_and_prune, one read-back
  torch   the reference's procedure restated in torch (tests/densify_twin_torch.py, float32): three boolean-indexed updates per
          iteration; clone, split and two prune_points with their nonzero()s, bincounts and re-concatenations per densification --
          what a caller had to run before these kernels existed

    python tools/densify_bench.py [--gaussians 200000] [--faces 79600] [--warmup 5] [--reps 30] [--out file.json]

stats.add is timed between two HIP events on torch's current stream; densify_and_prune synchronises by design, so it is timed with
the host clock from the call to a device synchronise after it.  Reported are the median, the minimum and the maximum per statement,
the synchronising torch calls each makes (torch's sync debug mode) and the device kernels each launches (torch's profiler, where it
is available), whether both give the same rows (src, kind, binding exactly, children within 1e-5), and whether two runs of ours
give the same bits.  "faster" is claimed only where our maximum is below torch's minimum."""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import densify_twin_torch as tw
from mpmavatar_amd.densify import PARAMS, DensifyStats, densify_and_prune

HYPER = dict(max_grad=0.0002, min_opacity=0.005, extent=2.0, max_screen_size=20, percent_dense=0.01)


def scene(n, n_f, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)
    uni = lambda *s: torch.rand(*s, device=dev, generator=g)
    fs = 0.02 + 0.06 * uni(n_f, 1)
    binding = torch.cat([torch.arange(n_f, device=dev), torch.randint(0, n_f, (n - n_f,), device=dev, generator=g)]).to(torch.int32)
    world = 0.02 * torch.exp(0.8 * rnd(n, 1)) * (0.2 + 0.8 * uni(n, 3))
    p = {"_xyz": 0.5 * rnd(n, 3), "_features_dc": rnd(n, 1, 3), "_features_rest": 0.1 * rnd(n, 15, 3), "_opacity": 2.0 * rnd(n, 1) - 1.0,
         "_scaling": torch.log(world / fs[binding.long()]), "_rotation": rnd(n, 4)}
    moments = {k: (0.01 * rnd(*v.shape), 1e-4 * uni(*v.shape)) for k, v in p.items()}
    denom = torch.randint(0, 6, (n, 1), device=dev, generator=g).float()
    accum = denom * 0.0002 * torch.exp(0.7 * rnd(n, 1))
    radii = torch.randint(0, 12, (n,), device=dev, generator=g).to(torch.int32) * (uni(n) > 0.3)
    return dict(params=p, moments=moments, binding=binding, fs=fs, accum=accum, denom=denom, noise=rnd(n, 2, 3), grad=1e-3 * rnd(n, 3),
                radii=radii.to(torch.int32), n_faces=n_f)


def ours_densify(s):
    stats = DensifyStats(s["binding"].shape[0], s["binding"].device)
    stats.xyz_gradient_accum, stats.denom = s["accum"].clone(), s["denom"].clone()
    return densify_and_prune(*[s["params"][k] for k in PARAMS], s["binding"], s["n_faces"], s["fs"], stats, HYPER["max_grad"], HYPER["min_opacity"],
                             HYPER["extent"], HYPER["max_screen_size"], HYPER["percent_dense"], moments=s["moments"], noise=s["noise"])


def torch_densify(s):
    return tw.densify_and_prune(s["params"], s["moments"], s["binding"].long(), s["n_faces"], s["fs"], s["accum"], s["denom"], s["noise"], **HYPER)


def torch_stats_add(accum, denom, max_radii, grad, radii):
    """train_appearance.py:248 and add_densification_stats as the reference writes them: in place, three boolean-indexed updates"""
    vis = radii > 0
    max_radii[vis] = torch.max(max_radii[vis], radii[vis].float())
    accum[vis] += torch.norm(grad[vis, :2], dim=-1, keepdim=True)
    denom[vis] += 1


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def synchronisations(fn):
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    return sum("synchronizing" in str(w.message).lower() and "prototype" not in str(w.message) for w in caught)


def kernels(fn):
    """device kernels (memsets and copies not counted) of one call, or None where the profiler sees none"""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA") and not e.name.lower().startswith(("memcpy", "memset"))]
        return len(names) or None
    except Exception:
        return None


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=200000)
    ap.add_argument("--faces", type=int, default=79600)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    s = scene(a.gaussians, a.faces, dev)
    n = a.gaussians
    stats = DensifyStats(n, dev)
    t_stats = [torch.zeros(n, 1, device=dev), torch.zeros(n, 1, device=dev), torch.zeros(n, device=dev)]
    sides = {"stats_add": {"ours": lambda: stats.add(s["grad"], s["radii"]), "torch": lambda: torch_stats_add(*t_stats, s["grad"], s["radii"])},
             "densify_and_prune": {"ours": lambda: ours_densify(s), "torch": lambda: torch_densify(s)}}
    out = {"gaussians": n, "faces": a.faces, "features_rest_rows": 15, "hyper": HYPER, "device": torch.cuda.get_device_name(0)}
    for op, pair in sides.items():
        timer = event_ms if op == "stats_add" else host_ms
        for _ in range(a.warmup):
            for fn in pair.values():
                fn()
        ms = {k: [] for k in pair}
        for _ in range(a.reps):
            for k, fn in pair.items():                    # alternating
                ms[k].append(timer(fn))
        out[op] = {k: dict(spread(v), synchronising_calls=synchronisations(pair[k]), kernels=kernels(pair[k])) for k, v in ms.items()}
        out[op]["faster"] = out[op]["ours"]["max_ms"] < out[op]["torch"]["min_ms"]
    # the same rows from both, and the same bits twice from ours
    r, again, t = ours_densify(s), ours_densify(s), torch_densify(s)
    out["rows"] = {"n_out": r.n_out, "n_cloned": r.n_cloned, "n_split": r.n_split, "n_pruned": r.n_pruned}
    same = all(torch.equal(getattr(r, k), t[k].to(torch.int32)) for k in ("src", "kind", "binding")) and \
        (r.n_out, r.n_cloned, r.n_split, r.n_pruned) == tuple(t["counts"])
    close = max(float((getattr(r, k) - t[k]).abs().max()) for k in PARAMS if t[k].numel())
    out["agreement"] = {"rows_identical": bool(same), "max_abs_difference": close,
                        "ours_same_bits_twice": all(torch.equal(getattr(r, k), getattr(again, k)) for k in PARAMS + ("src", "kind", "binding"))}
    stats.reset(n)
    for st in t_stats:
        st.zero_()
    stats.add(s["grad"], s["radii"])
    torch_stats_add(*t_stats, s["grad"], s["radii"])
    out["agreement"]["stats_max_abs_difference"] = max(float((x - y).abs().max()) for x, y in zip((stats.xyz_gradient_accum, stats.denom, stats.max_radii2D), t_stats))
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
