#!/usr/bin/env python
"""Time the optimiser step of the appearance loop (train_appearance.py:260) at the reference's size: 200,000 Gaussians with R = 15
(59 trained floats each, 45 of them in the f_rest group whose lr is 0), 40,000 x 3 vertex offsets, two camera tensors and 50 small
tensors standing in for the shadow network, in the reference's nine groups with its default rates.  Three statements of the same
step on the same device in one run, alternating:

  ours         mpmavatar_amd.optim.FusedAdam (csrc/adam.hip: one launch per 48 tensors)
  torch        torch.optim.Adam(l, lr=0.0, eps=1e-15) as the reference constructs it: torch's default path
  torch_fused  the same with fused=True

    python tools/optim_bench.py [--gaussians 200000] [--warmup 10] [--reps 50] [--out file.json] [--variant NAME]
    python tools/optim_bench.py --only ours --reps 30 --warmup 0       # nothing but that many steps of one side, for a kernel trace
    python tools/optim_bench.py --build-variants                       # compile the kernel alternatives (no GPU needed)

Each repetition is timed between two HIP events on torch's current stream; reported are the median, the minimum and the maximum per
statement, the host wall-time of a step() call that is not followed by a synchronisation, the device time of our launch alone
(--batch calls of mpmhip_adam_step back to back between two events: a step() is bound by its host side) with the achieved GB/s
against the algorithmic bytes (28 B per element, 20 B where lr == 0), and the agreement of the three results after the same number
of steps.
"faster" is claimed only where our maximum is below the other side's minimum.  --variant NAME runs ours from
mpmavatar_amd/lib/variants/libmpmhip_NAME.so, another build of csrc/adam.hip (VARIANTS below): grid cap and loads in flight."""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = {"nocap": ["-DMPMHIP_ADAM_GRID_CAP=0"], "acc2": ["-DMPMHIP_ADAM_ACCESSES=2"], "acc8": ["-DMPMHIP_ADAM_ACCESSES=8"],
            "acc2_nocap": ["-DMPMHIP_ADAM_ACCESSES=2", "-DMPMHIP_ADAM_GRID_CAP=0"], "cap1024": ["-DMPMHIP_ADAM_GRID_CAP=1024"]}
# arguments/__init__.py:115-126
OPT = SimpleNamespace(position_lr_init=0.00004, position_lr_final=0.00004, position_lr_delay_mult=0.01, position_lr_max_steps=30_000,
                      verts_lr_init=0.0, verts_lr_final=0.0, verts_lr_delay_mult=0.01, verts_lr_max_steps=30_000, feature_lr=0.0025,
                      opacity_lr=0.05, scaling_lr=0.005, rotation_lr=0.001)
SIDES = ("ours", "torch", "torch_fused")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=200000)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--only", choices=SIDES, default=None)
    ap.add_argument("--variant", choices=sorted(VARIANTS), default=None)
    ap.add_argument("--build-variants", action="store_true")
    ap.add_argument("--batch", type=int, default=20, help="launches between two events in the launch-alone measurement")
    ap.add_argument("--launch-only", action="store_true", help="print the launch-alone measurement and stop (for --variant runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.build_variants:
        from mpmavatar_amd import build as hipbuild
        for name, flags in VARIANTS.items():
            print(hipbuild.build_variant(name, flags, every=True, only=["adam.hip"]))
        return
    if a.variant:
        os.environ["MPMHIP_LIB"] = os.path.join(ROOT, "mpmavatar_amd", "lib", "variants", f"libmpmhip_{a.variant}.so")
    import numpy as np
    import torch

    from mpmavatar_amd.optim import FusedAdam, appearance_param_groups, update_learning_rate
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench.py measures on the GPU; there is none")
    dev = torch.device("cuda:0")
    n = a.gaussians
    shapes = [(n, 3), (n, 1, 3), (n, 15, 3), (n, 1), (n, 3), (n, 4), (40000, 3), (160, 3), (160, 3)]
    shapes += [((16, 64, 576, 128, 4608, 256, 36864, 32, 9216, 1)[i % 10],) for i in range(50)]
    gen = torch.Generator(device=dev).manual_seed(0)
    start = [torch.randn(s, device=dev, generator=gen) for s in shapes]
    grads = [torch.randn(s, device=dev, generator=gen) * 1e-3 for s in shapes]
    for g in grads[:6]:
        g[torch.rand(n, device=dev, generator=gen) < 0.5] = 0                         # the Gaussians a view does not see

    def make(side):
        leaves = [torch.nn.Parameter(t.clone()) for t in start]
        groups = appearance_param_groups(*leaves[:7], leaves[7:9], leaves[9:], OPT, 1.0)
        opt = FusedAdam(groups, lr=0.0, eps=1e-15) if side == "ours" else torch.optim.Adam(groups, lr=0.0, eps=1e-15, fused=side == "torch_fused")
        for p, g in zip(leaves, grads):
            p.grad = g
        return opt, leaves

    sides = {s: make(s) for s in ((a.only,) if a.only else SIDES)}
    count = [0]

    def step(side):
        update_learning_rate(sides[side][0], count[0] // len(sides) + 1)
        sides[side][0].step()
        count[0] += 1

    if a.only:
        for _ in range(a.warmup + a.reps):
            step(a.only)
        torch.cuda.synchronize()
        print(json.dumps({"only": a.only, "variant": a.variant, "steps": a.warmup + a.reps}))
        return
    for _ in range(a.warmup):
        for s in sides:
            step(s)
    times, host = {s: [] for s in sides}, {s: [] for s in sides}
    for _ in range(a.reps):                                  # the statements alternate, so that all see the same machine
        for s in sides:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            t0 = time.perf_counter()
            step(s)
            host[s].append((time.perf_counter() - t0) * 1e3)  # the call has returned; nothing has waited for the device
            e1.record()
            e1.synchronize()
            times[s].append(e0.elapsed_time(e1))
    rates = {g["name"]: float(g["lr"]) for g in sides["ours"][0].param_groups}
    nbytes = sum(p.numel() * (28 if rates[g["name"]] != 0 else 20) for g in sides["ours"][0].param_groups for p in g["params"])
    res = {"gaussians": n, "tensors": len(shapes), "elements": sum(t.numel() for t in start), "warmup": a.warmup, "reps": a.reps,
           "variant": a.variant, "algorithmic_bytes": nbytes, "device": torch.cuda.get_device_name(0)}
    for s in sides:
        res[s] = {"median_ms": statistics.median(times[s]), "min_ms": min(times[s]), "max_ms": max(times[s]),
                  "host_median_ms": statistics.median(host[s]), "host_min_ms": min(host[s]), "host_max_ms": max(host[s])}
    for s in SIDES[1:]:
        res[f"speedup_vs_{s}"] = res[s]["median_ms"] / res["ours"]["median_ms"]
        res[f"faster_than_{s}"] = res["ours"]["max_ms"] < res[s]["min_ms"]                 # our worst against its best
    # agreement after the same number of steps from the same start: parameters and both moments, max |a - b| / max |b| per tensor
    def state(side):
        opt, leaves = sides[side]
        return [(p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]) for p in leaves]
    mine = state("ours")
    for s in SIDES[1:]:
        worst = [0.0, 0.0, 0.0]
        for x, y in zip(mine, state(s)):
            for k in range(3):
                top = float(y[k].abs().max())
                worst[k] = max(worst[k], float((x[k] - y[k]).abs().max()) / (top if top > 0 else 1.0))
        res[f"rel_diff_vs_{s}"] = dict(zip(("param", "exp_avg", "exp_avg_sq"), worst))
    res["steps_each"] = count[0] // len(sides)
    # The launch alone: a step() is bound by its host side (host_median_ms), so the device time of the kernel is taken from
    # `batch` calls of mpmhip_adam_step with the same arguments, back to back between two events, per call
    from mpmavatar_amd import optim as O
    from mpmavatar_amd._call import call
    with torch.no_grad():
        (kdev, rows), = sides["ours"][0]._rows().items()
    args, keep = O.pack(rows)
    launch = []
    for rep in range(a.warmup + a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.batch):
            call("mpmhip_adam_step", kdev, *args)
        e1.record()
        e1.synchronize()
        if rep >= a.warmup:
            launch.append(e0.elapsed_time(e1) / a.batch)
    res["ours_launch"] = {"batch": a.batch, "median_ms": statistics.median(launch), "min_ms": min(launch), "max_ms": max(launch),
                          "GBps_at_median": nbytes / (statistics.median(launch) * 1e-3) / 1e9, "GBps_at_min": nbytes / (min(launch) * 1e-3) / 1e9}
    if a.launch_only:
        print(json.dumps({"variant": a.variant, "ours_launch": res["ours_launch"]}))
        return
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
