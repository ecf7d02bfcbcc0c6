#!/usr/bin/env python
"""Time forward + backward of the regularisation terms of the appearance loop (train_appearance.py:136-150) -- the three mesh terms
on verts and the three Gaussian terms on _opacity, _xyz, _scaling -> a weighted sum -> backward() -- at the size of
tools/shade_bench.py and tools/binding_bench.py: 200,000 Gaussians, and the mesh of the 200 x 200 cylinder (about 80,000 faces).  Two
statements of the same function on the same device in one run, alternating:

  ours    mpmavatar_amd.regularizers under autograd (csrc/reg.hip: two launches forward and two backward for the mesh, two forward
          and one backward for the Gaussians)
  torch   the float32 torch expression of the reference under torch's own autograd, restated below -- which is what a user had to
          run before these kernels existed; its index_put_ backward uses floating-point atomics

    python tools/reg_bench.py [--gaussians 200000] [--warmup 10] [--reps 50] [--out file.json]
    python tools/reg_bench.py --only ours --reps 30 --warmup 0        # nothing but that many steps of one side, for a kernel trace

Each repetition is timed between two HIP events on torch's current stream; reported are the median, the minimum and the maximum per
statement and per op, the agreement of the values and gradients, whether two runs of each side give the same bits, and the
algorithmic bytes of our launches.  "faster" is claimed only where our maximum is below torch's minimum.  Launches per step are
counted outside this script: the difference of the dispatch counts of two kernel traces of ``--only`` runs with different ``--reps``."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.nn.functional as F

from mpmavatar_amd import garment
from mpmavatar_amd.regularizers import MeshRegularizer, gaussian_terms

WEIGHTS = (0.1, 20.0, 1000.0, 0.05, 1.0, 1.0)        # normal, iso, eq_faces_weight, opacity, xyz, scale (train_appearance.py:87)
T_XYZ, T_SCALE = 1.0, 0.6


def torch_mesh(verts, faces, nb, nd, nw):
    t = verts[faces]
    d3 = torch.linalg.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    n = d3 / d3.norm(dim=1, keepdim=True)
    normal = ((n.unsqueeze(1) * n[nb]).sum(-1).mean(-1) - 1.0).abs().mean()
    c = verts[faces].mean(dim=1)
    mag = torch.sqrt(((c[nb] - c[:, None]) ** 2).sum(-1) + 1e-20)
    iso = torch.sqrt((mag - nd) ** 2 * nw + 1e-20).mean()
    t = verts[faces]
    a = 0.5 * torch.norm(torch.linalg.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), dim=1)
    return torch.stack([normal, iso, (a - a.mean()).abs().mean()])


def torch_gauss(opacity, xyz, scaling, vis):
    return torch.stack([(1.0 - torch.sigmoid(opacity)).mean(), F.relu(xyz[vis].norm(dim=1) - T_XYZ).mean(),
                        F.relu(torch.exp(scaling[vis]) - T_SCALE).norm(dim=1).mean()])


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
    ap.add_argument("--only", choices=("ours", "torch"), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("reg_bench.py measures on the GPU; there is none")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    v, f = garment.cylinder(200, 200, 0.25, 0.8, (1.0, 1.0, 1.0))
    v, n = np.asarray(v, np.float32), a.gaussians
    f32 = lambda x: torch.tensor(np.asarray(x, np.float32), device=dev)
    spacing = float(np.linalg.norm(v[f[:, 0]] - v[f[:, 1]], axis=1).mean())
    verts0 = f32(v)
    reg = MeshRegularizer(torch.tensor(np.asarray(f, np.int32), device=dev), verts0)
    n_f, n_v = reg.n_faces, reg.n_verts
    leaves = {"verts": f32(v + rng.normal(0, 0.1 * spacing, v.shape)), "_opacity": f32(rng.normal(0, 2, (n, 1))),
              "_xyz": f32(rng.normal(0, 0.8, (n, 3))), "_scaling": f32(rng.normal(-0.9, 0.5, (n, 3)))}
    for t in leaves.values():
        t.requires_grad_(True)
    radii = torch.tensor(rng.integers(0, 4, n).astype(np.int32), device=dev)
    vis, faces64, nb64 = radii > 0, reg.faces.long(), reg.face_neighbors.long()
    w = torch.tensor(WEIGHTS, device=dev)

    forward = {
        "ours": {"mesh": lambda: reg.terms(leaves["verts"]),
                 "gauss": lambda: gaussian_terms(leaves["_opacity"], leaves["_xyz"], leaves["_scaling"], radii, T_XYZ, T_SCALE)},
        "torch": {"mesh": lambda: torch_mesh(leaves["verts"], faces64, nb64, reg.neighbor_dist, reg.neighbor_weight),
                  "gauss": lambda: torch_gauss(leaves["_opacity"], leaves["_xyz"], leaves["_scaling"], vis)}}

    def step(who, ops=("mesh", "gauss")):
        for t in leaves.values():
            t.grad = None
        sum((w[3 * (op == "gauss"):][:3] * forward[who][op]()).sum() for op in ops).backward()

    if a.only:
        for _ in range(a.warmup + a.reps):
            step(a.only)
        torch.cuda.synchronize()
        print(json.dumps({"only": a.only, "steps": a.warmup + a.reps}))
        return
    for _ in range(a.warmup):
        for who in forward:
            step(who)
    kinds = {"both": ("mesh", "gauss"), "mesh": ("mesh",), "gauss": ("gauss",)}
    times = {f"{who}_{kind}": [] for who in forward for kind in kinds}
    for _ in range(a.reps):                      # the two statements alternate, so that both see the same machine
        for kind, ops in kinds.items():
            for who in forward:
                times[f"{who}_{kind}"].append(event_ms(lambda: step(who, ops)))
    # algorithmic bytes of our launches (csrc/reg.hip): mesh forward 52 B per face + the 12 B vertices once, the finish reads the areas
    # again; mesh backward 48 B in and 144 B out per face, then 4 B per stencil item, the 144 B rows again and 12 B out per vertex;
    # Gaussians 32 B in forward, 32 B in and 28 B out backward
    mesh_bytes = n_f * (52 + 4) + n_v * 12 + n_f * (48 + 144) + n_f * (48 + 144) + n_v * 12
    gauss_bytes = n * 32 + n * 60
    res = {"gaussians": n, "faces": n_f, "verts": n_v, "warmup": a.warmup, "reps": a.reps,
           "algorithmic_bytes": {"mesh": mesh_bytes, "gauss": gauss_bytes}}
    for k, ts in times.items():
        res[k] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}
    for kind in kinds:
        res[f"speedup_{kind}"] = res[f"torch_{kind}"]["median_ms"] / res[f"ours_{kind}"]["median_ms"]
        res[f"faster_{kind}"] = res[f"ours_{kind}"]["max_ms"] < res[f"torch_{kind}"]["min_ms"]      # our worst against torch's best
    grads, same = {}, {}
    for who in forward:
        step(who)
        grads[who] = {k: t.grad.clone() for k, t in leaves.items()}
        step(who)
        same[who] = all(torch.equal(grads[who][k], t.grad) for k, t in leaves.items())
    res["same_bits_twice"] = same
    with torch.no_grad():
        mine, ref = [torch.cat([forward[who]["mesh"](), forward[who]["gauss"]()]) for who in ("ours", "torch")]
    res["terms"] = {"ours": mine.tolist(), "torch": ref.tolist()}
    res["grad_rel_diff"] = {k: float((grads["ours"][k] - grads["torch"][k]).abs().max() / grads["torch"][k].abs().max()) for k in leaves}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
