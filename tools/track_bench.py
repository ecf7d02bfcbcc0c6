#!/usr/bin/env python
"""Time the three ops of the mesh tracking step (mpmavatar_amd.tracking, csrc/track.hip) against the same expressions written in
torch on the same device: ``render_vars`` (params2rendervar), ``terms`` (area, scale, opacity) and ``collision_penalty``, each
forward + backward, the two statements alternating in one process.

    python tools/track_bench.py [--faces 40000] [--cloth 15000] [--body 10475] [--warmup 10] [--reps 50] [--out file.json] [--md file.md]

The reference's data is not available to this tool, so the sizes are ASSUMPTIONS: a body of SMPL-X's 10,475 vertices, a mesh of about
40,000 faces (a sheet of 100 x 200 quads: 40,000 faces, 20,301 vertices) and about 15,000 cloth vertices.  The torch side is the
reference's expressions (tests/track_twin_torch.py is the same text in float64): pytorch3d's matrix_to_quaternion restated, and
collision_penalty with the full [n_cloth, n_body] distance matrix, as the reference materialises it on every iteration.

Each repetition is timed between two HIP events on torch's current stream, after the warm-up of both sides; reported are the minimum,
the median and the maximum per statement, and the agreement of the two results.  "faster" is claimed only where our maximum is below
torch's minimum; every op is reported, including any that is not faster.  No ratio is a pass condition."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sheet(nx, ny, h):
    import numpy as np
    i, j = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1))
    verts = np.stack([i.reshape(-1) * h, j.reshape(-1) * h, np.zeros(i.size)], 1)
    qi, qj = [a.reshape(-1) for a in np.meshgrid(np.arange(nx), np.arange(ny))]
    v00 = qj * (nx + 1) + qi
    faces = np.stack([np.stack([v00, v00 + 1, v00 + nx + 2], 1), np.stack([v00, v00 + nx + 2, v00 + nx + 1], 1)], 1).reshape(-1, 3)
    return verts, faces.astype(np.int32)


# ---- the torch side: the reference's expressions ------------------------------------------------------------------------------------

def torch_render_vars(torch, v, faces, ls, lo):
    v1, v2, v3 = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    e1, e2, e3 = v2 - v1, v3 - v2, v1 - v3
    n = torch.linalg.cross(e1, e2)
    n = n / n.norm(dim=1, keepdim=True)
    idx = torch.stack([e1.norm(dim=1), e2.norm(dim=1), e3.norm(dim=1)], 1).max(dim=1, keepdim=True).indices
    x = torch.where(idx == 0, e1, torch.where(idx == 1, e2, e3))
    x = x / x.norm(dim=1, keepdim=True)
    z = n / n.norm(dim=1, keepdim=True)
    y = torch.linalg.cross(z, x)
    y = y / y.norm(dim=1, keepdim=True)
    m = torch.stack([x, y, z], 2)
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = m.reshape(-1, 9).unbind(1)
    arg = torch.stack([1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22, 1.0 - m00 + m11 - m22, 1.0 - m00 - m11 + m22], 1)
    r = torch.zeros_like(arg)
    pos = arg > 0
    r[pos] = torch.sqrt(arg[pos])
    rows = torch.stack([torch.stack([r[:, 0] ** 2, m21 - m12, m02 - m20, m10 - m01], 1), torch.stack([m21 - m12, r[:, 1] ** 2, m10 + m01, m02 + m20], 1),
                        torch.stack([m02 - m20, m10 + m01, r[:, 2] ** 2, m12 + m21], 1), torch.stack([m10 - m01, m20 + m02, m21 + m12, r[:, 3] ** 2], 1)], 1)
    cand = rows / (2.0 * r[:, :, None].clamp(min=0.1))
    q = cand[torch.nn.functional.one_hot(r.argmax(dim=1), num_classes=4) > 0.5, :].reshape(-1, 4)
    q = torch.where(q[:, :1] < 0, -q, q)
    return (v1 + v2 + v3) / 3, q, torch.exp(ls), torch.sigmoid(lo)


def torch_terms(torch, v, faces, ls, lo):
    v1, v2, v3 = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    area = torch.linalg.cross(v2 - v1, v3 - v2).norm(dim=1) / 2
    s = torch.exp(ls)
    return torch.stack([(area - s[:, 0] * s[:, 1] * math.pi).abs().mean(), s[:, -1].mean(), (1 - torch.sigmoid(lo)).mean()])


def torch_collision(torch, va, vb, nb, eps=1e-3):
    d2 = -2 * torch.matmul(va, vb.transpose(-2, -1)) + (va ** 2).sum(-1).unsqueeze(-1) + (vb ** 2).sum(-1).unsqueeze(-2)
    j = torch.argmin(d2, dim=-1)
    d = torch.sum(-nb[j] * (va - vb[j]), dim=-1)
    return torch.sum(torch.maximum(eps - d, torch.tensor(0.0, device=va.device))) / va.shape[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, default=40000)
    ap.add_argument("--cloth", type=int, default=15000)
    ap.add_argument("--body", type=int, default=10475)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("track_bench: no GPU; a timing needs the device")
    from mpmavatar_amd.tracking import FaceGaussians, collision_penalty
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    ny = max(1, round(math.sqrt(a.faces / 4)))
    nx = max(1, a.faces // (2 * ny))
    h = 0.01
    verts, faces = sheet(nx, ny, h)
    verts = verts + rng.normal(0, 0.15 * h, verts.shape)
    n_f, n_v = faces.shape[0], verts.shape[0]
    t = lambda x: torch.tensor(np.asarray(x, np.float32), device=dev)
    faces_d = torch.tensor(faces, device=dev)
    faces_l = faces_d.long()
    ls = np.full((n_f, 3), -100.0)
    ls[:, :2] = 0.5 * math.log(0.5 * h * h / math.pi) + rng.normal(0, 0.4, (n_f, 2))
    v0, ls0, lo0 = t(verts), t(ls), t(rng.normal(0, 2, (n_f, 1)))
    w = [t(rng.normal(0, 1, s)) for s in ((n_f, 3), (n_f, 4), (n_f, 3), (n_f, 1))]
    w_terms = t([50.0, 1.0, 0.05])
    nb = rng.normal(0, 1, (a.body, 3))
    nb /= np.linalg.norm(nb, axis=1, keepdims=True)
    vb_np = 0.5 * nb
    va_np = vb_np[rng.integers(0, a.body, a.cloth)] * (1 + rng.uniform(-0.04, 0.04, (a.cloth, 1))) + rng.normal(0, 0.003, (a.cloth, 3))
    va0, vb, nbt = t(va_np), t(vb_np), t(nb)
    fg = FaceGaussians(faces_d)

    def leaves():
        return [x.clone().requires_grad_(True) for x in (v0, ls0, lo0)]

    def run_render(side):
        v, s, o = leaves()
        out = fg.render_vars(v, s, o) if side == "ours" else dict(zip(("means3D", "rotations", "scales", "opacities"), torch_render_vars(torch, v, faces_l, s, o)))
        sum((wk * out[k]).sum() for wk, k in zip(w, ("means3D", "rotations", "scales", "opacities"))).backward()
        return [out["rotations"].detach(), v.grad, s.grad, o.grad]

    def run_terms(side):
        v, s, o = leaves()
        terms = fg.terms(v, s, o) if side == "ours" else torch_terms(torch, v, faces_l, s, o)
        (w_terms * terms).sum().backward()
        return [terms.detach(), v.grad, s.grad, o.grad]

    def run_collision(side):
        va = va0.clone().requires_grad_(True)
        y = collision_penalty(va, vb, nbt) if side == "ours" else torch_collision(torch, va, vb, nbt)
        y.backward()
        return [y.detach(), va.grad]

    ops = {"render_vars": run_render, "terms": run_terms, "collision_penalty": run_collision}
    result = {"assumed_sizes": {"faces": n_f, "vertices": n_v, "cloth_vertices": a.cloth, "body_vertices": a.body}, "warmup": a.warmup, "reps": a.reps,
              "device": torch.cuda.get_device_name(0), "ops": {}}
    print(f"sizes (ASSUMED, the reference's data is not available): {n_f} faces, {n_v} vertices, {a.cloth} cloth x {a.body} body vertices")
    for name, run in ops.items():
        for _ in range(a.warmup):
            for side in ("ours", "torch"):
                run(side)
        torch.cuda.synchronize()
        times = {"ours": [], "torch": []}
        for _ in range(a.reps):
            for side in ("ours", "torch"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(side)
                e1.record()
                e1.synchronize()
                times[side].append(e0.elapsed_time(e1))
        mine, theirs = run("ours"), run("torch")
        again = run("ours")
        diff = [float((x - y).abs().max() / y.abs().max().clamp(min=1e-30)) for x, y in zip(mine, theirs)]
        stat = {side: {"min": min(ts), "median": statistics.median(ts), "max": max(ts)} for side, ts in times.items()}
        result["ops"][name] = {"ms": stat, "relative_difference_to_torch": diff, "same_bits_twice": all(torch.equal(x, y) for x, y in zip(mine, again)),
                               "faster": stat["ours"]["max"] < stat["torch"]["min"]}
        print(name, json.dumps(result["ops"][name]))
    lines = ["| forward + backward, milliseconds (min / median / max) | ours | torch | median ratio | our max below torch's min |", "|---|---|---|---|---|"]
    for name, r in result["ops"].items():
        o, p = r["ms"]["ours"], r["ms"]["torch"]
        lines.append(f"| `{name}` | {o['min']:.4f} / **{o['median']:.4f}** / {o['max']:.4f} | {p['min']:.4f} / **{p['median']:.4f}** / {p['max']:.4f} | "
                     f"{p['median'] / o['median']:.2f} x | {'yes' if r['faster'] else 'no'} |")
    table = "\n".join(lines)
    print(table)
    for path, text in ((a.out, json.dumps(result, indent=1)), (a.md, table + "\n")):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
