#!/usr/bin/env python
"""Time re-posing (mpmavatar_amd.reposing, csrc/repose.hip, csrc/knn_device.hpp) against torch expressions on the same device, the two
statements alternating in one process:

  (a) pose      ``transform_to_pose`` into all test frames at once (train_material_params.py:343-349) against the reference's lines with
                their ``repeat`` of the weights and the vertices; with the peak allocation of both sides
  (b) t_pose    ``transform_to_t_pose`` with ``lbs_w=None`` (train_mesh_lbs_actorshq.py:511): the 6-D search with k = 10, Shepard's
                weights, the gather and the inverse skinning.  The reference searches with pytorch3d's knn_points, which is not
                installed; the torch side here uses ``torch.cdist`` + ``topk`` instead, which is NOT what the reference runs
  (c) knn_self  ``knn_self(pts, 4)`` (o3d_knn(init_bary, 4), a host loop over an open3d KD-tree in the reference) against ``torch.cdist``
                + ``topk`` on the device, again not what the reference runs

    python tools/repose_bench.py [--frames 199] [--points 20301] [--joints 55] [--cloth 15000] [--body 10475] [--self 40000]
                                 [--warmup 5] [--reps 30] [--out file.json] [--md file.md]

The reference's data is not available to this tool, so the sizes are ASSUMPTIONS: 199 test frames, a garment of 20,301 vertices,
SMPL-X's 55 joints and 10,475 vertices, 15,000 tracked human vertices, 40,000 face barycentres.

Each repetition is timed between two HIP events on torch's current stream, after the warm-up of both sides; reported are the minimum,
the median and the maximum per statement, and the agreement of the two results.  "faster" is claimed only where our maximum is below
torch's minimum; every row is reported, including any that is not faster.  No ratio is a pass condition."""
import argparse
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


# ---- the torch side ----------------------------------------------------------------------------------------------------------------------

def torch_to_pose(torch, vertices, lbs_w, A, transl, scale):
    """utils/smplx_deformer.py:303-337 on vertices [P, 3] and lbs_w [P, J], with the repeats of train_material_params.py:344-345"""
    B, J = A.shape[0], A.shape[1]
    v, W = vertices.repeat(B, 1, 1), lbs_w.repeat(B, 1, 1)
    P = W.shape[1]
    T = torch.matmul(W, A.reshape((-1, B, J, 16))).reshape((-1, B, P, 4, 4))
    src = v.reshape((-1, B, P, 3))
    homo = torch.cat([src, torch.ones_like(src[..., :1])], dim=-1)
    out = torch.matmul(T, homo.unsqueeze(-1))[..., :3, 0]
    out += transl.unsqueeze(1)
    out *= scale.unsqueeze(1).unsqueeze(2)
    return out, T


def torch_knn(torch, a, b, k):
    d, i = torch.cdist(a, b).topk(k, dim=1, largest=False)
    return d * d, i


def torch_to_tpose(torch, vertices, normals, body, body_normals, lbs, A, transl, scale, k, normal_weight=0.1):
    """utils/smplx_deformer.py:229-288 for one frame, the search replaced by cdist + topk"""
    a, b = torch.cat([vertices, normal_weight * normals], -1), torch.cat([body, normal_weight * body_normals], -1)
    d2, idx = torch_knn(torch, a, b, k)
    w = torch.pow(torch.clamp(d2, min=1e-8), -2)
    w = w / w.sum(-1, keepdim=True)
    W = torch.einsum("pkj,pk->pj", lbs[idx], w)[None]
    P, J = W.shape[1], A.shape[1]
    T = torch.inverse(torch.matmul(W, A.reshape((-1, 1, J, 16))).reshape((-1, 1, P, 4, 4)))
    v = (vertices[None] / scale - transl.unsqueeze(1)).reshape((-1, 1, P, 3))
    homo = torch.cat([v, torch.ones_like(v[..., :1])], dim=-1)
    return torch.matmul(T, homo.unsqueeze(-1))[..., :3, 0], T, W


def torch_knn_self(torch, p, k):
    d2, idx = torch_knn(torch, p, p, k + 1)
    return d2[:, 1:], idx[:, 1:]


def unit(rng, n):
    import numpy as np
    p = rng.normal(0, 1, (n, 3))
    return p / np.linalg.norm(p, axis=1, keepdims=True)


def inputs(rng, frames, joints, points, body):
    """-> A [frames, J, 4, 4] (rotations of up to 30 degrees along a chain), lbs [body, J] and W [points, J] (four joints a row)"""
    import numpy as np
    A = np.zeros((frames, joints, 4, 4))
    for b in range(frames):
        for j in range(joints):
            axis, angle = unit(rng, 1)[0], rng.uniform(-np.pi / 6, np.pi / 6)
            k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
            local = np.eye(4)
            local[:3, :3] = np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * k @ k
            local[:3, 3] = rng.normal(0, 0.3, 3)
            A[b, j] = local if j == 0 else A[b, max(0, j - 1 - int(rng.integers(0, 3)))] @ local
    def rows(n):
        W = np.zeros((n, joints))
        main = rng.integers(0, joints, n)
        share = rng.dirichlet((6.0, 2.0, 1.0, 0.5), n)
        for c in range(4):
            np.add.at(W, (np.arange(n), np.maximum(main - c, 0)), share[:, c])
        return W
    return A, rows(body), rows(points)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=199)
    ap.add_argument("--points", type=int, default=20301)
    ap.add_argument("--joints", type=int, default=55)
    ap.add_argument("--cloth", type=int, default=15000)
    ap.add_argument("--body", type=int, default=10475)
    ap.add_argument("--self", dest="self_points", type=int, default=40000)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("repose_bench: no GPU; a timing needs the device")
    from mpmavatar_amd.reposing import Reposer, knn_self
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    t = lambda x: torch.tensor(np.asarray(x, np.float32), device=dev)
    A_np, lbs_np, W_np = inputs(rng, a.frames, a.joints, a.points, a.body)
    A, lbs, W = t(A_np), t(lbs_np), t(W_np)
    verts = t(rng.normal(0, 0.5, (a.points, 3)))
    transl, scale = t(rng.normal(0, 0.5, (a.frames, 3))), t(rng.uniform(0.9, 1.1, a.frames))
    body_n = unit(rng, a.body)
    body = 0.5 * body_n + rng.normal(0, 0.01, (a.body, 3))
    pick = rng.integers(0, a.body, a.cloth)
    cloth, cloth_n = body[pick] + rng.normal(0, 0.02, (a.cloth, 3)), body_n[pick]
    body, body_n, cloth, cloth_n = t(body), t(body_n), t(cloth), t(cloth_n)
    pts = t(rng.uniform(0, 1, (a.self_points, 3)))
    rp = Reposer(lbs)
    all_frames = types.SimpleNamespace(transform_mat=A)
    one_frame = types.SimpleNamespace(transform_mat=A[:1].contiguous(), vertices=body[None])
    s0 = scale[0].clone()

    def run_pose(side):
        if side == "ours":
            return [rp.transform_to_pose(verts, W[None], all_frames, transl, scale, with_T=False)[0]]
        return [torch_to_pose(torch, verts, W, A, transl, scale)[0]]

    def run_pose_T(side):
        if side == "ours":
            return list(rp.transform_to_pose(verts, W[None], all_frames, transl, scale))
        return list(torch_to_pose(torch, verts, W, A, transl, scale))

    def run_tpose(side):
        if side == "ours":
            return list(rp.transform_to_t_pose(cloth[None], one_frame, transl[:1], s0, k=10, v_normals=cloth_n[None], smplx_normals=body_n[None]))
        return list(torch_to_tpose(torch, cloth, cloth_n, body, body_n, lbs, A[:1], transl[:1], s0, 10))

    def run_self(side):
        return list(knn_self(pts, 4) if side == "ours" else torch_knn_self(torch, pts, 4))

    ops = {"(a) transform_to_pose, points only": run_pose, "(a) transform_to_pose, points and T": run_pose_T,
           "(b) transform_to_t_pose, lbs_w=None": run_tpose, "(c) knn_self, k = 4": run_self}
    result = {"assumed_sizes": {"frames": a.frames, "points": a.points, "joints": a.joints, "tracked_vertices": a.cloth, "body_vertices": a.body,
                                "self_points": a.self_points}, "warmup": a.warmup, "reps": a.reps, "device": torch.cuda.get_device_name(0), "ops": {}}
    print("sizes (ASSUMED, the reference's data is not available):", json.dumps(result["assumed_sizes"]))
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
        peak = {}
        for side in ("ours", "torch"):                                              # what one call allocates on top of its inputs
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            out = run(side)
            torch.cuda.synchronize()
            peak[side] = torch.cuda.max_memory_allocated() - before
            del out
        mine, theirs, again = run("ours"), run("torch"), run("ours")
        diff = []
        for x, y in zip(mine, theirs):
            if x.dtype == torch.int64:
                diff.append(float((x.reshape(y.shape) != y).float().mean()))         # the share of neighbour entries that differ
            else:
                diff.append(float((x.reshape(y.shape) - y).abs().max() / y.abs().max().clamp(min=1e-30)))
        stat = {side: {"min": min(ts), "median": statistics.median(ts), "max": max(ts)} for side, ts in times.items()}
        result["ops"][name] = {"ms": stat, "peak_bytes": peak, "difference_to_torch": diff,
                               "same_bits_twice": all(torch.equal(x, y) for x, y in zip(mine, again)), "faster": stat["ours"]["max"] < stat["torch"]["min"]}
        print(name, json.dumps(result["ops"][name]))
        del mine, theirs, again
    lines = ["| milliseconds (min / median / max) | ours | torch | median ratio | our max below torch's min | peak allocation of one call, ours / torch |",
             "|---|---|---|---|---|---|"]
    for name, r in result["ops"].items():
        o, p = r["ms"]["ours"], r["ms"]["torch"]
        lines.append(f"| {name} | {o['min']:.4f} / **{o['median']:.4f}** / {o['max']:.4f} | {p['min']:.4f} / **{p['median']:.4f}** / {p['max']:.4f} | "
                     f"{p['median'] / o['median']:.2f} x | {'yes' if r['faster'] else 'no'} | "
                     f"{r['peak_bytes']['ours'] / 2 ** 20:.1f} MiB / {r['peak_bytes']['torch'] / 2 ** 20:.1f} MiB |")
    table = "\n".join(lines)
    print(table)
    for path, text in ((a.out, json.dumps(result, indent=1)), (a.md, table + "\n")):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
