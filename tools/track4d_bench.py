#!/usr/bin/env python
"""Time the two terms the 4D-DRESS tracking script adds (mpmavatar_amd.tracking.MeshLaplacian and scale_ratio_loss, csrc/track4d.hip)
against torch on the same device, each forward + backward, the two statements alternating in one process:

    laplacian (dense)    lap.loss(v)  against the reference's line, laplacian_matrix.mm(v).norm(dim=1).mean() on the dense fp32 [V, V]
    laplacian (sparse)   lap.loss(v)  against the same matrix as a torch.sparse product: the fair baseline
    scale_ratio_loss     fg.scale_ratio_losses(v, scales), weights 10, 1000, 10, against the reference's expression

    python tools/track4d_bench.py [--warmup 10] [--reps 50] [--out file.json] [--md file.md]

The reference's data is not available to this tool, so the sizes are ASSUMPTIONS: the sheet of 100 x 200 quads that tools/track_bench.py
assumes (20,301 vertices, 40,000 faces) and the 181 x 182 sheet of the tests (33,306 vertices, 65,884 faces).  The matrix is this
project's restatement of pytorch3d's laplacian_packed (UNCONFIRMED against pytorch3d itself): 1 / deg off the diagonal, -1 on it.

Each repetition is timed between two HIP events on torch's current stream, after the warm-up of both sides; reported are the minimum,
the median and the maximum per statement, the agreement of the two results, and the device memory of each side: what it keeps (the
matrix or the adjacency table) and the peak of what one forward + backward allocates on top.  "faster" is claimed only where our
maximum is below the other side's minimum; every op is reported, including any that is not faster.  No ratio is a pass condition."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
SIZES = ((100, 200), (181, 182))
WEIGHTS = (10.0, 1000.0, 10.0)


def torch_scale_ratio(v, faces, scale, th_r=5.0, th_e=1.0):
    vf = v[faces]
    m = (vf - vf[:, [1, 2, 0]]).norm(dim=2).max(dim=1)[0]
    a, b = scale[:, :2].max(dim=1)[0], scale[:, :2].min(dim=1)[0]
    r, q = a / (b + 1e-8), a / (m + 1e-8)
    return (r.clamp(min=th_r) - th_r).mean(), (q.clamp(min=th_e) - th_e).mean(), q.var()


def nbytes(*tensors):
    return sum(t.numel() * t.element_size() for t in tensors)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("track4d_bench: no GPU; a timing needs the device")
    from track_bench import sheet
    from mpmavatar_amd.tracking import FaceGaussians, MeshLaplacian
    dev = torch.device("cuda:0")
    result = {"warmup": a.warmup, "reps": a.reps, "device": torch.cuda.get_device_name(0), "sizes": []}
    lines = ["| vertices / faces (ASSUMED) | forward + backward, ms (min / median / max) | ours | torch | median ratio | our max below torch's min | "
             "kept on the device, ours / torch | peak on top, ours / torch |", "|---|---|---|---|---|---|---|---|"]
    for nx, ny in SIZES:
        rng = np.random.default_rng(0)
        h = 0.01
        verts, faces = sheet(nx, ny, h)
        verts = verts + rng.normal(0, 0.15 * h, verts.shape)
        n_f, n_v = faces.shape[0], verts.shape[0]
        t = lambda x: torch.tensor(np.asarray(x, np.float32), device=dev)
        faces_d = torch.tensor(faces, device=dev)
        faces_l = faces_d.long()
        ls = 0.5 * np.log(0.5 * h * h / np.pi) + rng.normal(0, 1.0, (n_f, 3))
        v0, s0 = t(verts), t(np.exp(ls))
        fg, lap = FaceGaussians(faces_d), MeshLaplacian(faces_d)
        start, nbr = lap._adjacency(n_v)
        corner_start, corner_items = fg._table(n_v)
        row = torch.repeat_interleave(torch.arange(n_v, device=dev), (start[1:] - start[:-1]).long())
        deg = (start[1:] - start[:-1]).float()
        diag = torch.arange(n_v, device=dev)
        coo = torch.sparse_coo_tensor(torch.stack([torch.cat([row, diag]), torch.cat([nbr.long(), diag])]),
                                      torch.cat([1 / deg[row], -torch.ones(n_v, device=dev)]), (n_v, n_v)).coalesce()
        dense = coo.to_dense()
        try:
            sparse, layout = coo.to_sparse_csr(), "CSR"
            v = v0.clone().requires_grad_(True)
            sparse.mm(v).norm(dim=1).mean().backward()
        except Exception as e:                                                    # this torch cannot differentiate the CSR product
            sparse, layout = coo, "COO (CSR: %s)" % type(e).__name__
        sparse_kept = nbytes(sparse.crow_indices(), sparse.col_indices(), sparse.values()) if layout == "CSR" else nbytes(coo.indices(), coo.values())
        del coo
        print(f"sizes (ASSUMED, the reference's data is not available): {n_v} vertices, {n_f} faces; dense matrix {nbytes(dense)} bytes, "
              f"sparse {layout} {sparse_kept} bytes, adjacency table {nbytes(start, nbr)} bytes")

        def run_lap(matrix):
            def run(side):
                v = v0.clone().requires_grad_(True)
                y = lap.loss(v) if side == "ours" else matrix.mm(v).norm(dim=1).mean()
                y.backward()
                return [y.detach(), v.grad]
            return run

        def run_scale(side):
            v, s = v0.clone().requires_grad_(True), s0.clone().requires_grad_(True)
            terms = fg.scale_ratio_losses(v, s) if side == "ours" else torch_scale_ratio(v, faces_l, s)
            sum(w * y for w, y in zip(WEIGHTS, terms)).backward()
            return [torch.stack([y.detach() for y in terms]), v.grad, s.grad]

        ops = {"laplacian (dense mm, the reference's line)": (run_lap(dense), nbytes(start, nbr), nbytes(dense)),
               f"laplacian (torch.sparse {layout})": (run_lap(sparse), nbytes(start, nbr), sparse_kept),
               "scale_ratio_loss": (run_scale, nbytes(corner_start, corner_items), 0)}
        size = {"vertices": n_v, "faces": n_f, "ops": {}}
        for name, (run, kept_ours, kept_torch) in ops.items():
            for _ in range(a.warmup):
                for side in ("ours", "torch"):
                    run(side)
            torch.cuda.synchronize()
            times, peak = {"ours": [], "torch": []}, {}
            for _ in range(a.reps):
                for side in ("ours", "torch"):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    run(side)
                    e1.record()
                    e1.synchronize()
                    times[side].append(e0.elapsed_time(e1))
            for side in ("ours", "torch"):
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                out = run(side)
                torch.cuda.synchronize()
                peak[side] = torch.cuda.max_memory_allocated() - base
                del out
            mine, theirs = run("ours"), run("torch")
            again = run("ours")
            diff = [float((x - y).abs().max() / y.abs().max().clamp(min=1e-30)) for x, y in zip(mine, theirs)]
            stat = {side: {"min": min(ts), "median": statistics.median(ts), "max": max(ts)} for side, ts in times.items()}
            r = {"ms": stat, "relative_difference_to_torch": diff, "same_bits_twice": all(torch.equal(x, y) for x, y in zip(mine, again)),
                 "faster": stat["ours"]["max"] < stat["torch"]["min"], "bytes_kept": {"ours": kept_ours, "torch": kept_torch}, "peak_bytes_on_top": peak}
            size["ops"][name] = r
            print(name, json.dumps(r))
            o, p = stat["ours"], stat["torch"]
            lines.append(f"| {n_v} / {n_f} | `{name}` | {o['min']:.4f} / **{o['median']:.4f}** / {o['max']:.4f} | {p['min']:.4f} / **{p['median']:.4f}** / "
                         f"{p['max']:.4f} | {p['median'] / o['median']:.2f} x | {'yes' if r['faster'] else 'no'} | {kept_ours / 1e6:.2f} MB / "
                         f"{kept_torch / 1e6:.2f} MB | {peak['ours'] / 1e6:.2f} MB / {peak['torch'] / 1e6:.2f} MB |")
        result["sizes"].append(size)
        del dense, sparse
        torch.cuda.empty_cache()
    table = "\n".join(lines)
    print(table)
    for path, text in ((a.out, json.dumps(result, indent=1)), (a.md, table + "\n")):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
