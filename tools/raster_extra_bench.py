#!/usr/bin/env python
"""Time the rasteriser's extra attribute channels (mpmavatar_amd.rasterizer, csrc/raster_extra.hip; the reference's
preprocess/train_mesh_lbs_4ddress.py:260-277, :299, :306) with E = 2 against what a user could do without them, the statements
alternating in one process:

  fused     one call with ``extra_attrs``: slot 5 comes out of one more walk over the sorted tile lists, in both directions
  two-call  the same result from two calls: the table, padded to three channels, as ``colors_precomp`` of a second call over a zero
            background -- preprocess, scan, duplicate, sort, tile ranges, the saved frame and the backward pass all run twice
  plain     the call without extras: what the fused call costs on top of it is the overhead of the feature

each as the forward alone (grad mode off) and as forward + backward of L = sum Wi image + sum Wa alpha (+ sum Wx extra), at two sizes:

  raster   tools/raster_bench.py's frame: 200,000 Gaussians bound to the S3 garment, 1024 x 1024
  track    the tracking size that tools/track_bench.py assumes: one Gaussian per face of a mesh of about 40,000 faces, 1024 x 1024
           (the image size is an ASSUMPTION too; the reference's data is not available to this tool)

    python tools/raster_extra_bench.py [--warmup 5] [--reps 30] [--out file.json] [--md file.md]

Each repetition is timed between two HIP events on torch's current stream, after the warm-up of all three; reported are the minimum,
the median and the maximum, and the peak allocation of one call.  "cheaper than rendering twice" is claimed only where the fused
maximum is below the two-call minimum; every row is reported, including any that is not.  No ratio is a pass condition."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIDES = ("fused", "two-call", "plain")


def raster_frame(torch, np, dev, n=200000):
    """the arguments of tools/raster_bench.py's frame and its camera"""
    from mpmavatar_amd import scenes
    from mpmavatar_amd.render_inputs import BoundGaussians
    from mpmavatar_amd.mesh_frames import MeshFrames
    sc = scenes.garment_cylinder()
    faces = torch.as_tensor(sc.faces, device=dev)
    verts = torch.as_tensor(np.asarray(sc.x[sc.n_elements + sc.n_traditional:], np.float32), device=dev).contiguous()
    n_f = faces.shape[0]
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)
    binding = (torch.arange(n, device=dev) % n_f).to(torch.int32)
    gaussians = BoundGaussians(0.35 * rnd(n, 3) * torch.tensor([1.0, 1.0, 0.05], device=dev), rnd(n, 4), -0.6 + 0.2 * rnd(n, 3), 2.0 + rnd(n, 1),
                               torch.zeros(n, 1, 3, device=dev), torch.zeros(n, 0, 3, device=dev), binding)
    frames = MeshFrames(faces)
    frames.set_mesh_by_verts(verts)
    args = gaussians.render_inputs(frames, override_color=torch.rand(n, 3, device=dev, generator=g))
    centre = verts.mean(0).cpu().numpy()
    return {k: v for k, v in args.items() if isinstance(v, torch.Tensor)}, centre + np.array([0.0, 0.15, -1.6]), centre


def track_frame(torch, np, dev, faces=40000):
    """one Gaussian per face of a gently curved square sheet of about `faces` triangles, as FaceGaussians hands them over"""
    from mpmavatar_amd.tracking import FaceGaussians
    m = int(round((faces / 2) ** 0.5)) + 1
    i, j = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    x, y = i.reshape(-1) / (m - 1) - 0.5, j.reshape(-1) / (m - 1) - 0.5
    verts = np.stack([x, y, 0.15 * np.sin(4 * x) * np.cos(3 * y)], 1).astype(np.float32)
    q = (i[:-1, :-1] * m + j[:-1, :-1]).reshape(-1)
    tris = np.concatenate([np.stack([q, q + m, q + 1], 1), np.stack([q + 1, q + m, q + m + 1], 1)]).astype(np.int32)
    fg = FaceGaussians(torch.tensor(tris, device=dev))
    v = torch.tensor(verts, device=dev)
    n_f = tris.shape[0]
    log_scales = torch.full((n_f, 3), -100.0, device=dev)
    log_scales[:, :2] = 0.5 * torch.log(fg.face_areas(v) / torch.pi)[:, None]
    with torch.no_grad():
        args = fg.render_vars(v, log_scales, torch.full((n_f, 1), 2.0, device=dev))
    args["colors_precomp"] = torch.rand(n_f, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    return args, np.array([0.0, 0.2, -1.5]), np.zeros(3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("raster_extra_bench: no GPU; a timing needs the device")
    from mpmavatar_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer, look_at_camera
    dev = torch.device("cuda:0")
    result = {"E": 2, "size": a.size, "warmup": a.warmup, "reps": a.reps, "device": torch.cuda.get_device_name(0), "frames": {}}
    for frame_name, make in (("raster", raster_frame), ("track", track_frame)):
        base, eye, target = make(torch, np, dev)
        n = base["means3D"].shape[0]
        view, proj, campos, tanfov = look_at_camera(eye, target, 40.0, dev)
        mk = lambda bg: GaussianRasterizationSettings(a.size, a.size, tanfov, tanfov, bg, 1.0, view, proj, 0, campos, False, False)
        rast, rast0 = GaussianRasterizer(mk(torch.full((3,), 0.5, device=dev))), GaussianRasterizer(mk(torch.zeros(3, device=dev)))
        g = torch.Generator(device=dev).manual_seed(2)
        table = (torch.rand(n, 2, device=dev, generator=g) < 0.5).float()                 # upper / lower garment, 0 / 1
        padded = torch.cat([table, torch.zeros(n, 1, device=dev)], 1).contiguous()
        Wi, Wa, Wx = (torch.randn(c, a.size, a.size, device=dev, generator=g) for c in (3, 1, 2))

        def leaves(grad):
            d = {k: v.detach().clone().requires_grad_(grad) for k, v in base.items()}
            d["means2D"] = torch.zeros(n, 3, device=dev, requires_grad=True)
            return d

        def run(side, grad):
            d = leaves(grad)
            with torch.set_grad_enabled(grad):
                if side == "fused":
                    image, _, _, alpha, _, extra = rast(**d, extra_attrs=table)
                else:
                    image, _, _, alpha, _, _ = rast(**d)
                    extra = rast0(**dict(d, colors_precomp=padded))[0][:2] if side == "two-call" else None
                if grad:
                    loss = (Wi * image).sum() + (Wa * alpha).sum()
                    if extra is not None:
                        loss = loss + (Wx * extra).sum()
                    loss.backward()
                    return [image.detach(), alpha.detach(), extra if extra is None else extra.detach(), d["means3D"].grad, d["scales"].grad]
            return [image, alpha, extra]

        entries = None
        for grad in (False, True):
            mode = "forward + backward" if grad else "forward"
            for _ in range(a.warmup):
                for side in SIDES:
                    run(side, grad)
            torch.cuda.synchronize()
            times = {side: [] for side in SIDES}
            for _ in range(a.reps):
                for side in SIDES:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    run(side, grad)
                    e1.record()
                    e1.synchronize()
                    times[side].append(e0.elapsed_time(e1))
            peak = {}
            for side in SIDES:                                                            # what one call allocates on top of its inputs
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
                out = run(side, grad)
                torch.cuda.synchronize()
                peak[side] = torch.cuda.max_memory_allocated() - before
                del out
            fused, twice = run("fused", grad), run("two-call", grad)
            same = [bool(torch.equal(x, y)) for x, y in zip(fused[:3], twice[:3])]
            diff = [float((x - y).abs().max() / y.abs().max().clamp(min=1e-30)) for x, y in zip(fused[3:], twice[3:])]
            if entries is None:
                rast(**leaves(False))
                entries = rast.stats()
            stat = {side: {"min": min(ts), "median": statistics.median(ts), "max": max(ts)} for side, ts in times.items()}
            row = {"ms": stat, "peak_bytes": peak, "outputs_bit_equal_to_two_call": same, "gradient_difference_to_two_call": diff,
                   "cheaper_than_twice": stat["fused"]["max"] < stat["two-call"]["min"]}
            result["frames"].setdefault(frame_name, {"gaussians": n, "stats": entries, "modes": {}})["modes"][mode] = row
            print(frame_name, n, mode, json.dumps(row), flush=True)
            del fused, twice
    lines = ["| milliseconds (min / median / max), E = 2 | fused | two-call | plain | fused - plain (median) | fused max below two-call min | "
             "peak allocation of one call, fused / two-call / plain |", "|---|---|---|---|---|---|---|"]
    for frame_name, fr in result["frames"].items():
        for mode, r in fr["modes"].items():
            cell = lambda s: f"{r['ms'][s]['min']:.3f} / **{r['ms'][s]['median']:.3f}** / {r['ms'][s]['max']:.3f}"
            lines.append(f"| {frame_name} ({fr['gaussians']} Gaussians, {fr['stats']['n_entries']} entries), {mode} | {cell('fused')} | {cell('two-call')} | "
                         f"{cell('plain')} | {r['ms']['fused']['median'] - r['ms']['plain']['median']:.3f} | {'yes' if r['cheaper_than_twice'] else 'no'} | "
                         + " / ".join(f"{r['peak_bytes'][s] / 2 ** 20:.1f}" for s in SIDES) + " MiB |")
    table_md = "\n".join(lines)
    print(table_md)
    for path, text in ((a.out, json.dumps(result, indent=1)), (a.md, table_md + "\n")):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
