#!/usr/bin/env python
"""Time the geometry evaluation at the reference's size: one full all_mesh_metrics frame at 100,000
samples per mesh, the nearest-neighbour call alone, and beside them the reference's path -- metric.fscore plus
metric.mesh_chamfer_via_points, i.e. four cKDTree builds and queries, restated below -- on this machine's CPUs.

    python tools/gpu/geo_metrics_bench.py [--samples 100000] [--reps 100] [--variant name=path/to/libmpmhip_name.so ...] [--out file.json]

--variant times mpmhip_nn_dist2 of other builds of csrc/geo.hip (tools/build_variants.py, e.g. q8:ONLY=geo.hip,ALL,-DGEO_NN_Q=8)
on the same buffers, interleaved with the default build.  Times are HIP events on torch's current stream, where the
kernels are launched.  Rates: a "pair" is one (query, target) distance; the kernel spends 3.5 VALU instructions on it (per
two targets: 3 packed subtracts, 1 packed multiply, 2 packed FMAs, 1 three-way minimum), 8 flops of them arithmetic.
The fp32 vector peak of an MI355X, 157.3 TF, is 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz issuing one packed FMA (4 flops) each
clock; a kernel made of this instruction mix can reach 8 / (3.5 * 4) = 57 % of it."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

from mpmavatar_amd import _lib as L
from mpmavatar_amd import garment
from mpmavatar_amd import geo_metrics as gm

PEAK_FLOPS = 157.3e12
ISSUE_RATE = 256 * 4 * 16 * 2.4e9     # lane-instructions per second
FLOPS_PER_PAIR, INSTR_PER_PAIR = 8, 3.5


def sheet(nx, nz, y, amp):
    v, f = garment.grid_sheet(nx, nz, 0.0, 1.0, 0.0, 1.3, y)
    v[:, 1] += (amp * np.sin(6 * v[:, 0]) * np.cos(5 * v[:, 2])).astype(np.float32)
    return v, f


def events_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def reference_path(p1, p2, tau=1e-3):
    """metric.py:18-54 on two point sets, call for call (fscore and mesh_chamfer_via_points each query both directions)."""
    from scipy.spatial import cKDTree

    def nn(s, t):
        return cKDTree(t).query(s)[0]
    d12, d21 = nn(p1, p2), nn(p2, p1)
    pr, rc = (np.mean((d ** 2 <= tau).astype(np.float32)) * 100.0 for d in (d12, d21))
    fs = (2 * pr * rc) / (pr + rc + 1e-09)
    d12, d21 = nn(p1, p2), nn(p2, p1)
    return fs, 1000.0 * (np.mean(d12 ** 2) + np.mean(d21 ** 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--variant", action="append", default=[], help="name=path of another build of the library")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("geo_metrics_bench.py measures on the GPU; there is none")
    dev = torch.device("cuda:0")
    n = a.samples
    (v1, f1), (v2, f2) = sheet(201, 261, 0.5, 0.05), sheet(181, 231, 0.528, 0.06)   # ~104,000 and ~83,000 triangles
    t = [torch.from_numpy(x).to(dev) for x in (v1, f1, v2, f2)]
    gen = torch.Generator(device=dev).manual_seed(0)

    frame = lambda: gm.all_mesh_metrics(*t, sample_count=n, generator=gen)
    for _ in range(3):
        fs, cd = frame()
    frame_ms = events_ms(frame, a.reps)

    p1, _ = gm.sample_surface(t[0], t[1], n, gen)
    p2, _ = gm.sample_surface(t[2], t[3], n, gen)
    best = torch.empty(n, dtype=torch.int64, device=dev)
    d2 = torch.empty(n, dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    libs = {"default": L.load()}
    for spec in a.variant:
        name, _, path = spec.partition("=")
        lib = C.CDLL(path)
        lib.mpmhip_nn_dist2.restype, lib.mpmhip_nn_dist2.argtypes = L.SIGNATURES["mpmhip_nn_dist2"]
        libs[name] = lib

    def nn_call(lib):
        def run():
            rc = lib.mpmhip_nn_dist2(0, stream, p1.data_ptr(), n, p2.data_ptr(), n, 0, best.data_ptr(), d2.data_ptr(), None)
            assert rc == L.OK, rc
        return run
    want = None
    nn_ms = {k: [] for k in libs}
    for name, lib in libs.items():          # warm-up, and every build must give the same bits
        nn_call(lib)()
        got = d2.cpu()
        want = got if want is None else want
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), name
    for _ in range(3):                      # interleaved rounds: the spread between rounds is the noise
        for name, lib in libs.items():
            nn_ms[name].append(events_ms(nn_call(lib), a.reps))

    h1, h2 = p1.cpu().numpy(), p2.cpu().numpy()
    t0 = time.perf_counter()
    fs_ref, cd_ref = reference_path(h1, h2)
    host_ms = (time.perf_counter() - t0) * 1e3
    out = gm.chamfer_fscore(p1, p2).cpu().numpy()

    pairs = float(n) * n
    res = {"samples": n, "reps": a.reps, "cpus": len(os.sched_getaffinity(0)),
           "frame_ms_device": frame_ms, "frame_ms_reference_path_host": host_ms, "speedup": host_ms / frame_ms,
           "fscore_device": float(out[0]), "fscore_host": float(fs_ref), "chamfer_device": float(out[1]), "chamfer_host": float(cd_ref),
           "nn_dist2_ms_per_direction": {k: v for k, v in nn_ms.items()}}
    for name, ms in nn_ms.items():
        rate = pairs / (min(ms) * 1e-3)
        res[f"pair_rate_{name}"] = rate
        res[f"share_of_fp32_vector_peak_{name}"] = rate * FLOPS_PER_PAIR / PEAK_FLOPS
        res[f"share_of_valu_issue_slots_{name}"] = rate * INSTR_PER_PAIR / ISSUE_RATE
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
