"""Golden vectors for the geometry evaluation FROM THE REFERENCE ITSELF: metric.py needs only NumPy
and SciPy and is imported unchanged, so its outputs on seeded point sets pin mpmavatar_amd/csrc/geo_math.hpp (host build)
and the kernels of csrc/geo.hip.  Run in the build container (needs /root/reference):
    python tests/golden/make_golden_geo.py
The fixture holds inputs and expected outputs only.  trimesh (metric.py:5) is not installed there: the surface sampling
is NOT pinned by this file."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
import metric  # noqa: E402  (the reference's module)

TAU = 1e-3


def main():
    rng = np.random.default_rng(7)

    def sheet(n, off, amp):
        u = rng.random((n, 2))
        z = amp * np.sin(6 * u[:, 0]) * np.cos(5 * u[:, 1]) + off
        return np.stack([u[:, 0], u[:, 1], z], 1).astype(np.float32)

    p1 = sheet(3000, 0.0, 0.05)
    p2 = sheet(2500, 0.028, 0.06)
    p2[10] = p2[3]            # an exact duplicate target: the lower index must win
    p1[5] = (3.0, 3.0, 3.0)   # a far outlier
    d12, i12 = metric.pointcloud_neighbor_distances_indices(p1, p2)
    d21, i21 = metric.pointcloud_neighbor_distances_indices(p2, p1)
    # what makes the count comparison of the tests exact: no reference d^2 so close to the threshold that the 8 * 2^-24
    # (4.8e-7) relative error of an fp32 direct-form distance could move it across
    gap = min(np.abs(d12 ** 2 / TAU - 1).min(), np.abs(d21 ** 2 / TAU - 1).min())
    assert gap > 2e-6, gap
    out = dict(p1=p1, p2=p2, d12=d12, i12=i12.astype(np.int32), d21=d21, i21=i21.astype(np.int32),
               percent12=np.float64(metric.percent_below(d12, TAU)), percent21=np.float64(metric.percent_below(d21, TAU)),
               fscore=np.float64(metric.fscore(None, None, 0, TAU, p1, p2)),
               chamfer=np.float64(metric.mesh_chamfer_via_points(None, None, 0, p1, p2)), tau=np.float64(TAU))
    np.savez_compressed(os.path.join(HERE, "geo_metrics.npz"), **out)
    print(f"geo_metrics.npz: F = {out['fscore']:.4f}, CD = {out['chamfer']:.5f}, precision {out['percent12']:.2f}, "
          f"recall {out['percent21']:.2f}, closest d2 to tau {gap:.2e} relative")


if __name__ == "__main__":
    main()
