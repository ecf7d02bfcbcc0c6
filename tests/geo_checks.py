"""What the host build (tests/test_geo_metrics.py) and the kernels (tests/test_gpu_geo_metrics.py) of the geometry evaluation
are both held to, against tests/golden/geo_metrics.npz (made by the reference's own metric.py, tests/golden/make_golden_geo.py).

EPS: the direct-form squared distance is 3 subtractions, 3 products and 2 sums, each rounded once to fp32 -- within
8 * 2^-24 relative of the exact value; a minimum over candidates that are each within EPS of their true value is within
EPS of the true minimum.  The reference's distances are float64 (SciPy's cKDTree on the same float32 points)."""
import os

import numpy as np

EPS = 8 * 2.0 ** -24
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "geo_metrics.npz")


def load():
    return np.load(GOLDEN)


def check_nn(z, way, dist2, index):
    """way = "12" (p1 -> p2) or "21"."""
    ref = z["d" + way] ** 2
    err = np.abs(dist2.astype(np.float64) - ref)
    assert (err <= EPS * ref).all(), f"d2 {way}: worst {np.max(err / ref):.3e} relative (bound {EPS:.3e})"
    assert np.array_equal(index, z["i" + way]), f"index {way}: {np.count_nonzero(index != z['i' + way])} differ"
    if way == "12":
        assert not (index == 10).any()  # p2[10] duplicates p2[3]: the lower index wins


def check_metrics(z, fscore, chamfer, precision, recall, count12=None, count21=None):
    n1, n2 = z["p1"].shape[0], z["p2"].shape[0]
    want12, want21 = round(float(z["percent12"]) / 100 * n1), round(float(z["percent21"]) / 100 * n2)
    if count12 is None:  # the kernels report percentages; n * percent / 100 is exact to far better than 0.5
        count12, count21 = precision / 100 * n1, recall / 100 * n2
        assert abs(count12 - round(count12)) < 1e-6 and abs(count21 - round(count21)) < 1e-6
    assert (round(count12), round(count21)) == (want12, want21)
    # the reference's F is float32 arithmetic (np.mean of a float32 0/1 array, times 100): four roundings of 2^-24
    assert abs(fscore - float(z["fscore"])) <= 1e-6 * float(z["fscore"]), (fscore, float(z["fscore"]))
    # every d2 is off by at most EPS to one side at worst, plus float64 summation
    assert abs(chamfer - float(z["chamfer"])) <= 1e-6 * float(z["chamfer"]), (chamfer, float(z["chamfer"]))


def sample_point64(v0, v1, v2, u1, u2):
    """float64 restatement of trimesh's construction (geo_math.hpp sample_point) and the per-component bound
    8 * 2^-24 * (|v0|inf + |e1|inf + |e2|inf)."""
    v0, v1, v2, u1, u2 = (np.asarray(a, np.float64) for a in (v0, v1, v2, u1, u2))
    fold = u1 + u2 > 1.0
    u1 = np.where(fold, np.abs(u1 - 1.0), u1)
    u2 = np.where(fold, np.abs(u2 - 1.0), u2)
    e1, e2 = v1 - v0, v2 - v0
    p = v0 + u1[:, None] * e1 + u2[:, None] * e2
    bound = EPS * (np.abs(v0).max(1) + np.abs(e1).max(1) + np.abs(e2).max(1))
    return p, bound
