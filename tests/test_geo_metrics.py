"""The geometry evaluation without a GPU: mpmavatar_amd/csrc/geo_math.hpp compiled with g++ (tests/hostgeo/hostgeo.cpp, the way
test_hip_math_on_host.py compiles mpm_math.hpp) against the fixture the reference's own metric.py produced
(tests/golden/geo_metrics.npz), and the host side of the Python layer.  The kernels take the same checks in
tests/test_gpu_geo_metrics.py."""
import ctypes as C
import os

import numpy as np
import pytest

import geo_checks as gc
from hostbuild import host_lib


fp, ip, dp = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def hg():
    return host_lib("hostgeo")


def nn(hg, src, dst):
    src, dst = np.ascontiguousarray(src, np.float32), np.ascontiguousarray(dst, np.float32)
    d2, idx = np.empty(src.shape[0], np.float32), np.empty(src.shape[0], np.int32)
    hg.hg_nn(src.ctypes.data_as(fp), src.shape[0], dst.ctypes.data_as(fp), dst.shape[0], d2.ctypes.data_as(fp), idx.ctypes.data_as(ip))
    return d2, idx


def metrics(hg, d12, d21, tau):
    out = np.empty(6, np.float64)
    hg.hg_metrics(d12.ctypes.data_as(fp), d12.shape[0], d21.ctypes.data_as(fp), d21.shape[0], C.c_double(tau), out.ctypes.data_as(dp))
    return out


@pytest.fixture(scope="module")
def fixture_run(hg):
    """Both nearest-neighbour passes over the fixture, computed once."""
    z = gc.load()
    return z, nn(hg, z["p1"], z["p2"]), nn(hg, z["p2"], z["p1"])


def test_nearest_neighbours_match_the_reference(fixture_run):
    z, (d12, i12), (d21, i21) = fixture_run
    gc.check_nn(z, "12", d12, i12)
    gc.check_nn(z, "21", d21, i21)


def test_duplicate_target_lowest_index_wins(hg):
    z = gc.load()
    p2 = z["p2"]
    assert np.array_equal(p2[10], p2[3])
    d2, idx = nn(hg, p2[[3, 10]], p2)
    assert (d2 == 0).all() and (idx == 3).all()


def test_counts_fscore_and_chamfer_match_the_reference(hg, fixture_run):
    z, (d12, _), (d21, _) = fixture_run
    f, cd, p, r, c12, c21 = metrics(hg, d12, d21, float(z["tau"]))
    gc.check_metrics(z, f, cd, p, r, c12, c21)
    gc.check_metrics(z, f, cd, p, r)   # and through the percentages, the form the kernels report


def test_sets_farther_apart_than_the_threshold_score_zero(hg):
    rng = np.random.default_rng(3)
    a = rng.random((200, 3)).astype(np.float32)
    b = a[:150] + np.float32(2.0)   # every distance > 1 > sqrt(tau)
    (d12, _), (d21, _) = nn(hg, a, b), nn(hg, b, a)
    out = metrics(hg, d12, d21, 1e-3)
    assert np.isfinite(out).all()
    assert out[0] == 0.0 and out[2] == 0.0 and out[3] == 0.0 and out[1] > 1000.0


def test_sample_point_against_float64(hg):
    rng = np.random.default_rng(11)
    n = 4000
    v = [(rng.normal(size=(n, 3)) * rng.choice([1e-2, 1.0, 30.0], size=(n, 1))).astype(np.float32) for _ in range(3)]
    u1, u2 = rng.random(n).astype(np.float32), rng.random(n).astype(np.float32)
    u2[:500] = np.float32(1.0) - u1[:500]            # u1 + u2 == 1 (exactly, or one rounding away from it on either side)
    u1[500], u2[500] = 0.25, 0.75                    # exactly on the diagonal: not folded
    u1[501], u2[501] = 0.75, np.nextafter(np.float32(0.25), np.float32(1))  # one ulp beyond it: folded
    u1[502], u2[502] = 0.0, 0.0
    assert ((u1.astype(np.float64) + u2 > 1).sum() > 1000) and ((u1.astype(np.float64) + u2 == 1).sum() > 100)
    out = np.empty((n, 3), np.float32)
    hg.hg_sample_point(*(np.ascontiguousarray(a).ctypes.data_as(fp) for a in (v[0], v[1], v[2], u1, u2)), n, out.ctypes.data_as(fp))
    want, bound = gc.sample_point64(v[0], v[1], v[2], u1, u2)
    err = np.abs(out - want).max(1)
    assert (err <= bound).all(), float((err / bound).max())


def test_python_layer_imports_without_a_gpu_and_writes_the_reference_keys(tmp_path):
    from mpmavatar_amd import geo_metrics, io_formats
    for name in ("sample_surface", "nearest_dist2", "chamfer_fscore", "all_mesh_metrics", "all_mesh_metrics_points", "GeoEval"):
        assert callable(getattr(geo_metrics, name))
    cd, fs = [7.5, 8.25, 0.125], [67.0, 66.5, 99.0]
    path = io_formats.write_geo_metric_npz(str(tmp_path / "out"), cd, fs)
    assert os.path.basename(path) == "geo_metric.npz"
    z = np.load(path)
    assert sorted(z.files) == ["CD", "F-Score"]   # eval.py:31
    assert np.array_equal(z["CD"], cd) and np.array_equal(z["F-Score"], fs)
