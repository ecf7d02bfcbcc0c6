"""The geometry evaluation on the GPU: the kernels of csrc/geo.hip through the C ABI and
mpmavatar_amd/geo_metrics.py, against the fixture the reference's own metric.py produced (tests/golden/geo_metrics.npz,
the same checks as the host build in tests/test_geo_metrics.py), float64 brute force, and SciPy's cKDTree at the
reference's sample count."""
import numpy as np
import pytest

import geo_checks as gc

pytestmark = pytest.mark.gpu
EPS = gc.EPS


def dev():
    import torch
    return torch.device("cuda:0")


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def d2_matrix64(src, dst):
    s, d = src.astype(np.float64), dst.astype(np.float64)
    return ((s[:, None, :] - d[None, :, :]) ** 2).sum(-1)


@pytest.fixture(scope="module")
def fixture_runs():
    """Both directions over the fixture, for slices = 0 and 3, each twice: {(way, slices): [(d2, idx), (d2, idx)]}."""
    from mpmavatar_amd import geo_metrics as gm
    z = gc.load()
    p = {"12": (to_dev(z["p1"]), to_dev(z["p2"])), "21": (to_dev(z["p2"]), to_dev(z["p1"]))}
    runs = {}
    for way, (s, d) in p.items():
        for slices in (0, 3):   # 2500 and 3000 are no multiples of 3: the slice tail and the 64-bit fold
            runs[way, slices] = [tuple(t.cpu().numpy() for t in gm.nearest_dist2(s, d, return_index=True, slices=slices))
                                 for _ in range(2)]
    return z, runs


@pytest.mark.parametrize("slices", [0, 3])
def test_fixture_nearest_neighbours(fixture_runs, slices):
    z, runs = fixture_runs
    for way in ("12", "21"):
        gc.check_nn(z, way, *runs[way, slices][0])


def test_fixture_slicing_and_reruns_agree_bitwise(fixture_runs):
    _, runs = fixture_runs
    for way in ("12", "21"):
        d0, i0 = runs[way, 0][0]
        for d, i in (runs[way, 0][1], runs[way, 3][0], runs[way, 3][1]):
            assert np.array_equal(d.view(np.int32), d0.view(np.int32)) and np.array_equal(i, i0)


@pytest.mark.parametrize("slices", [0, 3])
def test_fixture_counts_fscore_and_chamfer(fixture_runs, slices):
    from mpmavatar_amd import geo_metrics as gm
    z, runs = fixture_runs
    d12, d21 = to_dev(runs["12", slices][0][0]), to_dev(runs["21", slices][0][0])
    out = [gm.reduce_dist2(d12, d21, float(z["tau"])).cpu().numpy() for _ in range(2)]
    assert np.array_equal(out[0].view(np.int64), out[1].view(np.int64))
    gc.check_metrics(z, *out[0])
    both = gm.chamfer_fscore(to_dev(z["p1"]), to_dev(z["p2"])).cpu().numpy()   # the public one-call form
    assert np.array_equal(both.view(np.int64), out[0].view(np.int64))


def test_far_sets_score_zero():
    from mpmavatar_amd import geo_metrics as gm
    rng = np.random.default_rng(3)
    a = rng.random((200, 3)).astype(np.float32)
    out = gm.chamfer_fscore(to_dev(a), to_dev(a[:150] + np.float32(2.0))).cpu().numpy()
    assert np.isfinite(out).all() and out[0] == 0.0 and out[2] == 0.0 and out[3] == 0.0


@pytest.mark.parametrize("n_dst", [1, 2, 513, 2049])
@pytest.mark.parametrize("n_src", [1, 255, 1025])
def test_tails(n_src, n_dst):
    """Sizes that are no multiple of the lanes x queries per workgroup, of the LDS tile, of the chunk, of two or of the slice
    count; 5 slices of 1 or 2 targets must be clamped."""
    from mpmavatar_amd import geo_metrics as gm
    rng = np.random.default_rng(1000 * n_src + n_dst)
    src, dst = rng.random((n_src, 3)).astype(np.float32), rng.random((n_dst, 3)).astype(np.float32)
    ref = d2_matrix64(src, dst)
    best = ref.min(1)
    first = None
    for slices in (0, 1, 5):
        d2, idx = (t.cpu().numpy() for t in gm.nearest_dist2(to_dev(src), to_dev(dst), return_index=True, slices=slices))
        assert (np.abs(d2 - best) <= EPS * best).all(), (slices, float((np.abs(d2 - best) / best).max()))
        assert ((idx >= 0) & (idx < n_dst)).all()
        # the fp32 winner may be another target than the float64 one if the two are closer than both their errors
        assert (ref[np.arange(n_src), idx] <= (1 + 2 * EPS) * best).all(), slices
        if first is None:
            first = (d2, idx)
        assert np.array_equal(d2.view(np.int32), first[0].view(np.int32)) and np.array_equal(idx, first[1])


def test_coincident_sets():
    from mpmavatar_amd import geo_metrics as gm
    rng = np.random.default_rng(9)
    p = rng.random((1500, 3)).astype(np.float32)
    p[700] = p[20]
    p[1499] = p[1300]
    t = to_dev(p)
    for slices in (0, 4):
        d2, idx = (a.cpu().numpy() for a in gm.nearest_dist2(t, t, return_index=True, slices=slices))
        assert (d2 == 0).all() and (idx <= np.arange(1500)).all()
        assert idx[700] == 20 and idx[1499] == 1300 and (np.delete(idx, [700, 1499]) == np.delete(np.arange(1500), [700, 1499])).all()


def wavy_grid():
    """24 x 24 quads (1,152 triangles), wavy; the triangle in the middle collapsed to zero area."""
    from mpmavatar_amd import garment
    v, f = garment.grid_sheet(25, 25, 0.0, 1.0, 0.0, 1.3, 0.5)
    v[:, 1] += (0.07 * np.sin(7 * v[:, 0]) * np.cos(5 * v[:, 2])).astype(np.float32)
    f = f.copy()
    f[576, 1] = f[576, 0]
    return v, f


def test_sampling():
    import torch
    from mpmavatar_amd import geo_metrics as gm
    v, f = wavy_grid()
    assert f.shape[0] == 1152
    tv, tf = to_dev(v), to_dev(f)
    n, seed = 20000, 5
    gen = lambda: torch.Generator(device=dev()).manual_seed(seed)
    pts, fidx = (t.cpu().numpy() for t in gm.sample_surface(tv, tf, n, generator=gen()))
    u = torch.rand(n, 3, generator=gen(), dtype=torch.float32, device=dev()).cpu().numpy()   # the draw sample_surface made
    area, cdf = (t.cpu().numpy() for t in gm.face_area_cdf(tv, tf))

    tri = v[f].astype(np.float64)
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    area64 = 0.5 * np.linalg.norm(np.cross(e1, e2), axis=1)
    assert (np.abs(area - area64) <= EPS * np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1)).all()
    assert area[576] == 0.0 and cdf.dtype == np.float64 and cdf[576] == cdf[575]

    want = np.searchsorted(cdf, u[:, 0].astype(np.float64) * cdf[-1])
    assert np.array_equal(fidx, want)
    assert not (fidx == 576).any()
    assert np.unique(fidx).size > 1000   # area-weighted over the whole mesh, not a corner of it

    t32 = v[f[fidx]]
    p64, bound = gc.sample_point64(t32[:, 0], t32[:, 1], t32[:, 2], u[:, 1], u[:, 2])
    err = np.abs(pts - p64).max(1)
    assert (err <= bound).all(), float((err / bound).max())

    pts2, fidx2 = (t.cpu().numpy() for t in gm.sample_surface(tv, tf, n, generator=gen()))
    assert np.array_equal(pts2.view(np.int32), pts.view(np.int32)) and np.array_equal(fidx2, fidx)


def test_reference_size():
    """The one test at the reference's 100,000 samples: the automatic slice count and the 64-bit fold under real contention."""
    import torch
    from scipy.spatial import cKDTree
    from mpmavatar_amd import garment
    from mpmavatar_amd import geo_metrics as gm
    v1, f1 = wavy_grid()
    v2, f2 = garment.grid_sheet(31, 23, 0.0, 1.0, 0.0, 1.3, 0.52)
    v2[:, 1] += (0.06 * np.sin(6 * v2[:, 0]) * np.cos(5 * v2[:, 2])).astype(np.float32)
    t = [to_dev(a) for a in (v1, f1, v2, f2)]
    gen = lambda: torch.Generator(device=dev()).manual_seed(21)
    fs, cd = gm.all_mesh_metrics(*t, generator=gen())

    g = gen()   # the same two draws, to look at what lies between them and the two numbers
    p1, _ = gm.sample_surface(t[0], t[1], 100000, g)
    p2, _ = gm.sample_surface(t[2], t[3], 100000, g)
    d12, d21 = gm.nearest_dist2(p1, p2), gm.nearest_dist2(p2, p1)
    out = gm.reduce_dist2(d12, d21).cpu().numpy()
    assert out[0] == float(fs) and out[1] == float(cd)

    h1, h2 = p1.cpu().numpy(), p2.cpu().numpy()
    tau, close, counts, sums = 1e-3, 0, [], []
    for d, src, dst in ((d12, h1, h2), (d21, h2, h1)):
        ref = cKDTree(dst).query(src)[0] ** 2
        got = d.cpu().numpy().astype(np.float64)
        assert (np.abs(got - ref) <= EPS * ref).all(), float((np.abs(got - ref) / ref).max())
        close += int((np.abs(ref - tau) <= EPS * tau).sum())   # the only distances whose side of tau fp32 may change
        counts.append(int((ref <= tau).sum()))
        sums.append(ref.mean())
    assert abs(out[2] / 100 * 100000 - counts[0]) <= close + 1e-6 and abs(out[3] / 100 * 100000 - counts[1]) <= close + 1e-6
    assert 0.0 < out[0] < 100.0
    assert abs(out[1] - 1000 * (sums[0] + sums[1])) <= 1e-6 * out[1]


def test_invalid_arguments():
    import torch
    from mpmavatar_amd import _lib as L
    lib = L.load()
    f32 = torch.zeros(64, 3, dtype=torch.float32, device=dev())
    i32 = torch.zeros(64, 3, dtype=torch.int32, device=dev())
    f64 = torch.ones(256, dtype=torch.float64, device=dev())
    i64 = torch.zeros(64, dtype=torch.int64, device=dev())
    a, b, c, w = f32.data_ptr(), i32.data_ptr(), f64.data_ptr(), i64.data_ptr()
    bad = L.ERR_INVALID
    assert lib.mpmhip_face_areas(0, None, a, b, 4, a) == L.OK
    for args in ((a, b, 0, a), (a, b, -1, a), (None, b, 4, a), (a, None, 4, a), (a, b, 4, None)):
        assert lib.mpmhip_face_areas(0, None, *args) == bad, args
    assert lib.mpmhip_mesh_sample(0, None, a, b, 4, c, a, 8, a, None) == L.OK
    for args in ((a, b, 0, c, a, 8, a, None), (a, b, 4, c, a, 0, a, None), (None, b, 4, c, a, 8, a, None), (a, None, 4, c, a, 8, a, None),
                 (a, b, 4, None, a, 8, a, None), (a, b, 4, c, None, 8, a, None), (a, b, 4, c, a, 8, None, None)):
        assert lib.mpmhip_mesh_sample(0, None, *args) == bad, args
    d2 = torch.empty(64, dtype=torch.float32, device=dev()).data_ptr()
    assert lib.mpmhip_nn_dist2(0, None, a, 8, a, 8, 0, w, d2, None) == L.OK
    for args in ((a, 0, a, 8, 0, w, d2, None), (a, -3, a, 8, 0, w, d2, None), (a, 8, a, 0, 0, w, d2, None), (a, 8, a, 8, -1, w, d2, None),
                 (None, 8, a, 8, 0, w, d2, None), (a, 8, None, 8, 0, w, d2, None), (a, 8, a, 8, 0, None, d2, None),
                 (a, 8, a, 8, 0, w, None, None)):
        assert lib.mpmhip_nn_dist2(0, None, *args) == bad, args
    out = torch.empty(4, dtype=torch.float64, device=dev()).data_ptr()
    assert lib.mpmhip_geo_reduce(0, None, d2, 8, d2, 8, 1e-3, c, out) == L.OK
    for args in ((d2, 0, d2, 8, 1e-3, c, out), (d2, 8, d2, 0, 1e-3, c, out), (None, 8, d2, 8, 1e-3, c, out), (d2, 8, None, 8, 1e-3, c, out),
                 (d2, 8, d2, 8, 1e-3, None, out), (d2, 8, d2, 8, 1e-3, c, None)):
        assert lib.mpmhip_geo_reduce(0, None, *args) == bad, args
    torch.cuda.synchronize()


def test_geo_eval_accumulates_on_the_device_and_saves_the_reference_keys(tmp_path):
    import torch
    from mpmavatar_amd import geo_metrics as gm
    v, f = wavy_grid()
    tv, tf = to_dev(v), to_dev(f)
    ev = gm.GeoEval(tf, sample_count=4000, seed=2)
    buffers = [t.data_ptr() for t in (ev._u, ev._best, ev._scratch, *ev._p, *ev._d)]
    row0 = ev.add_frame(tv, tv, tf)                                            # the mesh against itself
    row1 = ev.add_frame(tv + torch.tensor([0.0, 0.2, 0.0], device=dev()), tv, tf)   # moved 0.2 > sqrt(tau) off it
    assert row0.is_cuda and row0.dtype == torch.float64
    assert buffers == [t.data_ptr() for t in (ev._u, ev._best, ev._scratch, *ev._p, *ev._d)]
    z = np.load(ev.save(str(tmp_path)))
    assert sorted(z.files) == ["CD", "F-Score"] and z["CD"].shape == (2,)
    assert z["F-Score"][0] > 90.0 and z["CD"][0] < 1.0      # two draws of 4000 points on a 1.3 m^2 sheet: ~1e-4 apart squared
    assert z["F-Score"][1] == 0.0 and z["CD"][1] > 1000 * 2 * 0.15 ** 2
    # the same seed gives the same file
    ev2 = gm.GeoEval(tf, sample_count=4000, seed=2)
    ev2.add_frame(tv, tv, tf)
    assert float(ev2.rows[0][1]) == z["CD"][0] and float(ev2.rows[0][0]) == z["F-Score"][0]
