"""The Laplacian and scale-ratio terms of the 4D-DRESS tracking script without a GPU: the twin (tests/track4d_twin_torch.py) pinned
against the reference's own scale_ratio_loss (tests/golden/track4d.npz; the Laplacian has no such pin -- its matrix comes from pytorch3d,
which is not installed where the fixtures are made, so the twin's definition is UNCONFIRMED); central differences of the float64
twin; the measurement of S32, the constant the bound is built on; the conditions the cases must meet; mpmavatar_amd/csrc/track4d_math.hpp
compiled with g++ (tests/hosttrack4d/hosttrack4d.cpp: serial loops that mirror the kernels) against the float64 twin; exact zeros and
the decisions at equality; and the same file as a stand-alone program under AddressSanitizer and UBSan.  Every comparison prints its
figures before it asserts (run with -s)."""
import os
import subprocess
import warnings

import numpy as np
import pytest
import torch

import track4d_cases as t4
import track4d_twin_torch as tw

warnings.filterwarnings("ignore", message="var\\(\\): degrees of freedom")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "track4d.npz")
FIN = (84, 98, 182)                          # of `sheet`: the two ends of the edge with three faces, and the fin's own vertex


def _d(a, dtype=torch.float64):
    return torch.tensor(np.asarray(a), dtype=dtype)


def _long(a):
    return torch.from_numpy(np.asarray(a).astype(np.int64))


# ---- the twin is the reference --------------------------------------------------------------------------------------------------------

def test_twin_reproduces_the_reference():
    """tests/golden/track4d.npz: the reference's own scale_ratio_loss under autograd, float64, on the cases' float32 inputs.  Nothing
    here pins the Laplacian: test_laplacian_matrix_is_the_definition states what the twin takes it to be."""
    g = np.load(GOLD)
    assert os.path.getsize(GOLD) < 200 * 1024
    for name in t4.FIXTURE_CASES:
        t = t4.scale64(name)
        for k in t4.SCALE_TENSORS:
            ref = g[f"{name}_{k}"]
            err = t4.rel(t[k], ref)
            print(name, k, "twin against the fixture %.3g" % err)
            assert ref.dtype == np.float64 and err < 1e-13, (name, k)
    assert np.isnan(g["one_scale_edge_ratio_var"])


def test_laplacian_matrix_is_the_definition():
    """the dense L of the twin: rows sum to zero (to -1 for an isolated vertex), 1 / deg off the diagonal, the edge with three faces
    once, the degrees 2 .. 7 of the sheet; and the sparse form used above DENSE_MAX is the same matrix"""
    c = t4.case("sheet")
    faces, n_v = _long(c["faces"]), c["verts"].shape[0]
    m = tw.laplacian_matrix(faces, n_v, torch.float64)
    deg = (m > 0).sum(1)
    a, b, fin = FIN
    assert not m.is_sparse and torch.equal(m.diagonal(), -torch.ones(n_v, dtype=torch.float64)) and float(m.sum(1).abs().max()) < 1e-15
    assert int(((c["faces"] == a).any(1) & (c["faces"] == b).any(1)).sum()) == 3                             # three faces on one edge
    assert float(m[a, b]) == 1 / int(deg[a]) and float(m[b, a]) == 1 / int(deg[b]) and int(deg[fin]) == 2
    assert int(deg.min()) == 2 and int(deg.max()) == 7
    start, nbr = t4.adjacency(c["faces"], n_v)
    assert np.array_equal(np.diff(start), deg.numpy()) and all((np.diff(nbr[start[i]:start[i + 1]]) > 0).all() for i in range(n_v))
    old = tw.DENSE_MAX
    try:
        tw.DENSE_MAX = 0
        sparse = tw.laplacian_matrix(faces, n_v, torch.float64)
    finally:
        tw.DENSE_MAX = old
    assert sparse.is_sparse and torch.equal(sparse.to_dense(), m)
    lone = tw.laplacian_matrix(_long(t4.case("flat")["faces"]), 83, torch.float64)
    assert lone[81:].sum(1).tolist() == [-1.0, -1.0] and torch.equal(lone[81:, :81], torch.zeros(2, 81, dtype=torch.float64))


def test_twin_against_central_differences():
    """an anchor independent of autograd: the Laplacian on an interior vertex of the sheet, a boundary vertex and the two kinds of
    vertex on the edge with three faces; each scale term on a vertex of a face whose hinge is active and on that face's scales"""
    h = 1e-7
    c, t = t4.case("sheet"), t4.lap64("sheet")
    m = tw.laplacian_matrix(_long(c["faces"]), c["verts"].shape[0], torch.float64)
    for v, x in ((45, 0), (0, 2), (FIN[0], 1), (FIN[2], 2)):
        up, down = _d(c["verts"]), _d(c["verts"])
        up[v, x] += h
        down[v, x] -= h
        fd = float(tw.laplacian(m, up) - tw.laplacian(m, down)) / (2 * h)
        print("laplacian", (v, x), "autograd %.9g central difference %.9g" % (t["d_laplacian"][v, x], fd))
        assert abs(fd - t["d_laplacian"][v, x]) <= 1e-6 * np.abs(t["d_laplacian"]).max()
    t, faces = t4.scale64("sheet"), _long(c["faces"])
    r, q, _ = [a.numpy() for a in tw.face_quantities(_d(c["verts"]), faces, _d(c["scale"]))]
    f_r, f_q = int(np.flatnonzero(r > 6)[0]), int(np.flatnonzero(q > 1.2)[0])
    hs = 1e-9                                                                      # the scales are about 1e-2
    for i, (key, f) in enumerate((("ratio", f_r), ("edge", f_q), ("var", f_q))):
        fn = lambda v, s: tw.scale_ratio_loss(v, faces, s, *t4.TH)[i]
        for col in (0, 1):
            up, down = _d(c["scale"]), _d(c["scale"])
            up[f, col] += hs
            down[f, col] -= hs
            fd = float(fn(_d(c["verts"]), up) - fn(_d(c["verts"]), down)) / (2 * hs)
            print(key, "scale", (f, col), "autograd %.9g central difference %.9g" % (t[f"d_{key}_scale"][f, col], fd))
            assert abs(fd - t[f"d_{key}_scale"][f, col]) <= 1e-6 * np.abs(t[f"d_{key}_scale"]).max()
        if key == "ratio":
            continue
        moved = 0
        for v in c["faces"][f]:
            for x in range(3):
                up, down = _d(c["verts"]), _d(c["verts"])
                up[v, x] += h
                down[v, x] -= h
                fd = float(fn(up, _d(c["scale"])) - fn(down, _d(c["scale"]))) / (2 * h)
                print(key, "vertex", (int(v), x), "autograd %.9g central difference %.9g" % (t[f"d_{key}_verts"][v, x], fd))
                assert abs(fd - t[f"d_{key}_verts"][v, x]) <= 1e-6 * np.abs(t[f"d_{key}_verts"]).max()
                moved += fd != 0
        assert moved >= 3


# ---- the yardstick and the conditions of the comparison -----------------------------------------------------------------------------

def test_s32_is_the_measurement():
    worst, where = 0.0, None
    for name in t4.LAP_CASES:
        t32, t64 = t4.lap_twin(t4.case(name), torch.float32), t4.lap64(name)
        errs = {k: t4.rel(t32[k], t64[k]) for k in t4.LAP_TENSORS}
        print("laplacian", name, ", ".join("%s %.3g" % kv for kv in errs.items()))
        worst, where = max((worst, where), max((v, (name, k)) for k, v in errs.items()))
    for name in t4.SCALE_CASES:
        t32, t64 = t4.scale_twin(t4.case(name), torch.float32), t4.scale64(name)
        # `dyadic` through exp(log_scales) is no longer dyadic: its equalities would be decided by rounding
        errs = {k: t4.rel(t32[k], t64[k]) for k in t4.SCALE_TENSORS + (() if name == "dyadic" else ("d_log_scales",))}
        print("scale", name, ", ".join("%s %.3g" % kv for kv in errs.items()))
        worst, where = max((worst, where), max((v, (name, k)) for k, v in errs.items()))
    print("S32 measured %.4g at %s, committed %.4g" % (worst, where, t4.S32))
    assert 0.5 * t4.S32 < worst <= t4.S32
    assert t4.BOUND == 10 * t4.S32


@pytest.mark.parametrize("name", t4.LAP_CASES)
def test_laplacian_cases_meet_the_conditions(name):
    """the structure is the stated one, and outside the constructed zeros of `flat` no |Lv| is small against the mean edge: the
    direction Lv / |Lv| is well conditioned"""
    c, t = t4.case(name), t4.lap64(name)
    n_v, n_f = c["verts"].shape[0], c["faces"].shape[0]
    start, nbr = t4.adjacency(c["faces"], n_v)
    deg = np.diff(start)
    norm = np.linalg.norm(t["lv"], axis=1)
    e = c["verts"][c["faces"]].astype(np.float64)
    edge = np.linalg.norm(e - e[:, [1, 2, 0]], axis=2).mean()
    zero = norm == 0
    print(name, "V %d F %d |E| %d degrees %d..%d, min |Lv| / mean edge %.3g, exact zeros %d" % (n_v, n_f, nbr.size // 2, deg.min(), deg.max(),
                                                                                           norm[~zero].min() / edge, zero.sum()))
    assert norm[~zero].min() > 0.02 * edge
    assert (nbr >= 0).all() and (nbr < n_v).all() and start[-1] == nbr.size
    if name == "flat":
        interior = np.array([0 < i % 9 < 8 and 0 < i // 9 < 8 for i in range(81)] + [False, False])
        assert np.array_equal(zero, interior) and set(deg[interior]) == {4, 8} and (deg[81:] == 0).all()
        assert np.array_equal(t["lv"][81:], -c["verts"][81:].astype(np.float64))
        assert (t["d_laplacian"][81:] != 0).all() and (c["verts"] * 64 == np.round(c["verts"] * 64)).all()
    else:
        assert not zero.any() and (deg > 0).all()
    if name == "sheet":
        # 182 + 312 - 1 = 493 edges of the open grid (V - E + F = 1) and the fin's two; the edge under the fin counts once
        assert (n_v, n_f) == (183, 313) and n_v % t4.TPB != 0 and nbr.size // 2 == 495
    if name == "wide":
        assert n_f > t4.TPB * t4.TPB and n_v <= t4.TPB * t4.TPB
    if name == "grid257":
        assert n_v == 257 * 257 > t4.TPB * t4.TPB


@pytest.mark.parametrize("name", t4.SCALE_CASES)
def test_scale_cases_meet_the_conditions(name):
    """over EVERY face: the longest edge, the larger scale and the side of both hinges are decided alike in the twin's float32 and
    float64 runs, with a margin, outside the constructed equalities; on sheet and closed each hinge is active on at least 10 % of the
    faces and inactive on at least 10 %"""
    c = t4.case(name)
    faces, n_f = _long(c["faces"]), c["faces"].shape[0]
    dec = {}
    for dtype in (torch.float32, torch.float64):
        v, s = _d(c["verts"], dtype), _d(c["scale"], dtype)
        vf = v[faces]
        length = (vf - vf[:, [1, 2, 0]]).norm(dim=2)
        r, q, _ = tw.face_quantities(v, faces, s)
        dec[dtype] = (length.max(1).indices.numpy(), s[:, :2].max(1).indices.numpy(), s[:, :2].min(1).indices.numpy(), (r >= t4.TH[0]).numpy(),
                      (q >= t4.TH[1]).numpy())
        if dtype == torch.float64:
            top = length.sort(1, descending=True).values
            margins = {"edge": ((top[:, 0] - top[:, 1]) / top[:, 0]).numpy(), "scale": ((s[:, 0] - s[:, 1]).abs() / s[:, :2].max(1).values).numpy(),
                       "r": ((r - t4.TH[0]).abs() / t4.TH[0]).numpy(), "q": ((q - t4.TH[1]).abs() / t4.TH[1]).numpy()}
            r64, q64 = r.numpy(), q.numpy()
    for a, b in zip(dec[torch.float32], dec[torch.float64]):
        assert np.array_equal(a, b)
    tied = {k: np.zeros(n_f, bool) for k in margins}
    if name == "ties":
        tied["edge"][:4] = True
        assert (margins["edge"][:4] == 0).all() and dec[torch.float64][0][:4].tolist() == [0, 1, 0, 0]
    if name == "flat":
        tied["edge"] = margins["edge"] == 0                                        # a dyadic grid: equal lengths are exactly equal
    if name == "dyadic":
        tied["scale"][0], tied["r"][1], tied["q"][2], tied["edge"][3] = True, True, True, True
        assert margins["scale"][0] == 0 and r64[1] == 5.0 and q64[2] == 1.0 and margins["edge"][3] == 0
        assert dec[torch.float64][0][3] == 0 and dec[torch.float64][1][0] == 0 and dec[torch.float64][2][0] == 0     # the first wins
        assert dec[torch.float64][3][1] and dec[torch.float64][4][2] and dec[torch.float64][1][3] == 1
        assert (c["verts"] % t4.BIG == 0).all() and (c["scale"][:, :2] % t4.BIG == 0).all()
    print(name, "minimum margins (float64):", ", ".join("%s %.3g" % (k, m[~tied[k]].min() if (~tied[k]).any() else np.inf) for k, m in margins.items()),
          "; hinges active on %d and %d of %d" % (dec[torch.float64][3].sum(), dec[torch.float64][4].sum(), n_f))
    # s0 against s1 compares inputs; r is an addition and a division, q and the edge lengths three squares, two additions, a root, an
    # addition and a division: at most eight roundings of 2^-24 each.  1e-6 is sixteen of them
    for k, m in margins.items():
        assert (m[~tied[k]] > 1e-6).all(), k
    assert (c["log_scales"][:, 2] == -100).all() and c["scale"].dtype == np.float32
    if name in ("sheet", "closed"):
        for active in dec[torch.float64][3:]:
            assert 0.1 * n_f <= active.sum() <= 0.9 * n_f
    if name == "wide":
        assert n_f > t4.TPB * t4.TPB


# ---- track4d_math.hpp on the host against the float64 twin -----------------------------------------------------------------------------

@pytest.mark.parametrize("name", t4.LAP_CASES)
def test_host_laplacian_against_float64(name):
    got, want = t4.host_lap(t4.case(name)), t4.lap64(name)
    for k in t4.LAP_TENSORS:
        err = t4.rel(got[k], want[k])
        print(name, k, "%.3g of bound %.3g" % (err, t4.BOUND))
        assert np.isfinite(got[k]).all() and err <= t4.BOUND, k
    if name == "flat":                                                             # the exact zeros, and what they hand on
        zero = np.linalg.norm(want["lv"], axis=1) == 0
        assert zero.sum() == 49 and (got["lv"][zero] == 0).all() and np.array_equal(got["lv"][81:], -t4.case(name)["verts"][81:])
        assert np.array_equal((got["lv"] == 0).all(1), zero)
        deep = np.array([1 < i % 9 < 7 and 1 < i // 9 < 7 for i in range(81)] + [False, False])       # every neighbour an exact zero too
        assert (got["d_laplacian"][deep] == 0).all() and (got["d_laplacian"][~deep] != 0).any(1).all()


@pytest.mark.parametrize("name", t4.SCALE_CASES)
def test_host_scale_against_float64(name):
    got, want = t4.host_scale(t4.case(name)), t4.scale64(name)
    for k in t4.SCALE_TENSORS:
        err = t4.rel(got[k], want[k])
        print(name, k, "%.3g of bound %.3g" % (err, t4.BOUND))
        assert err <= t4.BOUND, k
        if k.startswith("d_"):
            assert np.array_equal(got[k] == 0, want[k] == 0), k                    # the rows of an inactive hinge, column 2: exact zeros
    assert (got["d_ratio_verts"] == 0).all()
    for k in ("d_ratio_scale", "d_edge_scale", "d_var_scale"):
        assert (got[k][:, 2] == 0).all(), k
    if name == "one":
        assert np.isnan(got["scale_edge_ratio_var"]) and np.isnan(got["d_var_scale"]).sum() == 1       # the larger scale; q does not read the smaller


def test_host_decisions_at_equality():
    """`dyadic`: s0 == s1 sends both gradients to column 0; r == 5 and q == 1 are on the slope-1 side; of two equal longest edges the
    first takes the gradient; and a longest edge of length zero gives a zero vertex gradient"""
    c, got = t4.case("dyadic"), t4.host_scale(t4.case("dyadic"))
    assert got["d_edge_scale"][0, 0] != 0 and got["d_edge_scale"][0, 1] == 0 and got["d_var_scale"][0, 1] == 0
    assert got["scale_ratio"] == 0 and got["d_ratio_scale"][1, 0] == np.float32(0.25 / t4.BIG) and got["d_ratio_scale"][1, 1] == np.float32(-1.25 / t4.BIG)
    assert (got["d_ratio_scale"][[0, 2, 3]] == 0).all()
    assert got["d_edge_scale"][2, 0] == np.float32(0.25 / (5 * t4.BIG)) and (got["d_edge_verts"][[7, 8]] != 0).any(1).all() and (got["d_edge_verts"][6] == 0).all()
    assert (got["d_var_verts"][[9, 10]] != 0).any(1).all() and (got["d_var_verts"][11] == 0).all()           # edge 0 = v0 - v1 of face 3
    point = dict(c, verts=np.zeros_like(c["verts"]))
    d = t4.host_scale_backward(point, t4.WEIGHTS)
    assert (d[0] == 0).all() and np.isfinite(d[1]).all()
    # a zero upstream leaves no trace, a missing output is not written
    assert all((a == 0).all() for a in t4.host_scale_backward(t4.case("sheet"), (0, 0, 0)))
    assert t4.host_scale_backward(t4.case("sheet"), t4.WEIGHTS, want=(False, True))[0] is None


def test_division_by_the_degree_gives_exact_zeros():
    """six neighbours placed symmetrically (one diagonal direction throughout): the sum is exactly 6 v and its correctly rounded
    quotient exactly v, which a stored fp32 1 / 6 does not give"""
    n, q = 7, 2.0 ** -6
    i, j = [a.reshape(-1) for a in np.meshgrid(np.arange(n), np.arange(n))]
    verts = np.stack([i * q + 3, j * q - 1, (3 * i - j) * q], 1).astype(np.float32)
    v00 = np.array([b * n + a for b in range(n - 1) for a in range(n - 1)])
    faces = np.concatenate([np.stack([v00, v00 + 1, v00 + n + 1], 1), np.stack([v00, v00 + n + 1, v00 + n], 1)]).astype(np.int32)
    got = t4.host_lap({"verts": verts, "faces": faces})
    interior = np.array([0 < a % n < n - 1 and 0 < a // n < n - 1 for a in range(n * n)])
    start, nbr = t4.adjacency(faces, n * n)
    assert (np.diff(start)[interior] == 6).all() and (got["lv"][interior] == 0).all() and (got["lv"][~interior] != 0).any(1).all()
    sixth, stored = np.float32(1) / np.float32(6), []
    for a in np.flatnonzero(interior):                                             # the matrix row with 1 / 6 stored, summed in fp32
        s = np.zeros(3, np.float32)
        for k in nbr[start[a]:start[a + 1]]:
            s = s + sixth * verts[k]
        stored.append(s - verts[a])
    print("with a stored 1 / 6: %d of %d entries not zero, the largest %.3g" % ((np.array(stored) != 0).sum(), 3 * len(stored), np.abs(stored).max()))
    assert (np.array(stored) != 0).any()
    assert np.isfinite(got["d_laplacian"]).all()


def test_stand_alone_program_under_sanitizers(tmp_path):
    """the loops over the sheet's index structure (the adjacency with its three-face edge, the corner table), two isolated vertices
    and F = 0, as a stand-alone program built with -fsanitize=address,undefined: an index past a row or a table ends it with a report"""
    c = t4.case("sheet")
    path = tmp_path / "structure.bin"
    with open(path, "wb") as f:
        np.array([c["verts"].shape[0], c["faces"].shape[0]], np.int32).tofile(f)
        c["faces"].astype(np.int32).tofile(f)
    exe = t4.sanitizer_program()
    for args in ([str(path)], []):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
        print(r.stdout.strip(), r.stderr.strip()[:2000])
        assert r.returncode == 0 and r.stdout.startswith("ok:"), (r.returncode, r.stderr[-2000:])
        if args:
            assert "313 faces, 183 vertices" in r.stdout
