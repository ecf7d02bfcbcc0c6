"""The regularisation terms of the appearance loop without a GPU: the twin (tests/reg_twin_torch.py) pinned against the reference's
own find_adjacent_faces, set-up lines, normal_loss, opacity_loss, iso_loss and area_loss (tests/golden/reg.npz); a central-difference
spot check of the twin; the measurement of S32, the constant the bound is built on; the conditions the cases must meet;
adjacent_faces against the reference's arrays; mpmavatar_amd/csrc/reg_math.hpp compiled with g++ (tests/hostreg/hostreg.cpp: serial
loops that mirror the kernels) against the float64 twin; exact zeros; and the same file as a stand-alone program under
AddressSanitizer and UBSan.  Every comparison prints its figures before it asserts (run with -s)."""
import os
import subprocess

import numpy as np
import pytest
import torch

import reg_cases as rc
import reg_twin_torch as tw

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reg.npz")
FIXTURE_MESHES = ("sheet", "closed", "one")
KINKED = ("sheet", "closed", "two", "wide")       # `one` and `flat` sit on their kinks by construction: test_host_exact_zeros


def _long(a):
    return torch.from_numpy(np.asarray(a).astype(np.int64))


# ---- the twin is the reference -----------------------------------------------------------------------------------------------

def test_twin_reproduces_the_reference():
    """tests/golden/reg.npz: the reference's own functions under autograd, float64, on the inputs of sheet, closed, one and
    Gaussians main -- which are the fixture's own, bit for bit"""
    g = np.load(GOLD)
    assert os.path.getsize(GOLD) < 200 * 1024
    for name in FIXTURE_MESHES:
        c = rc.mesh_case(name)
        for k, v in c.items():
            assert np.array_equal(g[f"{name}_{k}"], v) and g[f"{name}_{k}"].dtype == v.dtype, (name, k)
        nb = g[f"{name}_face_neighbors"]
        nd, nw = tw.setup(torch.tensor(c["verts0"], dtype=torch.float64), _long(c["faces"]), _long(nb))
        t = rc.mesh_twin(c, nb)
        pairs = {"neighbor_dist": (nd.numpy(), g[f"{name}_neighbor_dist"]), "neighbor_weight": (nw.numpy(), g[f"{name}_neighbor_weight"]),
                 "terms": (np.array([t[k] for k in rc.MESH_VALUES]), g[f"{name}_terms"])}
        pairs.update({k: (t[k], g[f"{name}_{k}"]) for k in rc.MESH_GRADS})
        for k, (mine, ref) in pairs.items():
            err = rc.rel(mine, ref)
            print(name, k, "twin against the fixture %.3g" % err)
            assert ref.dtype == np.float64 and err < 1e-13, (name, k)
    c, t = rc.gauss_case("main"), rc.gauss64("main")
    for k, v in c.items():
        assert np.array_equal(g[f"gauss_{k}"], v) and g[f"gauss_{k}"].dtype == v.dtype, k
    pairs = {"terms": (np.array([t[k] for k in rc.GAUSS_VALUES]), g["gauss_terms"])}
    pairs.update({k: (t[k], g[f"gauss_d{k}"]) for k in rc.GAUSS_GRADS})
    for k, (mine, ref) in pairs.items():
        err = rc.rel(mine, ref)
        print("gauss", k, "twin against the fixture %.3g" % err)
        assert ref.dtype == np.float64 and err < 1e-13, k


def test_twin_against_central_differences():
    """an anchor independent of autograd: central differences of the float64 twin on a handful of coordinates -- an interior vertex,
    a boundary vertex, a corner of the fin's edge, the fin's own vertex; a visible Gaussian with both terms active"""
    c, nb, g = rc.mesh_case("sheet"), rc.neighbors("sheet"), rc.mesh64("sheet")
    faces, nbl = _long(c["faces"]), _long(nb)
    nd, nw = tw.setup(torch.tensor(c["verts0"], dtype=torch.float64), faces, nbl)
    a = int(c["faces"][-1][0])
    h = 1e-7
    for v, x in ((45, 0), (0, 2), (a, 1), (182, 2), (100, 2), (13, 0)):
        up, down = [torch.tensor(c["verts"], dtype=torch.float64) for _ in range(2)]
        up[v, x] += h
        down[v, x] -= h
        fd = ((tw.mesh_terms(up, faces, nbl, nd, nw) - tw.mesh_terms(down, faces, nbl, nd, nw)) / (2 * h)).numpy()
        for i, k in enumerate(rc.MESH_GRADS):
            print("verts", (v, x), k, "autograd %.9g central difference %.9g" % (g[k][v, x], fd[i]))
            assert abs(fd[i] - g[k][v, x]) <= 1e-6 * np.abs(g[k]).max()
    c, g = rc.gauss_case("main"), rc.gauss64("main")
    vis = torch.from_numpy(c["radii"] > 0)
    a, b = tw.gauss_parts(torch.tensor(c["_xyz"], dtype=torch.float64), torch.tensor(c["_scaling"], dtype=torch.float64), *rc.THRESHOLDS)
    row = int(np.flatnonzero(vis.numpy() & (a.numpy() > 0) & (b.numpy() > 0).any(1))[0])
    h = 1e-6
    for k, at in (("_opacity", (row, 0)), ("_xyz", (row, 1)), ("_scaling", (row, int((b[row] > 0).nonzero()[0])))):
        t = {n: torch.tensor(c[n], dtype=torch.float64) for n in rc.GAUSS_GRADS}
        t[k][at] += h
        up = tw.gauss_terms(t["_opacity"], t["_xyz"], t["_scaling"], vis, *rc.THRESHOLDS).sum()
        t[k][at] -= 2 * h
        fd = float(up - tw.gauss_terms(t["_opacity"], t["_xyz"], t["_scaling"], vis, *rc.THRESHOLDS).sum()) / (2 * h)
        print(k, at, "autograd %.9g central difference %.9g" % (g[k][at], fd))
        assert g[k][at] != 0 and abs(fd - g[k][at]) <= 1e-6 * np.abs(g[k]).max()


# ---- the yardstick and the conditions of the comparison ---------------------------------------------------------------------------

def test_s32_is_the_measurement():
    """a tensor that float64 leaves below TINY (`one`, `flat`: exact zeros and sqrt(1e-20) constants) has no relative error to
    measure and is left out; rc.rel holds the code under test to an absolute error there"""
    worst = 0.0
    for name in rc.MESH_CASES:
        t32 = rc.mesh_twin(rc.mesh_case(name), rc.neighbors(name), torch.float32)
        errs = {k: rc.rel(t32[k], rc.mesh64(name)[k]) for k in rc.MESH_TENSORS if np.abs(rc.mesh64(name)[k]).max() >= rc.TINY}
        print(name, ", ".join("%s %.3g" % kv for kv in errs.items()))
        worst = max(worst, max(errs.values(), default=0.0))
    for name in rc.GAUSS_CASES:
        t32, t64 = rc.gauss_twin(rc.gauss_case(name), torch.float32), rc.gauss64(name)
        errs = {k: rc.rel(t32[k], t64[k]) for k in rc.GAUSS_TENSORS if not np.isnan(t64[k]).any()}
        print("gauss", name, ", ".join("%s %.3g" % kv for kv in errs.items()))
        worst = max(worst, max(errs.values()))
    print("S32 measured %.4g, committed %.4g" % (worst, rc.S32))
    assert 0.5 * rc.S32 < worst <= rc.S32
    assert rc.BOUND == 10 * rc.S32


@pytest.mark.parametrize("name", KINKED)
def test_mesh_cases_meet_the_conditions(name):
    """over EVERY face and neighbour: the sign of m_f - 1, the sign of a_f - mean(a) and, for a neighbour that is not the face
    itself, the sign of mag - nd are the same in the twin's float32 and float64 runs (nothing left out); the index structure is the
    stated one"""
    c, nb = rc.mesh_case(name), rc.neighbors(name)
    faces, nbl = _long(c["faces"]), _long(nb)
    n_f = faces.shape[0]
    own = nb == np.arange(n_f)[:, None]
    signs, margins = {}, {}
    for dtype in (torch.float32, torch.float64):
        nd, _ = tw.setup(torch.tensor(c["verts0"], dtype=dtype), faces, nbl)
        m, a, mag = tw.mesh_parts(torch.tensor(c["verts"], dtype=dtype), faces, nbl, nd)
        parts = {"1 - m_f": (1 - m).numpy(), "(a_f - mean) / mean": ((a - a.mean()) / a.mean()).numpy(),
                 "(mag - nd) / nd": ((mag - nd) / nd.clamp(min=1e-30)).numpy()[~own]}
        signs[dtype] = {k: np.sign(v) for k, v in parts.items()}
        margins[dtype] = {k: float(np.abs(v).min()) for k, v in parts.items()}
    print(name, "minimum margins (float64):", ", ".join("%s %.3g" % kv for kv in margins[torch.float64].items()))
    for k in signs[torch.float64]:
        assert signs[torch.float64][k].shape[0] in (n_f, int((~own).sum()))
        assert (signs[torch.float64][k] != 0).all() and np.array_equal(signs[torch.float32][k], signs[torch.float64][k]), k
    sym = all(f in nb[j] for f in range(n_f) for j in nb[f] if j != f) if n_f < 1000 else None
    if name == "sheet":
        per_edge = np.bincount(np.unique(np.sort(np.stack([c["faces"], c["faces"][:, [1, 2, 0]]], 2).reshape(-1, 2), 1), axis=0, return_inverse=True)[1].reshape(-1))
        assert (n_f, c["verts"].shape[0]) == (313, 183) and n_f > rc.TPB and n_f % rc.TPB != 0
        assert int(own.any(1).sum()) == 47 and per_edge.max() == 3 and (per_edge == 3).sum() == 1 and sym is False
    if name == "closed":
        assert (n_f, c["verts"].shape[0]) == (80, 42) and not own.any() and sym is True
    if name == "two":
        assert np.array_equal(nb, [[1, 0, 0], [0, 1, 1]])
    if name == "wide":
        assert n_f > rc.TPB * rc.TPB and 2 * (rc.WIDE[0] - 1) * rc.WIDE[1] <= rc.TPB * rc.TPB and -(-n_f // rc.TPB) > rc.TPB


@pytest.mark.parametrize("name", ("main", "one"))
def test_gauss_cases_meet_the_conditions(name):
    """over EVERY Gaussian and component: both relus and the zero-row test are decided alike in float32 and float64"""
    c = rc.gauss_case(name)
    vis = c["radii"] > 0
    dec = {}
    for dtype in (torch.float32, torch.float64):
        a, b = tw.gauss_parts(torch.tensor(c["_xyz"], dtype=dtype), torch.tensor(c["_scaling"], dtype=dtype), *rc.THRESHOLDS)
        dec[dtype] = (a.numpy(), b.numpy())
    a64, b64 = dec[torch.float64]
    print(name, "minimum margins (float64): |xyz| - t %.3g, exp(s) - t %.3g" % (np.abs(a64).min(), np.abs(b64).min()))
    assert np.array_equal(dec[torch.float32][0] > 0, a64 > 0) and np.array_equal(dec[torch.float32][1] > 0, b64 > 0)
    assert np.abs(a64).min() > 1e-5 and np.abs(b64).min() > 1e-5
    if name == "main":
        zero_rows = vis & ~(b64 > 0).any(1)
        print("visible %d, xyz active %d, visible all-zero scale rows %d" % (vis.sum(), (vis & (a64 > 0)).sum(), zero_rows.sum()))
        assert c["_xyz"].shape[0] == 300 and 200 <= vis.sum() <= 250 and (vis & (a64 > 0)).sum() >= 50 and zero_rows.sum() >= 50
        assert (vis & (b64 > 0).any(1) & ~(b64 > 0).all(1)).sum() >= 20         # rows with some components at the relu, some not


@pytest.mark.parametrize("name", FIXTURE_MESHES)
def test_adjacent_faces_is_the_references_array(name):
    ref = np.load(GOLD)[f"{name}_face_neighbors"]
    mine = rc.neighbors(name)
    assert mine.shape == ref.shape and np.array_equal(mine, ref)
    if name == "sheet":
        from mpmavatar_amd.regularizers import adjacent_faces
        assert np.array_equal(adjacent_faces(torch.from_numpy(np.asarray(rc.mesh_case(name)["faces"]))), ref)     # a tensor too
        assert adjacent_faces(np.zeros((0, 3), np.int32)).shape == (0, 3)


# ---- reg_math.hpp on the host against the float64 twin ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", rc.MESH_CASES + ("wide",))
def test_host_mesh_against_float64(name):
    got, want = rc.host_mesh(rc.mesh_case(name), rc.neighbors(name)), rc.mesh64(name)
    for k in rc.MESH_TENSORS:
        err = rc.rel(got[k], want[k])
        print(name, k, "%.3g of bound %.3g" % (err, rc.BOUND))
        assert np.isfinite(got[k]).all() and err <= rc.BOUND, k


@pytest.mark.parametrize("name", rc.GAUSS_CASES)
@pytest.mark.parametrize("mask", (False, True), ids=("radii", "mask"))
def test_host_gauss_against_float64(name, mask):
    c = rc.gauss_case(name)
    got, want = rc.host_gauss(c, mask=mask), rc.gauss64(name)
    assert got["n_visible"] == int((c["radii"] > 0).sum())
    for k in rc.GAUSS_TENSORS:
        if np.isnan(want[k]).any():
            assert name == "none_visible" and k in ("xyz", "scale") and np.isnan(got[k])
            continue
        err = rc.rel(got[k], want[k])
        print(name, k, "%.3g of bound %.3g" % (err, rc.BOUND))
        assert np.isfinite(got[k]).all() and err <= rc.BOUND, k
    if mask:
        plain = rc.host_gauss(c)
        for k in rc.GAUSS_TENSORS:
            assert np.array_equal(got[k], plain[k], equal_nan=True), k


def test_host_setup_is_the_references():
    """neighbor_dist and neighbor_weight as MeshRegularizer takes them (a forward on verts0 that stores the squared distances)
    against the fixture's"""
    g = np.load(GOLD)
    for name in FIXTURE_MESHES:
        nd, nw = rc.host_setup(rc.mesh_case(name), rc.neighbors(name))
        for k, mine in (("neighbor_dist", nd), ("neighbor_weight", nw)):
            err = rc.rel(mine, g[f"{name}_{k}"])
            print(name, k, "%.3g of bound %.3g" % (err, rc.BOUND))
            assert mine.dtype == np.float32 and err <= rc.BOUND
        own = rc.neighbors(name) == np.arange(nd.shape[0])[:, None]
        assert (nd[own] == 0).all() and (nw[own] == 1).all()


def test_host_exact_zeros():
    # flat: every dot product is exactly 1, every area the same, every distance its own neighbor_dist
    c, nb = rc.mesh_case("flat"), rc.neighbors("flat")
    assert (c["verts"] * 64 == np.round(c["verts"] * 64)).all() and np.array_equal(c["verts"], c["verts0"])
    r = rc.host_mesh(c, nb)
    assert r["normal"] == 0 and r["area"] == 0 and 0 < r["iso"] < 2e-10
    for k in rc.MESH_GRADS:
        assert (r[k] == 0).all(), k
    assert np.abs(rc.mesh64("flat")["d_iso"]).max() < 1e-10          # what float64 leaves of that zero
    # one: every neighbour is the face itself
    r = rc.host_mesh(rc.mesh_case("one"), rc.neighbors("one"))
    assert r["normal"] <= 2.0 ** -22 and r["area"] == 0
    for k in rc.MESH_GRADS:
        assert (r[k] == 0).all(), k
    # the self-neighbour slots of the sheet receive exactly nothing, under all three terms at once; the other slots do
    c, nb = rc.mesh_case("sheet"), rc.neighbors("sheet")
    full = rc.host_mesh(c, nb, g=(0.1, 20.0, 1000.0))
    own = nb == np.arange(nb.shape[0])[:, None]
    assert own.any() and (full["d_stencil"][:, 1:][own] == 0).all() and (full["d_stencil"][:, 1:][~own] != 0).any(-1).any(-1).all()
    assert (full["d_stencil"][:, 0] != 0).any(-1).any(-1).all()
    # a zero entry of the upstream: that term leaves no trace
    per = rc.host_mesh(c, nb)
    only = rc.host_mesh(c, nb, g=(0.0, 1.0, 0.0))
    assert np.array_equal(only["d_verts"], per["d_iso"])
    assert (rc.host_mesh(c, nb, g=(0.0, 0.0, 0.0))["d_verts"] == 0).all()
    # a vertex in no face gets exactly 0
    lone = {"faces": c["faces"], "verts0": np.concatenate([c["verts0"], [[1, 2, 3]]]).astype(np.float32),
            "verts": np.concatenate([c["verts"], [[1, 2, 3]]]).astype(np.float32)}
    r = rc.host_mesh(lone, nb)
    for k in rc.MESH_GRADS:
        assert (r[k][-1] == 0).all() and np.array_equal(r[k][:-1], per[k]), k
    # the invisible Gaussians; and with none visible every filtered gradient
    g = rc.gauss_case("main")
    r = rc.host_gauss(g)
    hidden = g["radii"] == 0
    assert hidden.any() and (r["_xyz"][hidden] == 0).all() and (r["_scaling"][hidden] == 0).all()
    assert (r["_xyz"][~hidden] != 0).any() and (r["_scaling"][~hidden] != 0).any() and (r["_opacity"] != 0).all()
    b = np.exp(g["_scaling"].astype(np.float64)) - rc.THRESHOLDS[1]
    assert (r["_scaling"][b <= 0] == 0).all() and (r["_scaling"][~hidden][(b > 0)[~hidden]] != 0).all()      # a relu that binds: zero slope
    r = rc.host_gauss(rc.gauss_case("none_visible"))
    assert np.isnan(r["xyz"]) and np.isnan(r["scale"]) and np.isfinite(r["opacity"]) and r["n_visible"] == 0
    assert (r["_xyz"] == 0).all() and (r["_scaling"] == 0).all() and np.array_equal(r["_opacity"], rc.host_gauss(g)["_opacity"])


def test_stand_alone_program_under_sanitizers(tmp_path):
    """the loops over the sheet's index structure (the cut rows, the 47 self rows, the stencil table) and F = 0 and n = 0, as a
    stand-alone program built with -fsanitize=address,undefined: an index past a row or a table ends it with a report"""
    c, nb = rc.mesh_case("sheet"), rc.neighbors("sheet")
    path = tmp_path / "structure.bin"
    with open(path, "wb") as f:
        np.array([c["verts"].shape[0], c["faces"].shape[0]], np.int32).tofile(f)
        c["faces"].astype(np.int32).tofile(f)
        nb.astype(np.int32).tofile(f)
    exe = rc.sanitizer_program()
    for args in ([str(path)], []):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
        print(r.stdout.strip(), r.stderr.strip()[:2000])
        assert r.returncode == 0 and r.stdout.startswith("ok:"), (r.returncode, r.stderr[-2000:])
        if args:
            slots = int((nb == np.arange(nb.shape[0])[:, None]).sum())
            assert f"313 faces, 183 vertices, {slots} self slots" in r.stdout
