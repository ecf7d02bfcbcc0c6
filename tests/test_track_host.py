"""The mesh tracking step without a GPU: the twin (tests/track_twin_torch.py) pinned against the reference's own geo_utils functions
and collision_penalty (tests/golden/track.npz); a central-difference spot check of the twin, through every quaternion branch; the
quaternion's properties (the conversion itself is UNCONFIRMED against pytorch3d); the measurement of S32, the constant the bound is
built on; the conditions the cases must meet; mpmavatar_amd/csrc/track_math.hpp compiled with g++ (tests/hosttrack/hosttrack.cpp:
serial loops that mirror the kernels) against the float64 twin; exact zeros; and the same file as a stand-alone program under
AddressSanitizer and UBSan.  Every comparison prints its figures before it asserts (run with -s)."""
import os
import subprocess

import numpy as np
import pytest
import torch

import track_cases as tc
import track_twin_torch as tw

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "track.npz")
BRANCH_FACES = range(4, 12)                  # of `ties`: two faces per quaternion branch 1, 2, 3, 0


def _long(a):
    return torch.from_numpy(np.asarray(a).astype(np.int64))


def _d(a, dtype=torch.float64):
    return torch.tensor(np.asarray(a), dtype=dtype)


# ---- the twin is the reference -----------------------------------------------------------------------------------------------

def test_twin_reproduces_the_reference():
    """tests/golden/track.npz: the reference's own functions under autograd, float64, on the cases' float32 inputs.  The matrices are
    what compute_q_from_faces hands to matrix_to_quaternion; nothing here pins the conversion behind them."""
    g = np.load(GOLD)
    assert os.path.getsize(GOLD) < 200 * 1024
    for name in tc.FIXTURE_MESHES:
        c = tc.mesh_case(name)
        faces, v = _long(c["faces"]), _d(c["verts"]).requires_grad_(True)
        vals = {"means3D": tw.barycenters(v, faces), "matrices": tw.frame_matrices(v, faces), "face_normals": tw.face_normals(v, faces),
                "face_areas": tw.face_areas(v, faces), "vertex_normals": tw.vertex_normals(v, faces)}
        pairs = {k: (t.detach().numpy(), g[f"{name}_{k}"]) for k, t in vals.items()}
        for k, w in (("means3D", c["w_means3D"]), ("matrices", c["w_matrices"]), ("face_areas", c["w_opacities"][:, 0])):
            pairs["d_" + k] = (torch.autograd.grad((_d(w) * vals[k]).sum(), v, retain_graph=True)[0].numpy(), g[f"{name}_d_{k}"])
        for k, (mine, ref) in pairs.items():
            err = tc.rel(mine, ref)
            print(name, k, "twin against the fixture %.3g" % err)
            assert ref.dtype == np.float64 and err < 1e-13, (name, k)
    for name in tc.COLLISION_CASES:
        t = tc.collision64(name)
        assert np.array_equal(t["index"], g[f"{name}_index"]), name        # direct form and expanded form agree on every row
        for k in tc.COLLISION_TENSORS:
            err = tc.rel(t[k], g[f"{name}_{k}"])
            print(name, k, "twin against the fixture %.3g" % err)
            assert g[f"{name}_{k}"].dtype == np.float64 and err < 1e-13, (name, k)


def test_twin_against_central_differences():
    """an anchor independent of autograd: central differences of the float64 twin on a vertex of the sheet's interior, its boundary and
    its fin, on one vertex of each branch face of `ties`, and on a cloth point with an active hinge"""
    h = 1e-7
    for name, spots in (("sheet", ((45, 0), (0, 2), (182, 2), (100, 1))), ("ties", tuple((3 * f + f % 3, f % 3) for f in BRANCH_FACES))):
        c, t = tc.mesh_case(name), tc.mesh64(name)
        faces = _long(c["faces"])

        def f(verts):
            out = tw.render_vars(verts, faces, _d(c["log_scales"]), _d(c["logit_opacities"]))
            return torch.stack([(_d(c["w_means3D"]) * out[0]).sum(), (_d(c["w_rotations"]) * out[1]).sum(),
                                tw.terms(verts, faces, _d(c["log_scales"]), _d(c["logit_opacities"]))[0]])

        for v, x in spots:
            up, down = _d(c["verts"]), _d(c["verts"])
            up[v, x] += h
            down[v, x] -= h
            fd = ((f(up) - f(down)) / (2 * h)).numpy()
            for i, k in enumerate(("d_means3D", "d_rotations", "d_area_verts")):
                print(name, (v, x), k, "autograd %.9g central difference %.9g" % (t[k][v, x], fd[i]))
                assert abs(fd[i] - t[k][v, x]) <= 1e-6 * np.abs(t[k]).max()
    roots = tw.quaternion_roots(tw.frame_matrices(_d(tc.mesh_case("ties")["verts"]), _long(tc.mesh_case("ties")["faces"])))
    assert sorted(roots.argmax(1)[4:].tolist()) == [0, 0, 1, 1, 2, 2, 3, 3]
    c, t = tc.collision_case("main"), tc.collision64("main")
    row = int(np.flatnonzero(c["eps"] - t["distance"] > 1e-3)[0])
    for mode in ("average", "cubed"):
        for x in range(3):
            up, down = _d(c["va"]), _d(c["va"])
            up[row, x] += h
            down[row, x] -= h
            fd = float(tw.collision(up, _d(c["vb"]), _d(c["nb"]), c["eps"], mode) - tw.collision(down, _d(c["vb"]), _d(c["nb"]), c["eps"], mode)) / (2 * h)
            print("va", (row, x), mode, "autograd %.9g central difference %.9g" % (t["d_" + mode][row, x], fd))
            assert abs(fd - t["d_" + mode][row, x]) <= 1e-6 * np.abs(t["d_" + mode]).max()


@pytest.mark.parametrize("name", tc.MESH_CASES)
def test_quaternion_properties(name):
    """what can be said of the UNCONFIRMED conversion without pytorch3d: R(q) is the frame matrix, |q| = 1 and w >= 0 -- in the twin
    (float64) and in the host build (float32, within BOUND); and `ties` takes every branch, and the sign rule both ways"""
    c = tc.mesh_case(name)
    m = tw.frame_matrices(_d(c["verts"]), _long(c["faces"]))
    for who, q, bound in (("twin", tc.mesh64(name)["rotations"], 1e-13), ("host", tc.host_mesh(c)["rotations"], tc.BOUND)):
        q = _d(q)
        back, norm, w = tc.rel(tw.quaternion_to_matrix(q).numpy(), m.numpy()), float((q.norm(dim=1) - 1).abs().max()), float(q[:, 0].min())
        print(name, who, "R(q) against the frame %.3g, | |q| - 1 | %.3g, min w %.3g, of bound %.3g" % (back, norm, w, bound))
        assert back <= bound and norm <= bound and w >= 0
    if name == "ties":
        r = tw.quaternion_roots(m)
        b = r.argmax(1)
        # w's numerator before the sign rule: r^2 > 0 on branch 0, an off-diagonal difference on branches 1-3
        raw_w = torch.stack([r[:, 0] ** 2, m[:, 2, 1] - m[:, 1, 2], m[:, 0, 2] - m[:, 2, 0], m[:, 1, 0] - m[:, 0, 1]], 1)[torch.arange(m.shape[0]), b]
        print("ties branches", b.tolist(), "w before the sign rule", raw_w.tolist())
        assert set(b.tolist()) == {0, 1, 2, 3}
        for k in (1, 2, 3):
            assert (raw_w[b == k] < 0).any() and (raw_w[b == k] > 0).any(), k


# ---- the yardstick and the conditions of the comparison ---------------------------------------------------------------------------

def test_s32_is_the_measurement():
    """a tensor that float64 leaves below TINY (the scale term and its gradient, from exp(-100)) has no relative error to measure and
    is left out; tc.rel holds the code under test to an absolute error there"""
    worst = 0.0
    for name in tc.MESH_CASES:
        t32, t64 = tc.mesh_twin(tc.mesh_case(name), torch.float32), tc.mesh64(name)
        errs = {k: tc.rel(t32[k], t64[k]) for k in tc.MESH_TENSORS if np.abs(t64[k]).max() >= tc.TINY}
        print(name, ", ".join("%s %.3g" % kv for kv in errs.items()))
        assert set(tc.MESH_TENSORS) - set(errs) == {"scale", "d_scale"}
        worst = max(worst, max(errs.values()))
    for name in tc.COLLISION_CASES:
        t32, t64 = tc.collision_twin(tc.collision_case(name), torch.float32), tc.collision64(name)
        errs = {k: tc.rel(t32[k], t64[k]) for k in tc.COLLISION_TENSORS}
        print("collision", name, ", ".join("%s %.3g" % kv for kv in errs.items()))
        assert all(np.abs(t64[k]).max() >= tc.TINY for k in tc.COLLISION_TENSORS)
        worst = max(worst, max(errs.values()))
    print("S32 measured %.4g, committed %.4g" % (worst, tc.S32))
    assert 0.5 * tc.S32 < worst <= tc.S32
    assert tc.BOUND == 10 * tc.S32


@pytest.mark.parametrize("name", tc.MESH_CASES)
def test_mesh_cases_meet_the_conditions(name):
    """over EVERY face: the longest edge (outside the constructed ties of `ties`), the largest quaternion root and the sign of
    face_area - pi s0 s1 are decided alike in the twin's float32 and float64 runs, with a margin; the structure is the stated one"""
    c = tc.mesh_case(name)
    faces, n_f = _long(c["faces"]), c["faces"].shape[0]
    dec, margins = {}, {}
    for dtype in (torch.float32, torch.float64):
        v = _d(c["verts"], dtype)
        length, root = tw.edge_lengths(v, faces), tw.quaternion_roots(tw.frame_matrices(v, faces))
        gap = tw.area_gap(v, faces, _d(c["log_scales"], dtype))
        top_l, top_r = length.sort(1, descending=True).values, root.sort(1, descending=True).values
        dec[dtype] = (length.max(1).indices.numpy(), root.argmax(1).numpy(), np.sign(gap.numpy()))
        margins[dtype] = {"edge": ((top_l[:, 0] - top_l[:, 1]) / top_l[:, 0]).numpy(), "root": (top_r[:, 0] - top_r[:, 1]).numpy(),
                          "gap": (gap.abs() / tw.face_areas(v, faces)).numpy()}
    m = margins[torch.float64]
    tied = np.zeros(n_f, bool)
    if name == "ties":
        tied[:4] = True
        assert (m["edge"][:4] == 0).all() and (margins[torch.float32]["edge"][:4] == 0).all()        # exactly equal, in both
        assert dec[torch.float64][0][:4].tolist() == [0, 1, 0, 0]                                    # the first of the longest
        assert (c["verts"] * 64 == np.round(c["verts"] * 64)).all()
    print(name, "minimum margins (float64): edge %.3g, root %.3g, |gap| / area %.3g" % (m["edge"][~tied].min() if (~tied).any() else np.inf,
                                                                                      m["root"].min(), m["gap"].min()))
    assert all(v.shape == (n_f,) for v in m.values())
    # the gap is a difference of two fp32 products of a few roundings of 2^-24 each: 1e-6 of the area is a dozen of them
    assert (m["edge"][~tied] > 1e-5).all() and (m["root"] > 1e-4).all() and (m["gap"] > 1e-6).all()
    for a, b in zip(dec[torch.float32], dec[torch.float64]):
        assert np.array_equal(a, b)
    assert (c["log_scales"][:, 2] == -100).all()
    assert n_f == 1 or ((c["logit_opacities"] > 0).any() and (c["logit_opacities"] < 0).any())
    assert n_f == 1 or ((dec[torch.float64][2] > 0).any() and (dec[torch.float64][2] < 0).any())       # both sides of the area's abs
    if name == "sheet":
        assert (n_f, c["verts"].shape[0]) == (313, 183) and n_f % tc.TPB != 0
    if name == "wide":
        assert n_f > tc.TPB * tc.TPB


@pytest.mark.parametrize("name", tc.COLLISION_CASES)
def test_collision_cases_meet_the_conditions(name):
    """over EVERY cloth point: the nearest body vertex (outside the constructed ties) and the side of the hinge (outside the
    constructed kink) are decided alike in float32 and float64, with a margin"""
    c, t64 = tc.collision_case(name), tc.collision64(name)
    n, m = tc.SIZES[name]
    assert c["va"].shape == (n, 3) and c["vb"].shape == (m, 3)
    d2 = tw.squared_distances(_d(c["va"]), _d(c["vb"])).sort(1).values
    near = ((d2[:, 1] - d2[:, 0]) / d2[:, 1]).numpy() if m > 1 else np.ones(n)
    side = np.abs(c["eps"] - t64["distance"]) / c["eps"]
    t32 = tc.collision_twin(c, torch.float32)
    tied, kink = np.zeros(n, bool), np.zeros(n, bool)
    if name == "dyadic":
        tied[list(tc.TIE_ROWS)], kink[tc.KINK_ROW] = True, True
        assert c["eps"] == 2.0 ** -10 and (near[tied] == 0).all() and side[tc.KINK_ROW] == 0
        for row, (lo, hi) in tc.TIE_ROWS.items():
            assert t64["index"][row] == lo and t32["index"][row] == lo and lo < hi
        assert t64["d_average"][tc.KINK_ROW].tolist() == (0.5 * c["nb"][500] / n).tolist()             # the slope is 1/2
        for k in ("va", "vb", "nb"):
            assert (c[k] * 1024 == np.round(c[k] * 1024)).all()
    active = c["eps"] - t64["distance"] > 0
    print(name, "minimum margins (float64): nearest %.3g, |eps - d| / eps %.3g; hinge active on %d of %d" % (near[~tied].min(), side[~kink].min(), active.sum(), n))
    assert (near[~tied] > 1e-5).all() and (side[~kink] > 1e-4).all()
    assert np.array_equal(t32["index"], t64["index"])
    assert np.array_equal(np.sign(c["eps"] - t32["distance"]), np.sign(c["eps"] - t64["distance"]))
    if n >= 300:
        assert 0.35 * n < active.sum() < 0.65 * n
    else:
        assert active.any() and (~active).any()


# ---- track_math.hpp on the host against the float64 twin ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", tc.MESH_CASES)
def test_host_mesh_against_float64(name):
    got, want = tc.host_mesh(tc.mesh_case(name)), tc.mesh64(name)
    for k in tc.MESH_TENSORS:
        err = tc.rel(got[k], want[k])
        print(name, k, "%.3g of bound %.3g" % (err, tc.BOUND))
        assert np.isfinite(got[k]).all() and err <= tc.BOUND, k


@pytest.mark.parametrize("name", tc.COLLISION_CASES)
def test_host_collision_against_float64(name):
    got, want = tc.host_collision(tc.collision_case(name)), tc.collision64(name)
    assert np.array_equal(got["index"], np.load(GOLD)[f"{name}_index"])
    for k in tc.COLLISION_TENSORS:
        err = tc.rel(got[k], want[k])
        print(name, k, "%.3g of bound %.3g" % (err, tc.BOUND))
        assert np.isfinite(got[k]).all() and err <= tc.BOUND, k
    if name == "dyadic":
        n = tc.SIZES[name][0]
        assert got["d_average"][tc.KINK_ROW].tolist() == (0.5 * tc.collision_case(name)["nb"][500] / n).tolist()
        for k in tc.COLLISION_TENSORS:
            assert np.array_equal(got[k], want[k].astype(np.float32)), k          # dyadic: exact


def test_host_exact_zeros():
    c = tc.mesh_case("sheet")
    per = tc.host_mesh(c)
    # the -100 column: subnormal or zero, never NaN or Inf
    assert 0 <= per["scale"] < 1e-40 and (per["scales"][:, 2] >= 0).all() and (per["scales"][:, 2] < 1e-40).all()
    assert np.isfinite(per["d_scale"]).all() and np.abs(per["d_scale"]).max() < 1e-40
    # a vertex in no face: gradient exactly 0 under every upstream, a NaN vertex normal, the rest unchanged
    lone = dict(c, verts=np.concatenate([c["verts"], [[1, 2, 3]]]).astype(np.float32))
    r = tc.host_mesh(lone)
    for k in ("d_means3D", "d_rotations", "d_area_verts"):
        assert (r[k][-1] == 0).all() and np.array_equal(r[k][:-1], per[k]), k
    assert np.isnan(r["vertex_normals"][-1]).all() and np.array_equal(r["vertex_normals"][:-1], per["vertex_normals"])
    # a zero upstream entry leaves no trace; a missing one counts as zeros
    only = tc.host_terms_backward(c, (0, 1, 0))
    assert (only[0] == 0).all() and (only[2] == 0).all() and (only[1][:, :2] == 0).all() and np.array_equal(only[1], per["d_scale"])
    assert all((d == 0).all() for d in tc.host_terms_backward(c, (0, 0, 0)))
    d = tc.host_render_backward(c, [c["w_means3D"], None, None, None])
    assert np.array_equal(d[0], per["d_means3D"]) and (d[1] == 0).all() and (d[2] == 0).all()
    assert tc.host_render_backward(c, [None, c["w_rotations"], None, None], want=(False, True, False))[0] is None
    # the hinge that is not active gives exactly 0, in both penalty modes; the active rows do not
    k, t = tc.collision_case("main"), tc.host_collision(tc.collision_case("main"))
    off = k["eps"] - t["distance"] < 0
    assert off.any() and (~off).any()
    for mode in ("d_average", "d_cubed"):
        assert (t[mode][off] == 0).all() and (t[mode][~off] != 0).any(1).all(), mode
    assert (t["d_distance"] != 0).any(1).all()


def test_stand_alone_program_under_sanitizers(tmp_path):
    """the loops over the sheet's index structure (the corner table, the edge with three faces) and F = 0 and n = 0, as a stand-alone
    program built with -fsanitize=address,undefined: an index past a row or a table ends it with a report"""
    c = tc.mesh_case("sheet")
    path = tmp_path / "structure.bin"
    with open(path, "wb") as f:
        np.array([c["verts"].shape[0], c["faces"].shape[0]], np.int32).tofile(f)
        c["faces"].astype(np.int32).tofile(f)
    exe = tc.sanitizer_program()
    for args in ([str(path)], []):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
        print(r.stdout.strip(), r.stderr.strip()[:2000])
        assert r.returncode == 0 and r.stdout.startswith("ok:"), (r.returncode, r.stderr[-2000:])
        if args:
            assert "313 faces, 183 vertices" in r.stdout
