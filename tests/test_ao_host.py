"""The AO bake on the CPU: mpmavatar_amd/csrc/ao_math.hpp compiled for the host (tests/hostao) against the float64 twin
(tests/ao_twin.py) and against known answers, before any GPU sees the kernels.  The cases are tests/ao_cases.py."""
import os
import subprocess

import numpy as np
import pytest

import ao_cases as ac
import ao_twin as tw
from hostbuild import host_program

baked = ac.baked


@pytest.mark.parametrize("name", ["A", "C0", "D"])
def test_coverage_equals_the_twin(name):
    h = baked(name)
    case = h["case"]
    face, bary = tw.coverage(case.faces, case.vt, case.ft, case.height, case.width)
    assert (h["face"] >= 0).sum() > 50
    assert np.array_equal(h["face"], face)
    assert np.abs(h["bary"] - bary).max() <= 1e-6
    cov = h["face"] >= 0
    b = h["bary"][cov].astype(np.float64)
    assert b.min() >= -1e-6 and (b.sum(1) <= 1 + 1e-6).all()
    assert not h["bary"][~cov].any()


def test_degenerate_faces_cover_nothing_and_the_lowest_face_wins():
    h = baked("D")
    n = len(ac.case_c(0).faces)
    face = h["face"]
    assert not np.isin(face, [n, n + 1, n + 2]).any()     # no area, no UV area, and the copy of face 5's UV triangle
    assert (face == 5).sum() > 0
    assert np.array_equal(face, baked("C0")["face"])       # the additions changed nothing of what C covers


@pytest.mark.parametrize("name", ["A", "C0", "D"])
def test_frames_against_the_twin(name):
    h = baked(name)
    case = h["case"]
    o, n, t, b = tw.frames(case.verts, case.faces, h["face"], h["bary"], h["rot"])
    for got, want in ((h["o"], o), (h["n"], n), (h["t"], t), (h["b"], b)):
        assert np.abs(got - want).max() <= 2e-6
    cov = h["face"] >= 0
    nn, tt, bb = (h[k][cov].astype(np.float64) for k in ("n", "t", "b"))
    for a in (nn, tt, bb):
        assert np.abs(np.linalg.norm(a, axis=1) - 1).max() <= 1e-6
    for a, c in ((nn, tt), (nn, bb), (tt, bb)):
        assert np.abs((a * c).sum(1)).max() <= 1e-6
    assert np.abs(np.cross(nn, tt) - bb).max() <= 1e-6
    assert not h["o"][~cov].any() and not h["n"][~cov].any() and not h["t"][~cov].any()
    if name == "A":
        assert np.array_equal(h["n"][cov], np.tile(np.float32([0, 1, 0]), (cov.sum(), 1)))


def _walk_equals_brute(verts, faces, o, d, cap_cells):
    walked, dims = ac.host_ray_faces(verts, faces, o, d, False, cap_cells)
    brute, _ = ac.host_ray_faces(verts, faces, o, d, True, cap_cells)
    assert brute.any()
    assert np.array_equal(walked, brute)
    return dims, brute


@pytest.mark.parametrize("name", ["C0", "C1", "C2", "B"])
def test_the_grid_walk_finds_what_brute_force_finds(name):
    """every ray of the case: the set of faces hit while walking the grid is the set hit by trying every face, same predicate"""
    h = baked(name)
    case = h["case"]
    o, d = ac.rays_of(h["o"], h["n"], h["t"], h["b"], h["dirs"], h["face"])
    dims, brute = _walk_equals_brute(case.verts, case.faces, o, d, case.cap_cells)
    if name == "B":
        assert dims[1] == 1 and dims[0] > 1                # one cell across the thin axis
        assert brute[:, -2:].any(1).all()                  # every ray meets the plate
    else:
        assert min(dims[:3]) > 1
    # the whole bake, grid against brute force
    _, occ = ac.host_bake(case, h["face"], h["bary"], h["rot"], h["dirs"], brute=True)
    assert np.array_equal(occ, h["occ"])


@pytest.mark.parametrize("cap_cells", [1, 40, 4096, 1 << 21])
def test_the_grid_walk_on_a_triangle_soup(cap_cells):
    verts, faces, o, d = ac.soup()
    dims, brute = _walk_equals_brute(verts, faces, o, d, cap_cells)
    assert dims[0] * dims[1] * dims[2] <= cap_cells
    assert brute.sum() > 2000                              # the rays do meet the soup


def test_a_flat_sheet_gets_one_padded_cell_across():
    a = ac.case_a()
    o = np.float32([[0.01, 0.0, 0.02], [0.01, -1.0, 0.02]])
    d = np.float32([[0.6, 0.0, 0.8], [0.0, 1.0, 0.0]])      # inside the sheet's plane; through it from below
    hits, dims = ac.host_ray_faces(a.verts, a.faces, o, d, False, a.cap_cells)
    brute, _ = ac.host_ray_faces(a.verts, a.faces, o, d, True, a.cap_cells)
    assert dims[1] == 1 and dims[0] >= 4 and dims[2] >= 4
    assert np.array_equal(hits, brute) and hits[1].sum() >= 1 and not hits[0].any()


@pytest.mark.parametrize("name", ["C0", "C1", "C2"])
def test_fp32_predicate_against_float64(name):
    """A condition, not a measurement: on the same fp32 frames and tables the fp32 predicate and float64 disagree on at most 0.1 % of
    the rays, and no texel is off by more than 2 rays."""
    h = baked(name)
    case = h["case"]
    want = tw.occluded(case.verts, case.faces, h["face"], h["o"], h["n"], h["t"], h["dirs"], ac.BIAS, ac.MAX_DISTANCE)
    cov = h["face"] >= 0
    rays = cov.sum() * case.samples
    diff = np.abs(want.sum(1) - h["occ"])
    mean_ao = h["ao"][cov].mean()
    print(f"{name}: {rays} rays, {diff.sum()} differing counts, worst texel {diff.max()}, mean AO {mean_ao:.3f}, "
          f"open {np.mean(h['occ'][cov] == 0):.2f}, closed {np.mean(h['occ'][cov] == case.samples):.2f}")
    assert diff.sum() <= 1e-3 * rays
    assert diff.max() <= 2
    assert 0.3 < mean_ao < 0.95 and (h["occ"][cov] == 0).any()          # not one-sided


def test_known_answers_open_sheet_and_lid():
    a, b = baked("A"), baked("B")
    cov = a["face"] >= 0
    assert cov.sum() > 500 and np.array_equal(cov, b["face"] >= 0)
    assert (a["ao"][cov] == 1.0).all() and (a["ao"][~cov] == 0.0).all()
    assert (b["ao"][cov] == 0.0).all() and (b["occ"][cov] == b["case"].samples).all()
    assert b["dirs"][:, 2].min() > 0.088


def test_margin_rule_on_a_hand_made_coverage():
    mask = np.array([[0, 0, 0, 0, 0],
                     [0, 1, 1, 0, 0],
                     [0, 1, 0, 0, 0],
                     [0, 0, 0, 0, 0],
                     [0, 0, 0, 0, 1]], np.uint8)
    val = np.where(mask, np.arange(25).reshape(5, 5) / 32.0, 0.0).astype(np.float32)     # (1,1) = 6/32, (1,2) = 7/32, (2,1) = 11/32, (4,4) = 24/32
    out, m = ac.host_margin(val.reshape(-1), mask.reshape(-1), 5, 5)
    out, m = out.reshape(5, 5), m.reshape(5, 5)
    f = np.float32
    assert np.array_equal(out[mask == 1], val[mask == 1])
    assert out[0, 0] == f(6 / 32) and out[2, 2] == (f(6 / 32) + f(7 / 32) + f(11 / 32)) / f(3)
    assert out[0, 1] == (f(6 / 32) + f(7 / 32)) / f(2) and out[3, 3] == f(24 / 32) and out[2, 3] == f(7 / 32)
    assert out[0, 4] == 0 and not m[0, 4] and out[4, 0] == 0 and not m[4, 0] and out[4, 2] == 0
    assert m.sum() == 4 + 15
    tv, tm = tw.margin(val.reshape(-1), mask.reshape(-1), 5, 5)
    assert np.array_equal(tm.reshape(5, 5), m.astype(bool)) and np.abs(tv.reshape(5, 5) - out).max() < 1e-7
    out2, m2 = ac.host_margin(out.reshape(-1), m.reshape(-1), 5, 5)      # a second pixel grows from the first
    assert m2.reshape(5, 5)[0, 4] and out2.reshape(5, 5)[0, 4] == (out[0, 3] + out[1, 3]) / f(2)


def test_uv_template_is_read_as_the_obj_writer_reads_it(tmp_path):
    """AOBaker.from_uv_obj's parser against io_formats.UVMeshWriter on one template: the 'vt' rows and the index after the slash"""
    from mpmavatar_amd import io_formats
    from mpmavatar_amd.ao_bake import read_uv_template
    c = ac.baked("C0")["case"]
    path = tmp_path / "uv.obj"
    with open(path, "w") as f:
        f.writelines(f"v {v[0]} {v[1]} {v[2]}\n" for v in c.verts)
        f.writelines(f"vt {t[0]} {t[1]}\n" for t in c.vt)
        f.write("vn 0 1 0\n# a comment\n")
        f.writelines(f"f {a[0] + 1}/{b[0] + 1}/1 {a[1] + 1}/{b[1] + 1}/1 {a[2] + 1}/{b[2] + 1}/1\n" for a, b in zip(c.faces, c.ft))
    vt, ft = read_uv_template(str(path))
    assert vt.dtype == np.float32 and ft.dtype == np.int32
    assert np.array_equal(vt, c.vt) and np.array_equal(ft, c.ft)
    lines = io_formats.UVMeshWriter(str(path), c.faces).vt_f
    assert [ln for ln in lines if ln[:2] == "f "] == [f"f {a[0] + 1}/{b[0] + 1} {a[1] + 1}/{b[1] + 1} {a[2] + 1}/{b[2] + 1}\n" for a, b in zip(c.faces, ft)]


# the twin's own error against R^2 / (R^2 + h^2), measured on the CPU with the tangent turned by 0.3 rad:
#   (R, h)        S = 64     S = 256
#   (0.5, 0.5)    +0.00000   +0.00000
#   (1.0, 0.5)    -0.00313   +0.00078
#   (0.3, 1.0)    -0.00444   -0.00054
# (with r = sqrt(u) and u in S equal strata the count can be off by one ray at the most: 1 / S = 0.0156 and 0.0039.)
# The tolerance is twice the worst of each column (the 64-gon's missing slivers and the table's discrepancy).
FORM_FACTOR_TOL = {64: 2 * 0.00444, 256: 2 * 0.00078}


@pytest.mark.parametrize("samples", [64, 256])
@pytest.mark.parametrize("radius,h", [(0.5, 0.5), (1.0, 0.5), (0.3, 1.0)])
def test_form_factor_of_a_disc(radius, h, samples):
    """sanity of the direction table (not of the kernel): the cosine-weighted fraction a disc over the texel stops"""
    got = tw.disc_fraction(radius, h, samples, angle=0.3)
    want = radius ** 2 / (radius ** 2 + h ** 2)
    print(f"R = {radius}, h = {h}, S = {samples}: {got:.5f} against {want:.5f}, error {got - want:+.5f}")
    assert abs(got - want) <= FORM_FACTOR_TOL[samples]
    from mpmavatar_amd.ao_bake import direction_table
    assert np.abs(direction_table(samples) - tw.directions(samples)).max() <= 6e-8       # the product's table is the twin's, rounded


def test_stand_alone_program_under_the_sanitizers():
    """the host build as a program of its own, with AddressSanitizer and UBSan, through every loop"""
    exe = host_program("hostao", name="hostao_asan", flags=["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DHOSTAO_MAIN"])
    r = subprocess.run([exe], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0 and r.stdout.startswith("ok:"), r.stdout + r.stderr
