"""The constitutive update of mpmavatar_amd/csrc/mpm_math.hpp on the host, against float64, on the edge table.

tests/constitutive_ref.py holds the float64 restatement of the update and the table (families of F_trial and of cloth
directors at the shapes and thresholds where the update branches; its docstring lists them, the margins the table keeps from
the real switches, the error norms and the measured distances).  Here, without a GPU:

* ``svd3`` itself (``hm_svd`` of tests/hostmath/hostmath.cpp), property by property, on every family;
* ``traditional_update`` and the element path against float64, field by field, for the contraction-free and the
  FMA-contracted host build.  The bound is max(4 x the fp32 oracle's distance from float64 on the same family and field,
  64 * 2^-24): the oracle (OracleMPM.compute_stress) is the project's pinned restatement, not the code under test, and the
  factor covers another SVD algorithm, 1-ulp rcp / rsq and contraction;
* the float64 module against tests/golden/ref_edge_constitutive.npz, which the reference's own unchanged
  compute_stress_from_F_trial produced on the same table (tests/golden/make_golden_ref.py): a misreading shared by the
  module and the oracle cannot pass;
* the table's own margins.

What the host build still cannot see -- v_rcp_f32 / v_rsq_f32, hipcc's contraction, the wave-wide vote that ends the sweep
loop of svd3 -- tests/test_gpu_constitutive_edges.py checks on the device with the same table and the same bound.
"""
import contextlib
import os

import numpy as np
import pytest

import constitutive_ref as cr
from test_hip_math_on_host import _build as build_hostmath, hooked

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_edge_constitutive.npz")
FIXTURE_COUNT = 8            # cases per family in the committed fixture (the tests themselves use 64)
MATERIALS = list(cr.TRAD_MATERIALS)
CLOTHS = {"cloth": None, "cloth_fc0": 0.0}
SVD_TOL = 32 * 2.0 ** -24   # the sweep loop ends at 4e-7 = 6.7 * 2^-24 of relative off-diagonal; <= 6 sweeps of 3 rotations round on top


@pytest.fixture(scope="module")
def hm():
    return {"off": build_hostmath("off"), "fma": build_hostmath("fma")}


# ------------------------------------------------------------------------------------------------ fp32 runners
def oracle_trad(tab, lib=None, F_trial=None, mu=None, lam=None, ys=None):
    """compute_stress_from_F_trial of the fp32 oracle on a table of traditional particles; lib: a host build of
    mpm_math.hpp whose hm_traditional takes the place of the oracle's own restatement."""
    from oracle.oracle import OracleMPM
    F = np.asarray(tab["F_trial"] if F_trial is None else F_trial, np.float32)
    n = F.shape[0]
    o = OracleMPM(n, 0, 0, n_grid=4, grid_lim=2.0)
    s = o.sim
    s.material, s.alpha, s.hardening, s.xi = int(tab["material"]), tab["alpha"], tab["hardening"], tab["xi"]
    s.plastic_viscosity, s.softening = tab["plastic_viscosity"], tab["softening"]
    o.F_trial[:] = F
    o.mu[:], o.lam[:], o.yield_stress[:] = (tab[k] if v is None else v for k, v in (("mu", mu), ("lam", lam), ("ys", ys)))
    with (hooked(lib) if lib is not None else contextlib.nullcontext()):
        o.compute_stress(tab["dt"])
    return {"F": o.F.copy(), "stress": o.stress.copy(), "mu": o.mu.copy(), "lam": o.lam.copy(), "ys": o.yield_stress.copy()}


def oracle_cloth(tab, lib=None, d=None):
    """The element branch of the oracle's compute_stress_from_F_trial; every element owns three vertices, so that
    vertex_force holds f1, f2, f3 element by element."""
    from oracle.oracle import OracleMPM
    d = np.asarray(tab["d"] if d is None else d, np.float32)
    n = d.shape[0]
    o = OracleMPM(4 * n, n, 3 * n, n_grid=4, grid_lim=2.0)
    o.sim.friction_coeff = tab["friction_coeff"]
    o.d[:], o.R_inv[:] = d, tab["R_inv"]
    o.faces[:] = np.arange(3 * n, dtype=np.float32).reshape(n, 3)
    for k in ("vol", "mu", "lam", "gamma", "kappa"):
        getattr(o, k)[:n] = tab[k]
    with (hooked(lib) if lib is not None else contextlib.nullcontext()):
        o.compute_stress(1e-6)
    vf = o.vertex_force.reshape(n, 3, 3)
    return {"d": o.d.copy(), "stress": o.stress[:n].copy(), "f1": vf[:, 0].copy(), "f2": vf[:, 1].copy(), "f3": vf[:, 2].copy()}


def report(title, tab, want, scales, runs, cond):
    """Per family and field: the oracle's distance from float64, the bound it gives, and each run's error; returns the
    violations.  runs: {label: fields}; the entry "oracle" is the yardstick, and is itself held to ORACLE_CEILING times the
    conditioning `cond` of the field (cr.conditioning), case by case."""
    fam, names = tab["family"], tab["names"]
    odist = cr.field_errors(runs["oracle"], want, scales)
    dist = {k: cr.by_family(e, fam, names) for k, e in odist.items()}
    over = {k: cr.by_family(np.where(np.isfinite(e), e, 0.0) / cond[k], fam, names) for k, e in odist.items()}
    errs = {lab: {k: cr.by_family(e, fam, names) for k, e in cr.field_errors(got, want, scales).items()}
            for lab, got in runs.items() if lab != "oracle"}
    bad = [f"{title} {nm} {k}: the oracle itself is {v:.2e} x its conditioning from float64 (ceiling {cr.ORACLE_CEILING:.0e})"
           for k in over for nm, v in over[k].items() if not v <= cr.ORACLE_CEILING]
    print(f"\n== {title}: family, field: oracle distance -> bound | " + " | ".join(errs))
    for nm in names:
        for k in want:
            if nm not in dist[k]:      # (a family with no case in this comparison)
                continue
            b = cr.bound(dist[k][nm])
            vals = [errs[lab][k][nm] for lab in errs]
            print(f"  {nm:18s} {k:6s} {dist[k][nm]:.2e} -> {b:.2e} | " + " | ".join(f"{v:.2e}" for v in vals))
            bad += [f"{title} {nm} {k} [{lab}]: {v:.2e} > {b:.2e}" for lab, v in zip(errs, vals) if not v <= b]
    worst = {k: max(dist[k].values()) for k in want}
    print(f"  -- worst per field: oracle " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()) + "; "
          + "; ".join(f"{lab} " + ", ".join(f"{k} {max(errs[lab][k].values()):.1e}" for k in want) for lab in errs))
    return bad


# ------------------------------------------------------------------------------------------------ svd3
@pytest.mark.parametrize("contract", ["off", "fma"])
def test_svd3_properties_on_every_family(contract, hm):
    import ctypes as C
    fp = C.POINTER(C.c_float)
    lib = hm[contract]
    bad = []
    for material in MATERIALS:
        tab = cr.trad_table(material)
        A = np.ascontiguousarray(tab["F_trial"], np.float32)
        n = A.shape[0]
        U, s, V = np.zeros((n, 3, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros((n, 3, 3), np.float32)
        lib.hm_svd(A.ctypes.data_as(fp), C.c_int(n), U.ctypes.data_as(fp), s.ctypes.data_as(fp), V.ctypes.data_as(fp))
        A64, U64, s64, V64 = (a.astype(np.float64) for a in (A, U, s, V))
        nA = np.sqrt((A64 ** 2).sum((1, 2)))
        eye = np.eye(3)
        checks = {
            "U orthonormal": np.abs(np.swapaxes(U64, 1, 2) @ U64 - eye).max((1, 2)),
            "V orthonormal": np.abs(np.swapaxes(V64, 1, 2) @ V64 - eye).max((1, 2)),
            "det U = +1": np.abs(np.linalg.det(U64) - 1.0),
            "det V = +1": np.abs(np.linalg.det(V64) - 1.0),
            "U S V^T = A": np.sqrt(((cr._udv(U64, s64, V64) - A64) ** 2).sum((1, 2))) / nA,
            "singular values": np.abs(np.abs(s64) - np.linalg.svd(A64, compute_uv=False)).max(1) / nA,
            "sign of s2 = sign of det A": np.where(np.sign(s64[:, 2]) == np.sign(np.linalg.det(A64)), 0.0, np.inf),
        }
        order = (s[:, 0] >= s[:, 1]) & (s[:, 1] >= np.abs(s[:, 2])) & (s[:, 1] >= 0)
        for i, nm in enumerate(tab["names"]):
            sel = tab["family"] == i
            if not order[sel].all():
                bad.append(f"{material} {nm}: not s0 >= s1 >= |s2| with the sign in s2 only")
            for what, e in checks.items():
                if not e[sel].max() <= SVD_TOL:
                    bad.append(f"{material} {nm}: {what} off by {e[sel].max():.2e}")
        print(f"svd3[{contract}] {material}: " + ", ".join(f"{k} {v.max():.1e}" for k, v in checks.items()))
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ the update against float64
@pytest.mark.parametrize("material", MATERIALS)
def test_traditional_update_against_float64(material, hm, oracle_lib):
    tab = cr.trad_table(material)
    info = {}
    want, scales = cr.trad_reference(tab, info=info), cr.trad_scales(tab)
    assert all(np.isfinite(v).all() for v in want.values())
    runs = {"oracle": oracle_trad(tab), "host off": oracle_trad(tab, hm["off"]), "host fma": oracle_trad(tab, hm["fma"])}
    bad = report(material, tab, want, scales, runs, cr.conditioning(tab, info, scales))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("which", list(CLOTHS))
def test_element_update_against_float64(which, hm, oracle_lib):
    tab = cr.cloth_table(friction_coeff=CLOTHS[which])
    info = {}
    want, scales = cr.cloth_reference(tab, info=info), cr.cloth_scales(tab)
    assert all(np.isfinite(v).all() for v in want.values())
    runs = {"oracle": oracle_cloth(tab), "host off": oracle_cloth(tab, hm["off"]), "host fma": oracle_cloth(tab, hm["fma"])}
    bad = report(which, tab, want, scales, runs, cr.conditioning(tab, info, scales))
    assert not bad, "\n".join(bad)


def test_inverted_sand_is_nan_in_the_same_entries(hm, oracle_lib):
    """Quirk Q10: the Drucker-Prager stress takes the log of a negative singular value.  Host only -- no GPU test is handed a
    non-finite stress -- and the assertion is NaN in the same entries (and the bound on the finite ones)."""
    tab = cr.trad_table("sand", host_only=True)
    info = {}
    want, scales = cr.trad_reference(tab, info=info), cr.trad_scales(tab)
    nan = ~np.isfinite(want["stress"])
    assert nan.any() and np.isfinite(want["F"]).all()
    runs = {"oracle": oracle_trad(tab), "host off": oracle_trad(tab, hm["off"]), "host fma": oracle_trad(tab, hm["fma"])}
    for lab, got in runs.items():
        assert (np.isnan(got["stress"]) == nan).all(), lab
    bad = report("sand (inverted)", tab, want, scales, runs, cr.conditioning(tab, info, scales))
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ the table itself
def test_table_keeps_its_margins():
    """Condition, not measurement: the float64 branch variables of every case stay the stated distance away from the real
    switches (see the MARGINS paragraph of constitutive_ref), so that no case has to be left out of a comparison."""
    for fc in CLOTHS.values():
        tab, info = cr.cloth_table(friction_coeff=fc), {}
        cr.cloth_reference(tab, info=info)
        flat = tab["family"] == tab["names"].index("flat_exact")
        assert (info["r22"][flat] == 1.0).all()             # the listed exception: exactly on the switch, in float64 too
        assert (np.abs(info["r22"][~flat] - 1.0) >= cr.MARGIN_R22).all()
        fr = info["fric"][~flat]
        assert (np.abs(fr[np.isfinite(fr)]) >= cr.MARGIN_FRIC).all()
        assert info["over"].any() and info["slide"].any() and (~info["over"] & ~info["slide"]).any()
        assert ((np.linalg.det(tab["d"].astype(np.float64)) < 0) == (tab["family"] == tab["names"].index("folded"))).all()
        v = tab["verts"]
        assert (tab["d"][:, :, 0] == v[:, 1] - v[:, 0]).all() and (tab["d"][:, :, 1] == v[:, 2] - v[:, 0]).all()
    for material in MATERIALS:
        tab, info = cr.trad_table(material), {}
        want = cr.trad_reference(tab, info=info)
        if material == "sand":
            rest = info["ehn"] + np.abs(info["tr"]) <= cr.REST_EPS
            names = {tab["names"][i] for i in np.unique(tab["family"][rest])}
            assert names <= {"identity", "rotation", "signed_perm"}, names
            live = (info["dg"] > 0) & ~rest
            assert (np.abs(info["tr"][live]) >= cr.MARGIN_TR).all()
            assert ((info["dg"] > 0) & (info["tr"] > 0)).any() and ((info["dg"] > 0) & (info["tr"] < 0)).any() and (info["dg"] < 0).any()
        if material == "plasticine":
            s = info["softened"]
            assert (np.abs(s[np.isfinite(s)]) >= cr.MARGIN_SOFTEN).all()
            assert (want["mu"] == 0).any() and (want["mu"] > 0).any()
        if material in ("metal", "foam", "plasticine", "sand"):   # the ladders sit where they say, both sides of the surface
            for i, nm in enumerate(tab["names"]):
                if nm.startswith("yield_"):
                    yf = info["yield_fn"][tab["family"] == i]
                    r = 0.0 if nm == "yield_on" else float(nm.split("_")[-1]) * (-1 if "_in_" in nm else 1)
                    # (sand's rungs are placed through F itself: its rounding to fp32, 6e-8 per entry over |dev eps| >= 0.05, moves them)
                    assert np.abs(yf - r).max() <= 3e-6 + 1e-2 * abs(r), (material, nm, yf.min(), yf.max())
            assert info["changed"].any() and (~info["changed"]).any()


def test_table_is_deterministic():
    a, b = cr.trad_table("plasticine"), cr.trad_table("plasticine")
    assert all(np.array_equal(a[k], b[k]) for k in ("F_trial", "mu", "lam", "ys"))
    a, b = cr.cloth_table(), cr.cloth_table()
    assert all(np.array_equal(a[k], b[k]) for k in ("d", "verts", "R_inv", "vol", "gamma"))


# ------------------------------------------------------------------------------------------------ the reference's own source
def test_float64_module_reproduces_the_reference_fixture():
    """ref_edge_constitutive.npz: the reference's unchanged compute_stress_from_F_trial (over the NumPy stand-in of warp:
    fp32 scalars with one rounding per operation, float64 LAPACK behind svd3 / qr3) on this table, FIXTURE_COUNT cases per
    family.  An ABSOLUTE statement about the float64 module, with no yardstick that the module could move: every case and
    field within 64 * 2^-24 in the norms of the table.  The stand-in rounds every operation, not only what it stores, so the
    two ill-conditioned outputs -- the Drucker-Prager stress of a compressed, ill-conditioned F and the vertex forces, which
    carry 1 / edge -- get that bound times their conditioning, computed case by case from float64 (cr.conditioning explains
    both).  Measured: everything else <= 2.2e-6; sand stress up to 2.0e-3 at condition 1e4 (bound there 1.7e-2 ... 8e-2);
    forces up to 1.5e-5 (bound >= 7.6e-5), 9.3e-5 in the 1:100 triangles."""
    z = np.load(GOLDEN)
    bad = []

    def compare(title, tab, want, scales, got, info):
        cond = cr.conditioning(tab, info, scales)
        for k, e in cr.field_errors(got, want, scales).items():
            ratio = cr.by_family(e / cond[k], tab["family"], tab["names"])
            for nm, v in cr.by_family(e, tab["family"], tab["names"]).items():
                print(f"  fixture {title:14s} {nm:18s} {k:6s} {v:.2e} ({ratio[nm] / cr.PIN:.2f} of its bound)")
                if not ratio[nm] <= cr.PIN:
                    bad.append(f"{title} {nm} {k}: {v:.2e}, {ratio[nm] / cr.PIN:.2f} of its bound")

    for material in MATERIALS + ["sand_inverted"]:
        tab = cr.trad_table(material.split("_")[0], count=FIXTURE_COUNT, host_only=material == "sand_inverted")
        for k in ("F_trial", "mu", "lam", "ys"):
            assert np.array_equal(z[f"{material}_in_{k}"], tab[k]), (material, k)    # the fixture was made from THIS table
        got = {"F": z[f"{material}_particle_F"], "stress": z[f"{material}_particle_stress"], "mu": z[f"{material}_mu"],
               "lam": z[f"{material}_lam"], "ys": z[f"{material}_yield_stress"]}
        info = {}
        want = cr.trad_reference(tab, info=info)
        if material == "sand_inverted":
            assert np.isnan(want["stress"]).any() and (np.isnan(got["stress"]) == np.isnan(want["stress"])).all()
        compare(material, tab, want, cr.trad_scales(tab), got, info)
    for which, fc in CLOTHS.items():
        tab = cr.cloth_table(count=FIXTURE_COUNT, friction_coeff=fc)
        for k in ("d", "R_inv", "vol", "mu", "lam", "gamma", "kappa"):
            assert np.array_equal(z[f"{which}_in_{k}"], tab[k]), (which, k)
        vf = z[f"{which}_vertex_force"].reshape(-1, 3, 3)
        got = {"d": z[f"{which}_particle_d"], "stress": z[f"{which}_particle_stress"], "f1": vf[:, 0], "f2": vf[:, 1], "f3": vf[:, 2]}
        info = {}
        compare(which, tab, cr.cloth_reference(tab, info=info), cr.cloth_scales(tab), got, info)
    assert not bad, "\n".join(bad)
