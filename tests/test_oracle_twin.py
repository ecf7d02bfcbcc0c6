"""The fp32 C oracle against the independent float64 NumPy twin (oracle/twin.py) on whole substeps.

The twin uses closed forms (Gram-Schmidt QR, 2x2 polar rotation, LAPACK SVD) where the oracle restates Warp's qr3 /
svd3 + the reference's sign flips, so agreement checks both the transcription and the convention handling.
Cloth scenes decorrelate in velocity after a few dozen substeps because the reference's anisotropic return mapping is
discontinuous at R22 == 1 (mpm_utils.py:196-204); the strict bounds therefore apply to the first substeps and to
positions, and the long-run velocity bound is looser (documented in DESIGN.md, section "Parity").
"""
import numpy as np
import pytest

from mpmavatar_amd import scenes
from oracle.scene_adapter import oracle_from_scene, run_scene
from oracle.twin import TwinMPM


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-3))


def pair(sc, n):
    o, t = oracle_from_scene(sc), TwinMPM(sc)
    run_scene(o, sc, n)
    run_scene(t, sc, n)
    return o, t


@pytest.mark.parametrize("material,params", [("jelly", {}), ("sand", {"friction_angle": 40.0})])
def test_cube_100_substeps(material, params, oracle_lib):
    o, t = pair(scenes.small_cube(material=material, params=params), 100)
    assert rel(o.x, t.x) < 1e-5 and rel(o.v, t.v) < 2e-4 and rel(o.F_trial, t.F_trial) < 1e-5


# The spinning cube strains itself to |dev tau| <= 0.035: yield stresses just under that put part of it through the return maps
# (measured: 2 % / 3 % / 0.4 % of all particle-substeps for metal / foam / plasticine, 14 % of the particles; 13 % of the plasticine ends with mu = lam = 0).
PLASTIC = [("metal", {"yield_stress": 0.025, "hardening": 1, "xi": 0.1}),
           ("foam", {"yield_stress": 0.03, "plastic_viscosity": 0.01}),
           ("plasticine", {"yield_stress": 0.025, "hardening": 1, "xi": 0.1, "softening": 300.0})]


@pytest.mark.parametrize("material,params", PLASTIC)
def test_plastic_cube_100_substeps(material, params, oracle_lib):
    """Hardening, viscoplastic flow and damage softening at the bounds of the elastic cube -- and they must have happened."""
    sc = scenes.small_cube(material=material, params=params)
    o, t = pair(sc, 100)
    assert rel(o.x, t.x) < 1e-5 and rel(o.v, t.v) < 2e-4 and rel(o.F_trial, t.F_trial) < 1e-5
    n, ys0 = sc.n_traditional, np.float32(params["yield_stress"])
    returned = t.n_returned / (100.0 * n)
    print(f"{material}: {returned:.4f} of the particle-substeps went through the return map; ys changed on "
          f"{(t.ys != ys0).mean():.2f} / {(o.yield_stress != ys0).mean():.2f} of the particles (twin / oracle); "
          f"mu = 0 on {(t.mu == 0).mean():.2f} / {(o.mu == 0).mean():.2f}")
    assert returned > {"metal": 0.01, "foam": 0.015, "plasticine": 0.002}[material]
    if material == "foam":
        assert (t.ys == ys0).all() and (o.yield_stress == ys0).all()      # the viscoplastic map leaves ys alone
    else:
        assert (t.ys != ys0).mean() > 0.1 and (o.yield_stress != ys0).mean() > 0.1     # measured 0.14, both
        sign = 1 if material == "metal" else -1                           # hardening raises ys; softening at 300 outweighs it
        assert (sign * (t.ys[t.ys != ys0] - ys0) > 0).all()
    if material == "plasticine":
        dead_t, dead_o = t.mu == 0, o.mu == 0
        assert dead_t.mean() > 0.05 and dead_o.mean() > 0.05 and (dead_t != dead_o).mean() < 0.01
        assert (t.lam[dead_t] == 0).all() and (t.ys[dead_t] <= 0).all()
    else:
        assert (t.mu > 0).all() and (o.mu > 0).all()


@pytest.mark.parametrize("params", [{"rpic_damping": 0.3}, {"rpic_damping": -1.0}, {"grid_v_damping_scale": 0.9},
                                    {"rpic_damping": 0.5, "grid_v_damping_scale": 0.97}])
def test_rpic_and_grid_damping(params, oracle_lib):
    """p2g's RPIC blend / PIC switch (mpm_utils.py:528-540) and add_damping_via_grid (:1162-1174, mpm_solver.py:373)."""
    o, t = pair(scenes.small_cube(n=6, params=params), 60)
    assert rel(o.x, t.x) < 1e-5 and rel(o.v, t.v) < 2e-4
    assert np.abs(o.C - t.C).max() < 1e-4   # absolute: C is tiny under damping, fp32 cancellation noise is not


def test_sheet_first_substep_strict(oracle_lib):
    o, t = pair(scenes.small_sheet(), 1)
    assert rel(o.x, t.x) < 1e-6 and rel(o.v, t.v) < 2e-5 and rel(o.C, t.C) < 5e-5 and rel(o.d, t.d) < 1e-6
    G = o.n_grid
    assert rel(o.grid_m, t.grid_m) < 1e-5
    act = t.grid_m > 1e-14
    assert rel(o.grid_v_out[act], t.grid_v_out[act]) < 1e-4


def test_sheet_200_substeps(oracle_lib):
    o, t = pair(scenes.small_sheet(), 200)
    assert rel(o.x, t.x) < 1e-5 and rel(o.v, t.v) < 5e-3   # cloth on the R22 = 1 discontinuity: see tests/test_ref_golden.py


def test_garment_with_collider_and_mover(oracle_lib):
    o, t = pair(scenes.small_garment(), 100)
    assert rel(o.x, t.x) < 1e-5 and rel(o.v, t.v) < 5e-3


def test_demo_mix(oracle_lib):
    o, t = pair(scenes.demo_mix(n_grid=48, n_sheet=16, sand=(16, 3, 8)), 60)
    assert rel(o.x, t.x) < 1e-5 and rel(o.v, t.v) < 1e-3 and rel(o.F_trial, t.F_trial) < 1e-5


def test_openmp_build_matches_serial(oracle_lib):
    sc = scenes.small_garment()
    a = oracle_from_scene(sc)
    b = oracle_from_scene(sc, omp=True, n_threads=4)
    run_scene(a, sc, 10)
    run_scene(b, sc, 10)
    assert rel(b.x, a.x) < 1e-6 and rel(b.v, a.v) < 1e-3


@pytest.mark.parametrize("surface", ["sticky", "cut"])
def test_moving_cuboid_with_reset_and_plane_kinds(surface, oracle_lib):
    """Grid BCs the twin states independently: a velocity cuboid that drags part of a cube along, moves with its own
    velocity (host-side modify, mpm_solver.py:975-981), ends and zeroes the whole grid for 15 more substeps (reset = 1,
    :968-970), over a plane of kind 'sticky' / 'cut' (:600-655; the cut band keeps 0.3 * (vx, 0, vz) for 0.4 <= z <= 0.53)."""
    sc = scenes.small_cube(n=6)
    lo = float(sc.x[:, 1].min())
    c = sc.x.mean(0)
    sc.bcs = [("bounding_box", {}),
              ("surface_collider", {"point": [0.0, lo + 0.02, 0.0], "normal": [0.0, 1.0, 0.0], "surface": surface, "friction": 0.0}),
              ("velocity_cuboid", {"point": [float(c[0]) + 0.013, float(c[1]) + 0.011, float(c[2]) + 0.007], "size": [0.04, 0.2, 0.2],
                                   "velocity": [0.6, 0.0, 0.2], "start_time": 0.0, "end_time": 0.0015, "reset": 1})]
    o, t = oracle_from_scene(sc), TwinMPM(sc)
    seen_drag = seen_zero = False
    for k in range(45):   # 15 substeps in the window, 15 of zeroed grid, 15 free
        run_scene(o, sc, 1, k0=k); run_scene(t, sc, 1, k0=k)
        assert rel(o.x, t.x) < 1e-5, k
        assert np.abs(np.asarray(o.v, np.float64) - t.v).max() < 2e-4 * max(np.abs(t.v).max(), 0.1), k
        seen_drag |= 2 <= k < 14 and np.abs(t.v[:, 0]).max() > 0.5
        seen_zero |= 16 <= k < 29 and np.abs(t.v).max() == 0.0
    assert seen_drag and seen_zero and np.abs(t.v).max() > 0.0
