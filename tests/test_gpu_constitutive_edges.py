"""The constitutive update on the device, through the real kernels, against float64 on the edge table.

The table, the float64 reference, the error norms and the margins are those of tests/constitutive_ref.py; the bound is the one
of tests/test_constitutive_edges.py, max(4 x the fp32 oracle's distance from float64 on the same family and field,
64 * 2^-24), with the oracle evaluated here on the same inputs.  What only the device has -- v_rcp_f32 / v_rsq_f32 in the
Jacobi rotations, hipcc's contraction, the wave-wide vote that ends the sweep loop of svd3 -- is what this module sees.

Mechanism (as tests/test_gpu_ref_golden.py): a scene with as many particles as the table has cases, on an interior lattice;
F_trial / d and the model arrays written into the state; one substep; F, stress, d, vertex_force and the model arrays read
back.  Each element owns three vertices, so that vertex_force holds f1, f2, f3 element by element.  The runs are gentle:
dt = 1e-6, E <= 100, no gravity, and a density of 1e6 -- the largest stress of the table then changes a velocity by ~1e-6 m/s,
and what g2p does to the state after the update under test ((I + dt grad v) on F_trial and on the director) stays below 1e-11
of it.  particle_d comes back with d1, d2 rebuilt from the vertices (they do not move: the table defines d1, d2 as those
differences) and the director as the return map left it.

Paths, every one of them on every traditional material and on cloth with and without friction:
  baseline           the stress kernel of the baseline back end
  fast               as shipped, first substep: stress at the head of k_p2g; k_stress_elem
  fast, profiled     stand-alone k_stress_trad; k_stress_elem with the stand-alone element finalize
  fast, 2nd substep  k_g2p2g (traditional-only scenes) / k_stress_elem with the fused finalize.  Its input is what the first
                     substep left, read from the one-substep run of the same back end: the float64 reference and the oracle
                     are evaluated on THAT state.  A first substep puts states ON two switches -- r22 := 1 for every stretched
                     element, ys ~ 0 for softened plasticine -- so this comparison alone is restricted to the cases whose
                     second-substep branch variables keep the table's margins (all of them but those two groups; the
                     restriction is asserted to be no larger than that), every case having been through the same device
                     functions in the three one-substep paths.  (Writing the table back into the state between the substeps
                     does not reach these kernels: a write makes the solver import the state again, which flushes the pending
                     g2p and finalizes the elements with the stand-alone kernel.  That k_g2p2g ran is counted by the solver;
                     the fused finalize has no counter: an unprofiled second substep of a cloth scene has no other path.)
  wave neighbours    baseline and fast once more with the families dealt out round-robin over the particle indices (and, for
                     traditional particles, over the lattice, which is what the fast back end sorts by): every wavefront then
                     mixes matrices that converge at once with slow ones.  Same bound, particle by particle.
After every run x, v, C and F_trial are finite.
"""
import time

import numpy as np
import pytest
import torch

import constitutive_ref as cr
from test_constitutive_edges import CLOTHS, MATERIALS, oracle_cloth, oracle_trad, report

pytestmark = pytest.mark.gpu
DENSITY = 1e6
N_GRID = 32
_T = {"total": 0.0}


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    yield
    print(f"\ntest_gpu_constitutive_edges: {_T['total']:.1f} s of wall time in its tests")


def _np(t):
    return t.detach().cpu().numpy().copy()


def _put(dst, a):
    dst.copy_(torch.as_tensor(np.ascontiguousarray(a, np.float32), device=dst.device).reshape(dst.shape))


def _finite(sim, what):
    for f in ("particle_x", "particle_v", "particle_C", "particle_F_trial"):
        assert np.isfinite(_np(getattr(sim.state, f))).all(), (what, f)


# ------------------------------------------------------------------------------------------------ traditional particles
def _run_trad(material, tab, mode, steps=1, profiled=False, order=None):
    """One (or two) substeps of a scene that holds the table, case order[k] in slot k; results in table order."""
    from mpmavatar_amd import harness, scenes
    n = tab["F_trial"].shape[0]
    order = np.arange(n) if order is None else order
    params = {"material": material, "g": [0.0, 0.0, 0.0], "density": DENSITY, "hardening": tab["hardening"], "xi": tab["xi"],
              "plastic_viscosity": tab["plastic_viscosity"], "softening": tab["softening"]}
    if material == "sand":
        params["friction_angle"] = cr.TRAD_PARAMS["friction_angle"]
    sc = scenes._trad_scene(f"edge-{material}", cr.lattice(n), 0.02 ** 3, N_GRID, material=material, params=params,
                            bcs=[("bounding_box", {})], E=100.0)
    sc.density, sc.dt = DENSITY, tab["dt"]
    sim = harness.build_solver(sc, "cuda:0", mode=mode)
    assert material != "sand" or abs(float(sim.model.alpha) - tab["alpha"]) <= 1e-7
    if profiled:
        sim.solver.enable_profiling(True)
    _put(sim.state.particle_F_trial, tab["F_trial"][order])
    for f, k in (("mu", "mu"), ("lam", "lam"), ("yield_stress", "ys")):
        _put(getattr(sim.model, f), tab[k][order])
    harness.run(sim, steps, fused=steps > 1)
    if mode == "fast" and not profiled:
        assert sim.solver.stats().get("g2p2g_launches", 0) == steps - 1     # the second update ran inside k_g2p2g
    if profiled:      # the stand-alone stress kernel has a phase of its own only when the update does not ride in k_p2g
        assert len(sim.solver.time_profile.get("compute_stress_from_F_trial", [])) == steps
    back = np.empty(n, np.int64)
    back[order] = np.arange(n)
    out = {"F": _np(sim.state.particle_F)[back], "stress": _np(sim.state.particle_stress)[back], "mu": _np(sim.model.mu)[back],
           "lam": _np(sim.model.lam)[back], "ys": _np(sim.model.yield_stress)[back]}
    _finite(sim, (material, mode, steps, profiled))
    return out


@pytest.mark.parametrize("material", MATERIALS)
def test_traditional_update_on_the_device(material, oracle_lib):
    t0 = time.time()
    tab = cr.trad_table(material)
    info0 = {}
    want, scales = cr.trad_reference(tab, info=info0), cr.trad_scales(tab)
    mix = cr.interleave(tab["family"])
    runs = {"oracle": oracle_trad(tab),
            "baseline": _run_trad(material, tab, "baseline"),
            "fast": _run_trad(material, tab, "fast"),
            "fast profiled": _run_trad(material, tab, "fast", profiled=True),
            "baseline mixed": _run_trad(material, tab, "baseline", order=mix),
            "fast mixed": _run_trad(material, tab, "fast", order=mix)}
    bad = report(f"{material} (device)", tab, want, scales, runs, cr.conditioning(tab, info0, scales))

    # second substep: the update inside k_g2p2g, on the state the first substep left
    first = runs["fast"]
    info = {}
    want2 = cr.trad_reference(tab, F_trial=first["F"], mu=first["mu"], lam=first["lam"], ys=first["ys"], info=info)
    keep = np.ones(len(tab["family"]), bool)
    if material == "plasticine":
        keep = ~(np.abs(info["softened"]) < cr.MARGIN_SOFTEN)        # (NaN: does not yield again)
        again = np.isfinite(info["softened"])
        print(f"  second substep: {int(again.sum())} cases yield again, {int((~keep).sum())} of them within the margin of ys = 0")
        assert (~keep).sum() <= 0.05 * len(keep)
    sub = {k: (v[keep] if isinstance(v, np.ndarray) and len(v) == len(keep) else v) for k, v in tab.items()}
    cut = lambda d: {k: v[keep] for k, v in d.items()}
    scales2 = cr.trad_scales(tab, F_trial=first["F"])
    runs2 = {"oracle": cut(oracle_trad(tab, F_trial=first["F"], mu=first["mu"], lam=first["lam"], ys=first["ys"])),
             "fast, 2nd substep": cut(_run_trad(material, tab, "fast", steps=2))}
    bad += report(f"{material} (device, second substep)", sub, cut(want2), cut(scales2), runs2, cut(cr.conditioning(tab, info, scales2)))
    _T["total"] += time.time() - t0
    print(f"  [{material}: {time.time() - t0:.1f} s]")
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ cloth elements
def _run_cloth(tab, mode, steps=1, profiled=False, order=None):
    from mpmavatar_amd import harness, scenes
    n = tab["d"].shape[0]
    order = np.arange(n) if order is None else order
    verts = tab["verts"][order]
    x = np.concatenate([verts.mean(1), verts.reshape(-1, 3)], 0).astype(np.float32)
    vol = np.concatenate([tab["vol"][order], np.repeat(tab["vol"][order], 3)]).astype(np.float32)
    fc0 = tab["friction_coeff"] == 0.0
    sc = scenes.Scene(name="edge-cloth", n_grid=N_GRID, grid_lim=2.0, n_elements=n, n_traditional=0, n_vertices=3 * n, x=x,
                      v=np.zeros_like(x), vol=vol, faces=np.arange(3 * n, dtype=np.int32).reshape(n, 3),
                      d=tab["d"][order], R_inv=tab["R_inv"][order], density=DENSITY, dt=1e-6,
                      bcs=[("bounding_box", {})],
                      params={"material": "cloth", "g": [0.0, 0.0, 0.0], "density": DENSITY,
                              "friction_angle": 0.0 if fc0 else cr.TRAD_PARAMS["friction_angle"]})
    sim = harness.build_solver(sc, "cuda:0", mode=mode)
    assert abs(float(sim.model.friction_coeff) - tab["friction_coeff"]) <= 1e-7
    if profiled:
        sim.solver.enable_profiling(True)
    for k in ("mu", "lam", "gamma", "kappa"):
        full = _np(getattr(sim.model, k))
        full[:n] = tab[k][order]
        _put(getattr(sim.model, k), full)
    harness.run(sim, steps, fused=steps > 1)
    if profiled:      # stress and the element finalize as launches of their own
        assert len(sim.solver.time_profile.get("compute_stress_from_F_trial", [])) == steps
        assert len(sim.solver.time_profile.get("g2p_e", [])) == steps
    back = np.empty(n, np.int64)
    back[order] = np.arange(n)
    vf = _np(sim.state.vertex_force).reshape(n, 3, 3)[back]
    out = {"d": _np(sim.state.particle_d)[back], "stress": _np(sim.state.particle_stress)[:n][back],
           "f1": vf[:, 0], "f2": vf[:, 1], "f3": vf[:, 2]}
    _finite(sim, ("cloth", mode, steps, profiled))
    return out


@pytest.mark.parametrize("which", list(CLOTHS))
def test_element_update_on_the_device(which, oracle_lib):
    t0 = time.time()
    tab = cr.cloth_table(friction_coeff=CLOTHS[which])
    info0 = {}
    want, scales = cr.cloth_reference(tab, info=info0), cr.cloth_scales(tab)
    mix = cr.interleave(tab["family"])
    runs = {"oracle": oracle_cloth(tab),
            "baseline": _run_cloth(tab, "baseline"),
            "fast": _run_cloth(tab, "fast"),
            "fast profiled": _run_cloth(tab, "fast", profiled=True),
            "baseline mixed": _run_cloth(tab, "baseline", order=mix),
            "fast mixed": _run_cloth(tab, "fast", order=mix)}
    for lab, got in runs.items():      # d1, d2 come back as the vertex differences the table defines them to be
        if lab != "oracle":
            assert np.array_equal(got["d"][:, :, :2], tab["d"][:, :, :2]), lab
    bad = report(f"{which} (device)", tab, want, scales, runs, cr.conditioning(tab, info0, scales))

    # second substep: k_stress_elem with the fused finalize, on the directors the first substep left
    d1 = runs["fast"]["d"]
    info = {}
    want2 = cr.cloth_reference(tab, d=d1, info=info)
    keep = np.abs(info["r22"] - 1.0) >= cr.MARGIN_R22
    fr = info["fric"]
    keep &= ~(np.isfinite(fr) & (np.abs(fr) < cr.MARGIN_FRIC))
    info1 = {}
    cr.cloth_reference(tab, info=info1)
    on_switch = info1["over"] | info1["slide"] | (tab["family"] == tab["names"].index("flat_exact"))
    print(f"  second substep: {int(keep.sum())} of {len(keep)} cases keep the margins; {int(on_switch.sum())} were mapped onto a switch")
    assert not (~keep & ~on_switch).any() and keep.sum() >= 0.25 * len(keep)
    sub = {k: (v[keep] if isinstance(v, np.ndarray) and len(v) == len(keep) else v) for k, v in tab.items()}
    cut = lambda dd: {k: v[keep] for k, v in dd.items()}
    runs2 = {"oracle": cut(oracle_cloth(tab, d=d1)), "fast, 2nd substep": cut(_run_cloth(tab, "fast", steps=2))}
    scales2 = cr.cloth_scales(tab, d=d1)
    bad += report(f"{which} (device, second substep)", sub, cut(want2), cut(scales2), runs2, cut(cr.conditioning(tab, info, scales2)))
    _T["total"] += time.time() - t0
    print(f"  [{which}: {time.time() - t0:.1f} s]")
    assert not bad, "\n".join(bad)
