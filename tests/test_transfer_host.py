"""The cases of tests/transfer_cases.py on the host: their preconditions, the float64 twin against itself, and the yardstick.

Nothing here runs the code under test.  What it establishes is what tests/test_gpu_transfer_edges.py relies on:

* exact family -- every p2g contribution is an integer multiple of the coarsest unit the packed fixed-point chunk tile can
  choose (2^-k, k the largest integer with 1.001 B 2^k < 2^30, B summed over ALL particles of the case: p2g_device.hpp,
  fx_bounds / fx_scales / fx_pow2), every position sits on fx in {0.5, 1.0}, the stress is bitwise zero, and the fp32 oracle's
  grid mass and momentum equal the twin's bit for bit after the cast -- with C, on every sub-case;
* general family -- the run offsets of `runs` (segments that end on lanes 15 / 16 / 17 and 63 / 64 / 65, runs longer than a
  16-lane row, one that straddles the 256-particle chunk), the share of moved particles of `moved` / `escaped` (with the oracle
  standing in for the device's own pre-steps), the branch margins and the force share of `sheet`, and the yardstick table:
  the oracle's distance from the twin per case and field, none above 1e-5 but C of `galilean` (the reference's own
  formulation of C cancels there);
* the twin -- sum of grid_m = sum of particle mass, sum of node momentum = sum of m v (+ dt sum of forces, which is zero in
  exact arithmetic), both to 1e-13.
"""
import numpy as np
import pytest

import constitutive_ref as cr
import transfer_cases as tc

EXACT = tc.exact_cases()
GENERAL = tc.general_cases()


@pytest.fixture(scope="module")
def refs(oracle_lib):
    """{case name: (state compared from, twin fields, oracle fields)} -- computed once."""
    out = {}
    for case in EXACT + GENERAL:
        st = tc.oracle_state(case, case.pre_steps) if case.pre_steps else case.state
        out[case.name] = (st, tc.twin(case, st), tc.oracle(case, st))
    return out


@pytest.mark.parametrize("case", EXACT, ids=lambda c: c.name)
def test_exact_family_preconditions_and_oracle_bitwise(case, refs):
    sc, st = case.scene, case.state
    xg = st["x"].astype(np.float64) / tc.DX
    fx = xg - np.trunc(xg - 0.5)
    assert np.isin(fx, (0.5, 1.0)).all()
    assert (fx == 0.5).any() and (fx == 1.0).any() or case.name == "e-one"     # the tie (cell boundary) is among them
    assert (xg >= 2.0).all() and (xg <= sc.n_grid - 2.0).all()                 # inside the position clamp
    v, C = st["v"].astype(np.float64), st["C"].astype(np.float64)
    assert (v == np.round(v)).all() and np.abs(v).max() <= 8
    assert (C / 16.0 == np.round(C / 16.0)).all() and np.abs(C).max() <= 64
    assert (sc.vol == np.float32(2.0 ** -12)).all() and sc.density == 1.0 and sc.E == 0.0 and not sc.bcs
    assert np.float32(sc.dt) == np.float32(2.0 ** -13) and not np.any(sc.params["g"])
    nodes, wm, add, ref = tc.p2g_contributions(case)
    aux = ref["_aux"]
    assert not aux["stress"].any()                                              # stress bitwise zero
    um, up = tc.fx_unit(aux["bm"].sum()), tc.fx_unit(aux["bp"].sum())
    assert (wm / um == np.round(wm / um)).all() and (add / up == np.round(add / up)).all()
    print(f"\n{case.name}: {len(v)} particles, units 2^{int(np.log2(um))} (mass), 2^{int(np.log2(up))} (momentum); largest node sums "
          f"{ref['grid_m'].max() / um:.0f}, {np.abs(ref['grid_p']).max() / up:.0f} units")
    assert ref["grid_m"].max() / um < 2.0 ** 30 and np.abs(ref["grid_p"]).max() / up < 2.0 ** 30
    # exact in fp32: the twin's sums survive the cast, and the oracle's fp32 sums are those
    _, t, o = refs[case.name]
    for k in ("grid_m", "grid_p"):
        assert np.array_equal(t[k].astype(np.float32).astype(np.float64), t[k]), k
        assert np.array_equal(o[k], t[k]), (case.name, k)
    mir = case.notes.get("mirror")
    if mir:
        p, has_m = t["grid_p"], t["grid_m"] > 0
        zero = {"y": [2], "x": [2], "z": [1], "all": [0, 1, 2]}[mir]
        neg = {"y": [1], "x": [0, 1], "z": [2], "all": []}[mir]
        assert has_m.sum() >= 64
        for a in zero:
            assert (p[:, a] == 0.0).all()
        for a in neg:
            assert (p[has_m, a] < 0.0).all()
    if case.name == "e-corner8":
        blocks = {tuple(b) for b in (np.trunc(xg - 0.5).astype(int) >> 2)}
        assert len(blocks) == 8
    if case.name == "e-face":
        b = np.trunc(xg - 0.5).astype(int) >> 2
        assert {tuple(r) for r in b} == {(0, 0, 0), (7, 7, 7)}
    if case.name.split("-")[1].isdigit():                                      # e-N: one block, whatever the predictive sort does
        cell = np.trunc(xg - 0.5).astype(int) - 4 * np.asarray(tc.BLOCK)
        assert ((cell >= 1) & (cell <= 2)).all()


@pytest.mark.parametrize("case", EXACT + GENERAL, ids=lambda c: c.name)
def test_twin_conserves_mass_and_momentum(case, refs):
    st, t, _ = refs[case.name]
    aux = t["_aux"]
    m_tot, p_tot = aux["mass"].sum(), aux["mv"].sum(0)
    assert abs(t["grid_m"].sum() - m_tot) <= 1e-13 * m_tot
    scale = np.abs(aux["mv"]).sum()
    # (p2g adds dt * force on top of m v; the stress terms and an element's three corner forces each sum to zero)
    assert np.abs(t["grid_p"].sum(0) - p_tot).max() <= 1e-13 * scale, np.abs(t["grid_p"].sum(0) - p_tot).max() / scale


def test_runs_hit_the_row_and_wave_boundaries():
    case = next(c for c in GENERAL if c.name == "runs")
    xg = case.state["x"].astype(np.float64) / tc.DX
    cell = np.trunc(xg - 0.5).astype(int) - 4 * np.asarray(tc.BLOCK)
    assert ((cell >= 0) & (cell <= 3)).all()                                   # one block
    frac = xg - 0.5 - np.trunc(xg - 0.5)
    # the look-ahead of the predictive sort (12 substeps at first) does not reach a cell face: block and order are those of x
    assert (np.minimum(frac, 1.0 - frac) * tc.DX > 12 * case.scene.dt * np.abs(case.state["v"])).all()
    ends, lengths = tc.run_offsets(xg)
    assert tuple(lengths) == tc.RUN_LENGTHS
    lane = set(int(e) for e in ends)
    print(f"\nruns: segments end at offsets {sorted(lane)}")
    assert {15, 16, 17, 63, 64, 65} <= lane
    assert max(lengths[:17]) > 16 and any(s < 256 < e for s, e in zip(np.r_[0, ends[:-1]], ends))   # longer than a row; across two chunks
    assert {1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 33} <= set(int(n) for n in lengths)


@pytest.mark.parametrize("name", ["moved", "escaped"])
def test_moved_cases_move(name, refs):
    case = next(c for c in GENERAL if c.name == name)
    st, _, _ = refs[name]
    c0 = np.trunc(case.state["x"].astype(np.float64) / tc.DX - 0.5).astype(int)
    c1 = np.trunc(st["x"].astype(np.float64) / tc.DX - 0.5).astype(int)
    share = (c0 != c1).any(1).mean()
    step = np.linalg.norm(case.scene.dt * case.state["v"].astype(np.float64), axis=1) / tc.DX
    print(f"\n{name}: {share:.2f} of the particles in another cell after {case.pre_steps} substeps; first step {step.mean():.2f} cell (max {step.max():.2f})")
    assert share >= 0.3
    if name == "escaped":
        rel_cell = c1 - (4 * np.asarray(tc.BLOCK) - 1)      # position in the tile of BLOCK: 0..5 is inside its margin
        assert ((rel_cell < 0) | (rel_cell > 5)).any(1).sum() >= 10
    # (`moved`: the device test asserts n_fallback_particles == 0 itself, the block a particle was sorted into being the predicted one)


@pytest.mark.parametrize("case", [c for c in GENERAL if c.notes.get("sheet")], ids=lambda c: c.name)
def test_sheet_keeps_margins_and_carries_force(case, refs):
    sc = case.scene
    assert sc.n_elements == 72 and sc.n_vertices == 49
    info = {}
    fc = cr.friction_coeff_of(sc.params["friction_angle"])
    cr.cloth_return_map(case.state["d"].astype(np.float64), sc.gamma, sc.kappa, fc, info)
    assert (np.abs(info["r22"] - 1.0) >= cr.MARGIN_R22).all()
    fr = info["fric"]
    assert not (np.isfinite(fr) & (np.abs(fr) < cr.MARGIN_FRIC)).any()
    _, t, _ = refs[case.name]
    aux = t["_aux"]
    nnv = sc.n_elements
    share = aux["dt"] * np.abs(aux["vertex_force"]).max() / np.abs(aux["mv"][nnv:]).max()
    print(f"\n{case.name}: r22 {info['r22'].min():.3f}..{info['r22'].max():.3f}, {int(info['over'].sum())} over, {int(info['slide'].sum())} sliding; "
          f"dt max|vertex_force| / max|m v| = {share:.2f}")
    assert share >= 0.1


def test_yardstick_table(refs):
    """The oracle's distance from the twin, per case and field: what the device's bounds are multiples of."""
    bad = []
    print("\n== oracle against the float64 twin, max|a - b| / max|b| ==")
    for case in GENERAL:
        _, t, o = refs[case.name]
        d = tc.distance(o, t, case.fields)
        print(f"  {case.name:16s} " + "  ".join(f"{k} {v:.1e}" for k, v in d.items()))
        for k, v in d.items():
            if not v <= tc.YARDSTICK_CEILING and not (case.name == "galilean" and k == "C"):
                bad.append(f"{case.name} {k}: {v:.2e}")
    assert not bad, bad


@pytest.mark.parametrize("case", [c for c in GENERAL if c.name in ("plain", "range", "sheet-d0.9-gk500")], ids=lambda c: c.name)
def test_fixed_tile_allowance_is_finite_and_positive(case, refs):
    st, t, _ = refs[case.name]
    allow = tc.fixed_tile_allowance(case, t, st)
    print(f"\n{case.name}: allowance of the fixed-point tile " + "  ".join(f"{k} {v:.1e}" for k, v in allow.items()))
    assert set(allow) == set(case.fields) and all(np.isfinite(v) and v > 0 for v in allow.values())
