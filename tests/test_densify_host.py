"""Densification without a GPU: the twin (tests/densify_twin_torch.py) pinned against the reference's own densify_and_prune,
add_densification_stats and reset_opacity run on a stand-in model with a real Adam (tests/golden/densify.npz); the measurement of
S32, the constant the bound is built on; mpmavatar_amd/csrc/densify_math.hpp compiled with g++ (tests/hostdensify/hostdensify.cpp:
serial loops that mirror the kernels) against the float64 twin -- src, kind, binding, binding_counter, the counts, copied rows and
moments exactly, computed values within BOUND; the situations the cases are named for, as the results show them; and the same file
as a stand-alone program under AddressSanitizer and UBSan.  The conditions of the comparison (margins, situations) are asserted by
the case builder itself.  Every comparison prints its figures before it asserts (run with -s)."""
import os
import subprocess

import numpy as np
import pytest
import torch

import densify_cases as dc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "densify.npz")
FIXTURE_KEYS = dc.PARAMS + tuple(p + k for p in ("m_", "v_") for k in dc.PARAMS) + ("binding", "binding_counter", "add_accum", "add_denom",
                                                                                  "add_max_radii", "reset")


@pytest.mark.parametrize("name", dc.CASES)
def test_twin_reproduces_the_reference(name):
    """integer outputs and copied rows bit for bit; child xyz / _scaling, the statistics and the reset opacities to 1e-13"""
    g = np.load(GOLD)
    assert os.path.getsize(GOLD) < 200 * 1024
    t = dc.twin64(name)
    new = t["kind"] == 2
    for k in FIXTURE_KEYS:
        ref, mine = g[f"{name}_{k}"], t[k]
        assert ref.shape == mine.shape, (name, k, ref.shape, mine.shape)
        if k in dc.NUMERIC:
            err = dc.rel(mine, ref)
            print(name, k, "twin against the fixture %.3g" % err)
            assert ref.dtype == np.float64 and err < 1e-13, (name, k)
            if k in dc.COMPUTED:
                assert np.array_equal(mine[~new], ref[~new]), (name, k)
        else:
            assert np.array_equal(mine, ref.astype(mine.dtype)), (name, k)
    # src and kind are ours: every output row is its source's row, which pins them to the reference's rows
    c = dc.case(name)
    for k in ("_rotation", "_opacity", "_features_dc"):
        assert np.array_equal(g[f"{name}_{k}"], c[k][t["src"]]), (name, k)
    kept = t["kind"] == 0
    assert np.array_equal(g[f"{name}_m__xyz"][kept], c["m__xyz"][t["src"][kept]]) and not g[f"{name}_m__xyz"][~kept].any()


def test_s32_is_the_measurement():
    worst = 0.0
    for name in dc.CASES:
        t32, t64 = dc.twin(dc.case(name), torch.float32), dc.twin64(name)
        assert all(np.array_equal(t32[k], t64[k]) for k in ("src", "kind", "binding", "binding_counter", "counts")), name
        errs = {k: dc.rel(t32[k], t64[k]) for k in dc.NUMERIC}
        print(name, ", ".join("%s %.3g" % kv for kv in errs.items()))
        worst = max(worst, max(errs.values()))
    print("S32 measured %.4g, committed %.4g" % (worst, dc.S32))
    assert 0.5 * dc.S32 < worst <= dc.S32
    assert dc.BOUND == 10 * dc.S32


@pytest.mark.parametrize("name", dc.CASES)
def test_cases_hold_what_they_are_named_for(name):
    """as the float64 twin's RESULT shows it (the builder asserts the inputs)"""
    c, t = dc.case(name), dc.twin64(name)
    n = c["binding"].shape[0]
    n_out, n_cloned, n_split, n_pruned = t["counts"]
    assert n_out == n + n_cloned + n_split - n_pruned == t["src"].shape[0]
    assert np.array_equal(t["binding_counter"], np.bincount(t["binding"], minlength=c["n_faces"]))
    assert (t["binding_counter"][np.bincount(c["binding"], minlength=c["n_faces"]) > 0] >= 1).all()       # no face lost its last Gaussian
    blocks = np.flatnonzero(np.diff(t["kind"]))                                                           # kept, clones, children: in that order
    assert (np.diff(t["kind"]) >= 0).all() and len(blocks) <= 2
    if name == "main":
        d = dc.decisions(c)
        assert n_cloned == d["clone"].sum() and n_split == d["split"].sum() and n_pruned > 50
        assert t["binding_counter"][0] == 1 and t["src"][0] == 0                # the flagged single Gaussian stayed
        on1 = t["binding"] == 1                                                  # the all-flagged face: 2 kept, 1 clone, 2 children, none removed
        assert sorted(t["kind"][on1]) == [0, 0, 1, 2, 2] and t["binding_counter"][1] == 5
        removed_faint = d["faint"] & ~d["split"] & ~np.isin(np.arange(n), t["src"][t["kind"] == 0])
        assert removed_faint.sum() > 20                                          # elsewhere the same flag does remove rows
        children = t["src"][t["kind"] == 2]
        assert np.array_equal(children[: len(children) // 2], children[len(children) // 2:]) and (np.diff(children[: len(children) // 2]) > 0).all()
        assert {14, 15} <= set(t["src"][t["kind"] != 0])                         # g == max_grad is selected
    if name == "none":
        assert n_out == n and np.array_equal(t["src"], np.arange(n)) and not t["kind"].any()
        for k in dc.PARAMS:
            assert np.array_equal(t[k], c[k].astype(np.float64)) and np.array_equal(t["m_" + k], c["m_" + k].astype(np.float64))
    if name == "all_split":
        assert (t["kind"] == 2).all() and n_out == 2 * n and np.array_equal(t["src"], np.tile(np.arange(n), 2))
    if name == "empty":
        assert n_out == 0 and t["_features_rest"].shape == (0, 3, 3) and not t["binding_counter"].any()
    if name == "tiny":
        assert t["_features_rest"].shape == (n_out, 0, 3)


@pytest.mark.parametrize("name", dc.CASES)
@pytest.mark.parametrize("mask", (False, True), ids=("radii", "mask"))
def test_host_against_float64(name, mask):
    got = dc.host(dc.case(name), mask=mask)
    assert all(v.dtype in (np.float32, np.int32) for v in got.values())
    dc.compare(got, dc.twin64(name, mask), dc.BOUND, name)


def test_host_leaves_rows_outside_the_update_alone():
    c = dc.case("main")
    got = dc.host(c)
    hidden = c["radii"] == 0
    assert hidden.sum() > 100
    for k in ("add_accum", "add_denom", "add_max_radii"):
        assert np.array_equal(got[k][hidden], c[k][hidden]), k
    assert (got["add_denom"][~hidden] == c["add_denom"][~hidden] + 1).all()
    assert (got["reset"] <= np.float32(np.log(0.01 / 0.99)) + 1e-6).all()


def test_stand_alone_program_under_sanitizers():
    """every loop on exactly sized arrays, with and without zero-width rows and with n = 0, as a stand-alone program built with
    -fsanitize=address,undefined: an index past a row or a table ends it with a report"""
    r = subprocess.run([dc.sanitizer_program()], capture_output=True, text=True, timeout=120)
    print(r.stdout.strip(), r.stderr.strip()[:2000])
    assert r.returncode == 0 and r.stdout.startswith("ok: 301 Gaussians on 17 faces"), (r.returncode, r.stderr[-2000:])
