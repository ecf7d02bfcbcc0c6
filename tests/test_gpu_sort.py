"""The sort of the re-sort (csrc/resort.hip: k_rs_hist + k_rs_scatter, two launches a pass) on its own and inside the loop.

A re-sort orders the particles by class | state | block | cell with a STABLE sort of (key, index) pairs; the radix passes
written for it must produce the permutation a stable reference sort produces, for every size around the tile and slice
boundaries, for keys that are all equal, already sorted, reversed, and for the bit widths the solver uses.  Inside the loop:
with the library's sort instead (MPMHIP_SORT=rocprim) the same scene must come out the same after several re-sorts, up to the
run-to-run noise of the flush's floating-point atomics."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from mpmavatar_amd import harness, scenes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    sim = harness.build_solver(scenes.small_cube(), "cuda:0", mode="fast")
    yield sim.solver
    sim.solver.close()


def _sort(sv, keys, bits):
    k = torch.from_numpy(keys.view(np.int32).copy()).cuda()
    n = k.numel()
    ko = torch.empty_like(k)
    oo = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    sv._call("mpmhip_debug_sort", C.c_void_p(k.data_ptr() if n else 0), n, bits, C.c_void_p(ko.data_ptr() if n else 0),
             C.c_void_p(oo.data_ptr() if n else 0))
    return ko.cpu().numpy().view(np.uint32), oo.cpu().numpy()


def _check(sv, keys, bits):
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    ko, oo = _sort(sv, keys, bits)
    ref = np.argsort(keys, kind="stable").astype(np.int32)
    assert np.array_equal(oo, ref), f"n = {keys.size}, bits = {bits}: permutation differs from the stable reference sort"
    assert np.array_equal(ko, keys[ref])


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8191, 8193, 100_003])
def test_sizes_around_slice_and_tile_boundaries(solver, n):
    rng = np.random.default_rng(n)
    _check(solver, rng.integers(0, 1 << 30, n, dtype=np.uint32), 30)


@pytest.mark.parametrize("bits", [1, 7, 8, 9, 16, 17, 24, 30, 32])
def test_bit_widths(solver, bits):
    rng = np.random.default_rng(bits)
    hi = (1 << bits) - 1
    _check(solver, rng.integers(0, hi, 50_000, dtype=np.uint64, endpoint=True).astype(np.uint32), bits)


def test_few_distinct_keys_keep_their_input_order(solver):
    """Runs of equal keys far longer than a wavefront, a slice or a tile: stability is the whole result."""
    rng = np.random.default_rng(3)
    n = 300_000
    _check(solver, rng.integers(0, 5, n, dtype=np.uint32) << 20, 30)
    _check(solver, np.zeros(n, np.uint32), 30)
    _check(solver, np.full(n, (1 << 30) - 1, np.uint32), 30)


def test_sorted_reversed_and_nearly_sorted_input(solver):
    n = 200_001
    base = (np.arange(n, dtype=np.uint64) * 5000 % (1 << 30)).astype(np.uint32)
    s = np.sort(base)
    _check(solver, s, 30)
    _check(solver, s[::-1].copy(), 30)
    rng = np.random.default_rng(11)
    near = s.copy()
    idx = rng.integers(0, n, n // 50)
    near[idx] = rng.integers(0, 1 << 30, idx.size, dtype=np.uint32)   # what a re-sort sees: 2 % of the particles changed block
    _check(solver, near, 30)


def test_headline_size(solver):
    """497,762 keys shaped like the headline scene's (class | state | 18-bit block | 8-bit cell)."""
    rng = np.random.default_rng(5)
    n = 497_762
    cls = np.where(np.arange(n) < 331_298, 0, 2).astype(np.uint32)
    blk = rng.integers(0, 2704, n, dtype=np.uint32) * 37
    cell = rng.integers(0, 216, n, dtype=np.uint32)
    _check(solver, (cls << 28) | (blk << 8) | cell, 30)


def test_above_the_size_limit_the_library_sorts(solver):
    """More than 2^21 pairs go to rocPRIM (its Onesweep is built for that size): same contract."""
    rng = np.random.default_rng(21)
    _check(solver, rng.integers(0, 1 << 30, (1 << 21) + 5, dtype=np.uint32), 30)
    _check(solver, rng.integers(0, 1 << 30, 1 << 21, dtype=np.uint32), 30)   # the largest input of the own passes


def _run(sc_name, n_steps, sort):
    old = os.environ.get("MPMHIP_SORT")
    if sort:
        os.environ["MPMHIP_SORT"] = sort
    else:
        os.environ.pop("MPMHIP_SORT", None)
    try:
        sim = harness.build_solver(scenes.REGISTRY[sc_name](), "cuda:0", mode="fast", rebin_interval=-25)
    finally:
        if old is None:
            os.environ.pop("MPMHIP_SORT", None)
        else:
            os.environ["MPMHIP_SORT"] = old
    harness.run(sim, n_steps, fused=True)
    st = sim.solver.stats()
    out = {k: getattr(sim.state, k).cpu().numpy().copy() for k in ("particle_x", "particle_v", "particle_C", "particle_F_trial")}
    sim.solver.close()
    return out, st


def _dist(a, b, k):
    return float(np.abs(a[k].astype(np.float64) - b[k]).max()) / max(float(np.abs(b[k]).max()), 1e-3)


@pytest.mark.parametrize("scene", ["demo-mix", "garment-120k-aniso"])
def test_same_simulation_as_with_the_library_sort(scene):
    """A re-sort every 25 substeps (body faces included where the scene has a body).  Both sorts are stable sorts of the same
    keys, i.e. the same particle order; what differs between two runs is the order of the fp32 atomics of p2g's flush, and how
    far that noise grows depends on the scene (the anisotropic garment amplifies it).  So the yardstick is measured:
    the library-sort run against a repeat of itself."""
    a, sa = _run(scene, 130, None)
    b, sb = _run(scene, 130, "rocprim")
    b2, _ = _run(scene, 130, "rocprim")
    assert sa["rebins"] == sb["rebins"] and sa["rebins"] >= 5
    for k, floor in (("particle_x", 1e-6), ("particle_v", 1e-4), ("particle_C", 1e-3), ("particle_F_trial", 1e-5)):
        d, noise = _dist(a, b, k), _dist(b2, b, k)
        assert d <= 3.0 * noise + floor, (k, d, noise)
