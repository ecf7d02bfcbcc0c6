"""The capacity-retry loop of the re-sort (csrc/resort.hip rebin): the block tables are built with the capacities the last
re-sort suggested, and a re-sort that finds more particle blocks than that grows the tables and builds them again.

The first re-sort of a scene starts from min(blocks, max(1024, n_p / 16)) particle blocks.  A scene of one particle per block
in about 2,000 of the 4,096 blocks of a 64^3 grid is past that at once: the first attempt overflows, the second must leave the
same tables a big enough first attempt would have left."""
import numpy as np
import pytest

from mpmavatar_amd import harness
from mpmavatar_amd.scenes import _trad_scene

pytestmark = pytest.mark.gpu

N_GRID, NB, N_P = 64, 16, 2000


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-3))


def _scene():
    """One particle at rest in each of N_P blocks, drawn from the blocks 0..14 per axis (the last layer lies past the position
    clamp of g2p, 2 dx from the faces).  A block's particles are those whose base cell floor(x / dx - 0.5) is one of its four per
    axis; x / dx = 4 b + 2.5 puts the base cell on 4 b + 2 exactly (dx = 2^-5: no rounding), a cell and a half from either face."""
    rng = np.random.default_rng(5)
    cand = np.stack(np.meshgrid(*[np.arange(NB - 1)] * 3, indexing="ij"), -1).reshape(-1, 3)
    blk = cand[rng.permutation(len(cand))[:N_P]]
    dx = 2.0 / N_GRID
    pts = ((4 * blk + 2.5) * dx).astype(np.float32)
    return _trad_scene("one-per-block", pts, (dx / 2) ** 3, N_GRID, E=100.0, bcs=[("bounding_box", {})], n_steps=4), blk


def test_first_resort_grows_the_tables_and_builds_them_again():
    sc, blk = _scene()
    n_particle_blocks = len(np.unique((blk[:, 0] * NB + blk[:, 1]) * NB + blk[:, 2]))
    initial_capacity = min(NB ** 3, max(1024, sc.n_particles // 16))
    assert n_particle_blocks > initial_capacity, "the scene does not overflow the first attempt's tables"
    occupied = np.zeros((NB + 2,) * 3, bool)
    occupied[blk[:, 0] + 1, blk[:, 1] + 1, blk[:, 2] + 1] = True
    active = np.zeros((NB,) * 3, bool)
    for ox in range(3):   # the 27 neighbours, clipped to the grid by the padding layer
        for oy in range(3):
            for oz in range(3):
                active |= occupied[2 - ox:2 - ox + NB, 2 - oy:2 - oy + NB, 2 - oz:2 - oz + NB]
    fast = harness.build_solver(sc, "cuda:0", mode="fast")
    harness.run(fast, 1, fused=True)
    st = fast.solver.stats()
    print("particle blocks", n_particle_blocks, "initial capacity", initial_capacity, "active blocks", int(active.sum()), "stats", st)
    assert st["rebins"] == 1
    assert st["n_active_blocks"] == int(active.sum())
    harness.run(fast, 3, fused=True)
    base = harness.build_solver(sc, "cuda:0", mode="baseline")
    harness.run(base, 4, fused=True)
    xf, vf = fast.state.particle_x.cpu().numpy(), fast.state.particle_v.cpu().numpy()
    xb, vb = base.state.particle_x.cpu().numpy(), base.state.particle_v.cpu().numpy()
    print("fast against baseline after 4 substeps: rel x", rel(xf, xb), "rel v", rel(vf, vb))
    assert np.isfinite(xf).all() and np.isfinite(vf).all()
    # (the bounds of tests/test_gpu_parity.py test_cube_materials, a scene of traditional particles only)
    assert rel(xf, xb) < 1e-4
    assert rel(vf, vb) < 1e-4
