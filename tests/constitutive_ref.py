"""float64 restatement of the per-particle constitutive update, and the edge table it is tested on (TEST INFRASTRUCTURE ONLY).

Two parts.

1.  ``trad_update`` / ``cloth_update``: pure NumPy float64 functions on arrays, written from the reference's
    warp_mpm/mpm_utils.py (line numbers at each function) the way oracle/twin.py is: convention-free -- LAPACK SVD made
    proper (det U = det V = +1, the sign of det F in the last singular value; for det F > 0 nothing depends on that choice),
    closed-form QR with R00, R11 >= 0 and det Q = +1, closed-form 2x2 polar rotation.  They do not take a scene.  The twin
    (oracle/twin.py) delegates its constitutive methods to them; tests/golden/ref_edge_constitutive.npz, produced by the
    reference's own unchanged ``compute_stress_from_F_trial``, pins them (tests/test_constitutive_edges.py).

2.  ``trad_table`` / ``cloth_table``: the seeded edge table.  The host tests, the GPU tests and the fixture generator all
    build their inputs with these two functions and nothing else.

    Traditional particles, F_trial = U diag(s) V^T with random proper rotations unless said otherwise:
      sv_range         s log-uniform in [0.005, 5]: the domain on which ``svd3`` of mpm_math.hpp is sound (a probe of the
                       contraction-free host build: reconstruction, orthogonality and singular values within 8.2e-7 for
                       identity, rotations, reflections, equal singular values, rank 2 / 1 / 0, condition up to 1e6; it
                       breaks at overall scale 1e-12 through its 1e-10 rank threshold and at 1e12 where app * aqq
                       overflows -- neither is a physical state)
      identity, rotation, two_equal_large (a, a, b), two_equal_small (a, b, b), three_equal (a, a, a),
      near_equal_1e-5  (singular values equal to within 1e-5), compression (0.3 .. 0.9, nearly uniform),
      stretch (1.1 .. 3 along one axis), cond_1e2, cond_1e4, below_clamp_1 / _2 / _3 (that many singular values under the
      0.01 clamp of the StVK stress and the von Mises / viscoplastic maps), diagonal (no rotations), signed_perm (signed
      permutation matrices of determinant +1), inverted (jelly only: det F < 0).
    Thresholds, per material -- placed through the per-particle yield stress (metal, foam, plasticine) or through the
    volumetric strain (sand), from the float64 branch variable of the fp32-rounded input:
      yield_in_<r>, yield_out_<r>, yield_on      relative distance r = 1e-1, 1e-3, 1e-5 under / over the yield function and on
                       it (metal, plasticine: |dev tau| against ys; foam: |s_trial| against sqrt(2/3) ys; sand: delta_gamma
                       against 0, as delta_gamma / |dev eps|).  Every return map is continuous there: nothing is excused.
      tr_neg_<d>, tr_pos_<d>   sand with delta_gamma > 0 and tr eps = -+d, d = 1e-1 .. 1e-4: the switch to F = U V^T
      soften_live_<r>, soften_dead_<r>   plasticine whose softened yield stress ends at +-r of the old one, r = 1e-1 .. 1e-3:
                       the switch to mu = lam = 0
      ys_zero, ys_negative   plasticine that arrives with ys <= 0 (the input itself decides: no rounding is involved)
      rest_ys_negative       metal at rest (identity and signed permutations: log strain exactly 0 in every precision) with a
                       negative yield stress: |dev tau| = 0 > ys takes the plastic branch with dev eps = 0, the 0 / 0 that the
                       reference's "+ 1e-6" on |dev eps| (mpm_utils.py:234) exists for.  Only exact rest states: with a
                       rounding-level dev eps the reference's own (delta_gamma / |dev eps|) dev eps amplifies that rounding
                       by |ys| / (2 mu 1e-6), in any fp32 evaluation.

    Cloth elements (d1, d2 are differences of fp32 vertex positions, so that a solver which rebuilds them from its vertices
    sees the same numbers):
      flat_exact       rest states whose QR is exact in fp32 and in float64 (r22 == 1 bit for bit): axis-aligned, and turned by
                       signed permutations, with and without shear of the director.  THE exception to the r22 margin below.
      general, r22_over_<d>, r22_under_<d> (d = 1e-4 .. 0.5), fric_in_<r>, fric_out_<r> (shear force at 1 -+ r of the friction
      threshold, same ladder), gamma0, aspect (triangles up to 1:100), folded (det d < 0).
      ``cloth_table(friction_coeff=0.0)`` is the same table with the model's friction coefficient at zero.

    MARGINS (asserted on the table itself by tests/test_constitutive_edges.py::test_table_keeps_its_margins): the float64
    branch variables of every case stay away from the four real switches by
        |r22 - 1|                    >= 5e-5     (flat_exact excepted: r22 == 1 exactly in both precisions)
        |ff / (fc fn) - 1|           >= 5e-5     (where the friction branch is reached and fc fn > 0)
        |tr eps| (sand, dg > 0)      >= 5e-5     (excepted: states at rest, |eps| <= 1e-6, where all three branches of the
                                                 sand map return F_trial to that rounding: identity, rotation, signed_perm)
        |ys_softened| / ys           >= 5e-4     (plasticine that yields)
    i.e. half the smallest rung of each ladder (1e-4, 1e-4, 1e-4, 1e-3): a rung is placed in float64 and the rounding of the
    input to fp32 moves it by ~1e-6 of itself.  No rung of the issue's ladders was dropped: fp32 resolves r22 to ~2e-7 and tr eps to ~3e-7, two orders under the
    smallest rung; the softening switch was given its own ladder (1e-1 .. 1e-3) because ys - softening |d eps| cancels.

ERROR NORMS (``stress_scale``): a stress or force error is divided by (2 mu + lam) max(1, |F|^2) -- times vol for cloth,
where F = d D^-1 -- and an F or d error by |F| or |d|; never by the particle's own stress, which is ~0 near rest.

TOLERANCE: max(4 x the fp32 oracle's own distance from this module on the same family and field, 64 * 2^-24), measured
at test time.  Measured table (worst family per material; normalised as above; host = g++ builds of mpm_math.hpp without
/ with FMA contraction, device = MI355X, all back ends):

Per family: the worst case's oracle distance, host error (the larger of the two builds), device error (the
largest over baseline, fast, fast profiled, the two mixed-wavefront runs and the second substep); f = the largest of f1, f2, f3;
fields that are 0 everywhere (mu, lam; ys where the material has none) are left out.
  jelly: family | stress: oracle, host, device
    sv_range          | 8.9e-8, 7.8e-8, 7.5e-8
    identity          | 0, 0, 1.7e-14
    rotation          | 2.2e-7, 9.5e-8, 8.7e-8
    two_equal_large   | 1.4e-7, 7.6e-8, 8.1e-8
    two_equal_small   | 1.1e-7, 8.3e-8, 7.9e-8
    three_equal       | 5.9e-7, 6.6e-7, 4.1e-7
    near_equal_1e-5   | 4.8e-7, 6.5e-7, 6.5e-7
    compression       | 1.2e-7, 1.1e-7, 1.1e-7
    stretch           | 1.4e-7, 1.5e-7, 1.1e-7
    cond_1e2          | 1.1e-7, 1.5e-7, 1.1e-7
    cond_1e4          | 1.0e-7, 1.3e-7, 9.7e-8
    below_clamp_1     | 1.2e-7, 1.1e-7, 1.1e-7
    below_clamp_2     | 7.0e-8, 8.5e-8, 9.4e-8
    below_clamp_3     | 1.9e-9, 1.5e-9, 1.5e-9
    diagonal          | 1.7e-7, 1.7e-7, 1.7e-7
    signed_perm       | 0, 0, 8.1e-16
    inverted          | 2.0e-6, 5.1e-6, 6.1e-6
  metal: family | F: oracle, host, device | stress: oracle, host, device | ys: oracle, host, device
    sv_range          | 3.6e-7, 4.1e-7, 4.8e-7 | 2.8e-7, 6.3e-7, 3.4e-7 | 3.4e-7, 3.4e-7, 2.4e-7
    identity          | 0, 0, 8.6e-15 | 0, 0, 0 | 0, 0, 0
    rotation          | 0, 0, 0 | 7.1e-7, 2.0e-7, 1.7e-7 | 0, 0, 0
    two_equal_large   | 5.2e-7, 3.2e-7, 2.7e-7 | 5.0e-7, 2.1e-7, 2.0e-7 | 5.1e-8, 3.4e-8, 3.8e-8
    two_equal_small   | 4.7e-7, 2.5e-7, 2.1e-7 | 6.9e-7, 4.1e-7, 3.3e-7 | 4.5e-8, 3.8e-8, 4.0e-8
    three_equal       | 0, 0, 0 | 7.3e-7, 2.0e-7, 2.9e-7 | 0, 0, 0
    near_equal_1e-5   | 0, 0, 0 | 8.1e-7, 3.2e-7, 4.0e-7 | 0, 0, 0
    compression       | 3.7e-7, 4.0e-7, 3.3e-7 | 4.4e-7, 4.9e-7, 3.6e-7 | 3.5e-8, 3.2e-8, 2.8e-8
    stretch           | 3.5e-7, 3.5e-7, 2.5e-7 | 3.8e-7, 2.0e-7, 1.6e-7 | 2.5e-8, 2.2e-8, 2.8e-8
    cond_1e2          | 3.3e-7, 3.2e-7, 4.3e-7 | 4.8e-7, 6.7e-7, 4.6e-7 | 2.2e-7, 2.2e-7, 2.6e-7
    cond_1e4          | 8.1e-6, 8.1e-6, 7.4e-6 | 3.6e-7, 4.3e-7, 2.4e-7 | 6.6e-8, 6.6e-8, 6.6e-8
    below_clamp_1     | 1.3e-7, 1.3e-7, 1.7e-7 | 2.5e-7, 4.6e-7, 5.3e-7 | 8.2e-8, 8.2e-8, 8.2e-8
    below_clamp_2     | 2.2e-7, 2.2e-7, 2.0e-7 | 3.3e-7, 5.9e-7, 4.6e-7 | 5.6e-8, 6.1e-8, 6.1e-8
    below_clamp_3     | 0, 0, 0 | 2.4e-8, 2.5e-8, 1.9e-8 | 0, 0, 0
    diagonal          | 7.3e-8, 1.1e-7, 1.2e-7 | 6.9e-8, 1.5e-7, 1.9e-7 | 2.8e-8, 2.8e-8, 2.8e-8
    signed_perm       | 0, 0, 3.2e-15 | 0, 0, 0 | 0, 0, 0
    yield_in_1e-01    | 0, 0, 0 | 2.4e-7, 2.9e-7, 2.2e-7 | 0, 0, 0
    yield_in_1e-03    | 0, 0, 0 | 2.2e-7, 2.5e-7, 1.7e-7 | 0, 0, 0
    yield_in_1e-05    | 0, 0, 0 | 2.4e-7, 2.4e-7, 1.6e-7 | 0, 0, 0
    yield_on          | 7.5e-7, 7.3e-7, 7.3e-7 | 4.3e-7, 3.4e-7, 3.2e-7 | 1.4e-7, 1.5e-7, 1.4e-7
    yield_out_1e-01   | 5.8e-7, 4.7e-7, 2.7e-7 | 5.8e-7, 2.2e-7, 1.6e-7 | 3.0e-8, 3.0e-8, 2.1e-8
    yield_out_1e-03   | 4.3e-7, 4.6e-7, 4.7e-7 | 6.0e-7, 2.4e-7, 2.5e-7 | 1.9e-8, 3.0e-8, 2.8e-8
    yield_out_1e-05   | 4.2e-7, 4.6e-7, 3.4e-7 | 6.7e-7, 2.3e-7, 1.9e-7 | 2.9e-8, 3.5e-8, 2.9e-8
    rest_ys_negative  | 0, 0, 2.2e-15 | 0, 0, 0 | 6.7e-10, 6.7e-10, 6.7e-10
  sand: family | F: oracle, host, device | stress: oracle, host, device
    sv_range          | 2.1e-6, 2.5e-6, 1.5e-6 | 4.4e-5, 3.0e-5, 3.7e-5
    identity          | 0, 0, 2.4e-14 | 0, 0, 0
    rotation          | 5.9e-7, 1.9e-7, 2.8e-7 | 1.0e-6, 1.4e-7, 1.5e-7
    two_equal_large   | 4.0e-7, 3.0e-7, 2.0e-7 | 6.3e-7, 4.0e-7, 4.3e-7
    two_equal_small   | 3.5e-7, 3.3e-7, 2.5e-7 | 1.5e-6, 1.4e-6, 9.9e-7
    three_equal       | 5.3e-7, 1.5e-7, 1.7e-7 | 2.2e-6, 5.4e-7, 6.9e-7
    near_equal_1e-5   | 9.0e-7, 2.5e-7, 1.8e-7 | 3.7e-6, 9.9e-7, 1.0e-6
    compression       | 0, 0, 0 | 1.2e-6, 1.3e-6, 1.4e-6
    stretch           | 2.0e-7, 2.2e-7, 3.1e-7 | 7.3e-7, 5.5e-16, 1.6e-7
    cond_1e2          | 0, 0, 0 | 4.8e-5, 4.3e-5, 4.5e-5
    cond_1e4          | 0, 0, 0 | 7.2e-3, 7.2e-3, 7.0e-3
    below_clamp_1     | 0, 0, 0 | 6.2e-5, 1.2e-4, 8.9e-5
    below_clamp_2     | 0, 0, 0 | 1.6e-4, 1.4e-4, 1.8e-4
    below_clamp_3     | 0, 0, 0 | 5.6e-6, 4.8e-6, 5.2e-6
    diagonal          | 7.2e-8, 8.8e-8, 9.2e-8 | 2.5e-7, 4.0e-7, 4.0e-7
    signed_perm       | 0, 0, 2.9e-14 | 0, 0, 0
    yield_in_1e-01    | 0, 0, 0 | 2.6e-7, 2.6e-7, 1.8e-7
    yield_in_1e-03    | 0, 0, 0 | 2.2e-7, 2.4e-7, 1.9e-7
    yield_in_1e-05    | 0, 2.7e-7, 0 | 2.1e-7, 2.2e-7, 1.8e-7
    yield_on          | 7.1e-7, 7.3e-7, 3.3e-7 | 6.1e-7, 3.4e-7, 1.7e-7
    yield_out_1e-01   | 6.0e-7, 6.0e-7, 4.0e-7 | 6.7e-7, 3.4e-7, 2.0e-7
    yield_out_1e-03   | 6.1e-7, 6.3e-7, 5.2e-7 | 5.4e-7, 2.8e-7, 2.3e-7
    yield_out_1e-05   | 8.1e-7, 6.2e-7, 5.0e-7 | 6.4e-7, 3.3e-7, 2.8e-7
    tr_neg_1e-01      | 5.0e-7, 5.7e-7, 4.7e-7 | 5.1e-7, 2.9e-7, 1.8e-7
    tr_neg_1e-02      | 6.6e-7, 6.4e-7, 4.7e-7 | 4.8e-7, 2.9e-7, 2.1e-7
    tr_neg_1e-03      | 6.0e-7, 5.8e-7, 4.2e-7 | 5.6e-7, 2.4e-7, 1.8e-7
    tr_neg_1e-04      | 5.1e-7, 7.8e-7, 5.1e-7 | 7.5e-7, 3.0e-7, 2.0e-7
    tr_pos_1e-01      | 3.7e-7, 2.7e-7, 2.4e-7 | 6.8e-7, 5.3e-16, 1.3e-7
    tr_pos_1e-02      | 3.1e-7, 2.5e-7, 2.6e-7 | 8.2e-7, 5.8e-16, 1.7e-7
    tr_pos_1e-03      | 3.3e-7, 2.4e-7, 2.5e-7 | 1.1e-6, 7.0e-16, 1.5e-7
    tr_pos_1e-04      | 2.5e-7, 2.7e-7, 2.8e-7 | 8.4e-7, 5.7e-16, 1.8e-7
  foam: family | F: oracle, host, device | stress: oracle, host, device
    sv_range          | 4.4e-7, 4.5e-7, 6.6e-7 | 6.5e-7, 9.9e-7, 6.9e-7
    identity          | 0, 0, 9.9e-15 | 0, 0, 0
    rotation          | 0, 0, 0 | 6.3e-7, 1.3e-7, 1.9e-7
    two_equal_large   | 4.4e-7, 3.3e-7, 3.1e-7 | 3.9e-7, 1.8e-7, 2.2e-7
    two_equal_small   | 3.3e-7, 2.5e-7, 2.4e-7 | 5.2e-7, 3.9e-7, 5.8e-7
    three_equal       | 0, 0, 0 | 6.7e-7, 2.3e-7, 3.4e-7
    near_equal_1e-5   | 0, 0, 0 | 1.2e-6, 2.9e-7, 3.6e-7
    compression       | 2.8e-7, 4.9e-7, 3.4e-7 | 4.4e-7, 4.3e-7, 3.7e-7
    stretch           | 3.0e-7, 4.3e-7, 2.8e-7 | 3.8e-7, 2.9e-7, 2.1e-7
    cond_1e2          | 4.6e-7, 4.6e-7, 3.4e-7 | 1.4e-6, 1.2e-6, 1.0e-6
    cond_1e4          | 2.6e-6, 2.6e-6, 1.3e-6 | 1.0e-6, 1.3e-6, 1.4e-6
    below_clamp_1     | 3.2e-7, 3.6e-7, 3.1e-7 | 1.1e-6, 1.1e-6, 7.7e-7
    below_clamp_2     | 3.7e-7, 4.0e-7, 5.2e-7 | 6.7e-7, 1.4e-6, 1.2e-6
    below_clamp_3     | 0, 0, 0 | 2.3e-8, 2.7e-8, 2.2e-8
    diagonal          | 6.8e-8, 1.4e-7, 1.8e-7 | 1.1e-7, 1.9e-7, 3.2e-7
    signed_perm       | 0, 0, 7.1e-15 | 0, 0, 0
    yield_in_1e-01    | 0, 0, 0 | 2.1e-7, 2.2e-7, 1.4e-7
    yield_in_1e-03    | 0, 0, 0 | 1.9e-7, 2.3e-7, 1.8e-7
    yield_in_1e-05    | 0, 0, 0 | 2.0e-7, 2.3e-7, 1.7e-7
    yield_on          | 3.2e-7, 4.1e-7, 3.1e-7 | 3.9e-7, 2.2e-7, 1.7e-7
    yield_out_1e-01   | 5.2e-7, 5.8e-7, 3.1e-7 | 5.8e-7, 3.0e-7, 1.7e-7
    yield_out_1e-03   | 4.0e-7, 4.6e-7, 3.0e-7 | 4.7e-7, 2.8e-7, 1.8e-7
    yield_out_1e-05   | 4.0e-7, 4.3e-7, 3.2e-7 | 4.8e-7, 2.4e-7, 1.8e-7
  plasticine: family | F: oracle, host, device | stress: oracle, host, device | ys: oracle, host, device
    sv_range          | 2.4e-7, 2.9e-7, 2.9e-7 | 6.9e-8, 7.5e-8, 8.8e-8 | 3.1e-7, 3.1e-7, 3.3e-7
    identity          | 0, 0, 8.9e-14 | 0, 0, 2.9e-14 | 0, 0, 0
    rotation          | 0, 0, 0 | 2.2e-7, 5.9e-8, 1.0e-7 | 0, 0, 0
    two_equal_large   | 8.1e-7, 2.9e-7, 2.8e-7 | 4.9e-7, 2.5e-7, 1.8e-7 | 5.2e-8, 5.2e-8, 5.2e-8
    two_equal_small   | 5.2e-7, 3.0e-7, 2.2e-7 | 1.7e-7, 1.4e-7, 8.8e-8 | 4.3e-8, 5.0e-8, 3.3e-8
    three_equal       | 0, 0, 0 | 3.3e-7, 3.8e-7, 7.5e-7 | 0, 0, 0
    near_equal_1e-5   | 0, 0, 0 | 6.0e-7, 5.3e-7, 5.3e-7 | 0, 0, 0
    compression       | 3.3e-7, 4.0e-7, 2.9e-7 | 1.4e-7, 1.7e-7, 1.2e-7 | 2.5e-8, 2.8e-8, 2.6e-8
    stretch           | 3.0e-7, 3.3e-7, 2.9e-7 | 6.9e-7, 9.5e-7, 7.0e-7 | 2.7e-8, 2.6e-8, 3.0e-8
    cond_1e2          | 3.7e-7, 3.8e-7, 2.6e-7 | 5.1e-8, 6.6e-8, 8.6e-8 | 1.7e-7, 1.7e-7, 1.6e-7
    cond_1e4          | 2.0e-6, 3.5e-6, 3.0e-6 | 5.3e-8, 7.0e-8, 6.1e-8 | 6.7e-8, 6.7e-8, 6.7e-8
    below_clamp_1     | 1.9e-7, 1.8e-7, 1.1e-7 | 7.8e-8, 7.2e-8, 6.8e-8 | 1.1e-7, 1.1e-7, 6.3e-8
    below_clamp_2     | 1.7e-7, 2.0e-7, 2.8e-7 | 3.1e-8, 2.5e-8, 3.9e-8 | 8.4e-8, 8.4e-8, 8.9e-8
    below_clamp_3     | 0, 0, 0 | 1.4e-9, 1.7e-9, 1.8e-9 | 0, 0, 0
    diagonal          | 9.2e-8, 9.9e-8, 1.1e-7 | 1.2e-7, 1.6e-7, 2.7e-7 | 1.8e-8, 1.8e-8, 1.8e-8
    signed_perm       | 0, 0, 3.3e-15 | 0, 0, 9.8e-16 | 0, 0, 0
    yield_in_1e-01    | 0, 0, 0 | 1.1e-7, 1.0e-7, 6.6e-8 | 0, 0, 0
    yield_in_1e-03    | 0, 0, 0 | 8.4e-8, 8.2e-8, 8.1e-8 | 0, 0, 0
    yield_in_1e-05    | 0, 0, 0 | 8.7e-8, 9.6e-8, 6.6e-8 | 0, 0, 0
    yield_on          | 6.3e-7, 7.3e-7, 7.1e-7 | 3.2e-7, 5.1e-7, 3.8e-7 | 1.4e-7, 1.4e-7, 1.3e-7
    yield_out_1e-01   | 4.6e-7, 4.6e-7, 3.4e-7 | 3.9e-7, 4.1e-7, 3.3e-7 | 3.0e-8, 2.9e-8, 2.1e-8
    yield_out_1e-03   | 4.6e-7, 4.1e-7, 2.8e-7 | 6.0e-7, 4.5e-7, 2.9e-7 | 2.2e-8, 2.3e-8, 2.7e-8
    yield_out_1e-05   | 4.9e-7, 5.1e-7, 3.0e-7 | 5.2e-7, 3.5e-7, 3.5e-7 | 2.9e-8, 2.5e-8, 2.5e-8
    soften_live_1e-01 | 3.9e-7, 5.1e-7, 3.0e-7 | 4.1e-7, 6.0e-7, 2.8e-7 | 2.3e-8, 2.8e-8, 2.4e-8
    soften_live_1e-02 | 3.7e-7, 4.4e-7, 3.8e-7 | 5.1e-7, 5.9e-7, 2.9e-7 | 3.0e-8, 2.9e-8, 2.4e-8
    soften_live_1e-03 | 4.6e-7, 4.1e-7, 2.8e-7 | 4.1e-7, 3.6e-7, 2.9e-7 | 2.6e-8, 3.5e-8, 2.1e-8
    soften_dead_1e-01 | 3.5e-7, 3.6e-7, 3.5e-7 | 0, 0, 0 | 6.3e-10, 9.3e-10, 1.1e-9
    soften_dead_1e-02 | 4.0e-7, 4.0e-7, 3.4e-7 | 0, 0, 0 | 1.0e-9, 1.5e-9, 1.3e-9
    soften_dead_1e-03 | 4.4e-7, 4.1e-7, 3.9e-7 | 0, 0, 0 | 1.7e-9, 1.3e-9, 1.1e-9
    ys_zero           | 0, 0, 0 | 7.8e-8, 9.5e-8, 6.8e-8 | 0, 0, 0
    ys_negative       | 0, 0, 0 | 6.8e-8, 8.5e-8, 6.4e-8 | 0, 0, 0
  cloth: family | d: oracle, host, device | stress: oracle, host, device | f: oracle, host, device
    flat_exact        | 0, 0, 3.5e-15 | 0, 0, 0 | 2.0e-6, 1.5e-6, 1.5e-6
    general           | 2.6e-7, 2.6e-7, 2.6e-7 | 4.4e-7, 4.5e-7, 4.7e-7 | 1.7e-5, 2.2e-5, 1.8e-5
    r22_over_1e-04    | 1.9e-7, 1.9e-7, 1.9e-7 | 8.1e-7, 5.0e-7, 5.7e-7 | 2.7e-5, 2.0e-5, 2.4e-5
    r22_over_1e-03    | 1.7e-7, 1.7e-7, 1.7e-7 | 1.2e-6, 7.7e-7, 7.7e-7 | 4.8e-5, 3.4e-5, 3.4e-5
    r22_over_1e-02    | 2.0e-7, 2.0e-7, 2.0e-7 | 1.2e-6, 7.3e-7, 7.3e-7 | 4.8e-5, 2.9e-5, 2.8e-5
    r22_over_1e-01    | 2.1e-7, 2.1e-7, 2.1e-7 | 1.1e-6, 5.7e-7, 5.6e-7 | 5.6e-5, 2.4e-5, 2.3e-5
    r22_over_5e-01    | 1.8e-7, 1.8e-7, 1.8e-7 | 1.2e-6, 7.8e-7, 7.8e-7 | 6.3e-5, 4.0e-5, 4.0e-5
    r22_under_1e-04   | 1.6e-7, 1.6e-7, 1.6e-7 | 1.3e-6, 6.8e-7, 6.9e-7 | 3.8e-5, 2.9e-5, 2.9e-5
    r22_under_1e-03   | 3.0e-7, 3.0e-7, 3.0e-7 | 5.5e-7, 2.0e-7, 4.6e-7 | 3.2e-5, 9.9e-6, 2.8e-5
    r22_under_1e-02   | 3.0e-7, 3.0e-7, 3.0e-7 | 6.7e-7, 3.5e-7, 3.5e-7 | 1.5e-5, 8.2e-6, 8.2e-6
    r22_under_1e-01   | 2.8e-7, 3.6e-7, 2.8e-7 | 6.4e-7, 4.1e-7, 4.1e-7 | 2.7e-5, 1.7e-5, 1.7e-5
    r22_under_5e-01   | 3.9e-7, 3.9e-7, 3.9e-7 | 5.5e-7, 6.8e-7, 7.7e-7 | 1.4e-5, 1.5e-5, 1.6e-5
    fric_in_1e-04     | 3.6e-7, 3.6e-7, 3.6e-7 | 8.3e-7, 4.6e-7, 3.3e-7 | 2.4e-5, 1.6e-5, 1.3e-5
    fric_in_1e-03     | 2.2e-7, 2.2e-7, 3.2e-7 | 8.8e-7, 4.0e-7, 4.2e-7 | 3.3e-5, 2.3e-5, 2.5e-5
    fric_in_1e-02     | 3.1e-7, 3.1e-7, 3.1e-7 | 6.4e-7, 4.2e-7, 5.5e-7 | 1.5e-5, 1.2e-5, 1.3e-5
    fric_in_1e-01     | 2.9e-7, 3.6e-7, 3.3e-7 | 5.0e-7, 2.2e-7, 2.4e-7 | 1.2e-5, 7.2e-6, 6.5e-6
    fric_in_5e-01     | 3.6e-7, 3.6e-7, 3.6e-7 | 4.7e-7, 3.0e-7, 2.7e-7 | 1.1e-5, 1.4e-5, 1.2e-5
    fric_out_1e-04    | 2.9e-7, 2.9e-7, 2.9e-7 | 1.4e-6, 5.9e-7, 6.3e-7 | 6.0e-5, 2.8e-5, 2.8e-5
    fric_out_1e-03    | 2.6e-7, 2.6e-7, 2.6e-7 | 4.2e-7, 1.9e-7, 2.2e-7 | 1.0e-5, 1.7e-5, 1.7e-5
    fric_out_1e-02    | 2.8e-7, 3.5e-7, 2.8e-7 | 6.5e-7, 4.1e-7, 4.1e-7 | 2.3e-5, 2.1e-5, 2.0e-5
    fric_out_1e-01    | 3.1e-7, 3.1e-7, 3.1e-7 | 9.7e-7, 4.4e-7, 4.4e-7 | 2.9e-5, 1.8e-5, 2.1e-5
    fric_out_5e-01    | 3.9e-7, 3.9e-7, 3.9e-7 | 4.4e-7, 4.4e-7, 4.3e-7 | 3.0e-5, 2.3e-5, 2.1e-5
    gamma0            | 2.9e-7, 3.1e-7, 2.9e-7 | 2.5e-7, 7.3e-8, 9.7e-8 | 3.6e-6, 3.3e-6, 3.2e-6
    aspect            | 3.4e-7, 4.9e-7, 3.4e-7 | 2.1e-6, 3.3e-6, 1.9e-6 | 4.2e-3, 3.8e-3, 3.6e-3
    folded            | 2.2e-7, 2.3e-7, 2.6e-7 | 6.4e-6, 3.9e-6, 4.1e-6 | 5.6e-5, 3.7e-5, 3.3e-5
  cloth_fc0: family | d: oracle, host, device | stress: oracle, host, device | f: oracle, host, device
    flat_exact        | 0, 0, 3.5e-15 | 0, 0, 0 | 2.0e-6, 1.5e-6, 1.5e-6
    general           | 2.3e-7, 2.3e-7, 2.3e-7 | 4.4e-7, 4.5e-7, 4.7e-7 | 1.6e-5, 2.2e-5, 1.8e-5
    r22_over_1e-04    | 1.9e-7, 1.9e-7, 1.9e-7 | 8.1e-7, 5.0e-7, 5.7e-7 | 2.7e-5, 2.0e-5, 2.4e-5
    r22_over_1e-03    | 1.7e-7, 1.7e-7, 1.7e-7 | 1.2e-6, 7.7e-7, 7.7e-7 | 4.8e-5, 3.4e-5, 3.4e-5
    r22_over_1e-02    | 2.0e-7, 2.0e-7, 2.0e-7 | 1.2e-6, 7.3e-7, 7.3e-7 | 4.8e-5, 2.9e-5, 2.8e-5
    r22_over_1e-01    | 2.1e-7, 2.1e-7, 2.1e-7 | 1.1e-6, 5.7e-7, 5.6e-7 | 5.6e-5, 2.4e-5, 2.3e-5
    r22_over_5e-01    | 1.8e-7, 1.8e-7, 1.8e-7 | 1.2e-6, 7.8e-7, 7.8e-7 | 6.3e-5, 4.0e-5, 4.0e-5
    r22_under_1e-04   | 1.6e-7, 1.6e-7, 1.6e-7 | 1.3e-6, 6.8e-7, 6.9e-7 | 3.8e-5, 2.9e-5, 2.9e-5
    r22_under_1e-03   | 2.4e-7, 2.4e-7, 2.4e-7 | 3.9e-7, 1.1e-9, 1.1e-9 | 2.4e-5, 5.5e-6, 6.5e-6
    r22_under_1e-02   | 2.8e-7, 2.8e-7, 3.3e-7 | 3.3e-7, 9.9e-9, 1.3e-8 | 9.5e-6, 3.7e-6, 4.0e-6
    r22_under_1e-01   | 2.3e-7, 2.8e-7, 2.3e-7 | 4.4e-7, 1.3e-7, 1.3e-7 | 1.6e-5, 3.8e-6, 3.7e-6
    r22_under_5e-01   | 3.1e-7, 3.1e-7, 3.2e-7 | 4.0e-7, 2.4e-7, 2.5e-7 | 1.0e-5, 4.4e-6, 4.3e-6
    fric_in_1e-04     | 3.6e-7, 3.6e-7, 3.6e-7 | 5.7e-7, 1.2e-7, 1.9e-7 | 9.2e-6, 4.2e-6, 4.2e-6
    fric_in_1e-03     | 2.6e-7, 2.6e-7, 3.4e-7 | 4.1e-7, 1.1e-7, 1.4e-7 | 8.9e-6, 5.0e-6, 5.0e-6
    fric_in_1e-02     | 2.9e-7, 3.0e-7, 2.9e-7 | 4.8e-7, 1.7e-7, 1.7e-7 | 7.8e-6, 5.5e-6, 5.7e-6
    fric_in_1e-01     | 3.0e-7, 3.3e-7, 3.0e-7 | 3.9e-7, 1.1e-7, 2.1e-7 | 6.8e-6, 3.4e-6, 3.6e-6
    fric_in_5e-01     | 3.4e-7, 3.4e-7, 3.4e-7 | 5.9e-7, 1.4e-7, 1.4e-7 | 6.7e-6, 4.1e-6, 4.6e-6
    fric_out_1e-04    | 2.9e-7, 2.9e-7, 3.0e-7 | 7.6e-7, 1.7e-7, 1.7e-7 | 2.3e-5, 5.5e-6, 4.7e-6
    fric_out_1e-03    | 2.7e-7, 2.8e-7, 3.4e-7 | 2.8e-7, 1.7e-7, 1.7e-7 | 6.0e-6, 4.9e-6, 4.5e-6
    fric_out_1e-02    | 2.7e-7, 3.5e-7, 2.7e-7 | 6.0e-7, 1.8e-7, 2.1e-7 | 1.2e-5, 5.2e-6, 5.4e-6
    fric_out_1e-01    | 2.2e-7, 2.8e-7, 3.0e-7 | 5.7e-7, 1.4e-7, 1.8e-7 | 6.4e-6, 3.8e-6, 3.9e-6
    fric_out_5e-01    | 3.8e-7, 3.8e-7, 3.9e-7 | 3.2e-7, 9.8e-8, 8.0e-8 | 1.2e-5, 4.8e-6, 4.8e-6
    gamma0            | 2.9e-7, 3.1e-7, 2.9e-7 | 2.5e-7, 7.3e-8, 9.7e-8 | 3.6e-6, 3.3e-6, 3.2e-6
    aspect            | 3.8e-7, 5.1e-7, 3.8e-7 | 2.1e-6, 3.3e-6, 1.9e-6 | 4.2e-3, 3.8e-3, 3.6e-3
    folded            | 2.0e-7, 2.4e-7, 3.2e-7 | 6.8e-6, 4.2e-6, 4.5e-6 | 2.4e-5, 6.3e-6, 6.3e-6
"""
from __future__ import annotations

import numpy as np

TRAD_MATERIALS = {"jelly": 0, "metal": 1, "sand": 2, "foam": 3, "plasticine": 5}
SV_MIN, SV_MAX = 0.005, 5.0          # singular values of the tested domain (family sv_range)
MARGIN_R22 = MARGIN_FRIC = MARGIN_TR = 5e-5     # half the smallest rung (1e-4): the fp32 rounding of the input moves a rung by ~1e-6 of itself
MARGIN_SOFTEN = 5e-4                            # half of 1e-3
REST_EPS = 1e-6
FLOOR = 64.0 * 2.0 ** -24
FACTOR = 4.0


# ------------------------------------------------------------------------------------------------ algebra
def svd_rot(A):
    """LAPACK SVD A = U diag(s) V^T with det U = det V = +1; the sign of det A sits in s[..., 2]."""
    U, s, Vt = np.linalg.svd(A)
    V = np.swapaxes(Vt, -1, -2).copy()
    U, s = U.copy(), s.copy()
    for M in (U, V):
        neg = np.linalg.det(M) < 0
        M[neg, :, 2] *= -1.0
        s[neg, 2] *= -1.0
    return U, s, V


def _udv(U, t, V):
    return np.einsum("nij,nj,nkj->nik", U, t, V)


def qr_closed(d):
    """The unique QR with R00, R11 >= 0 and det Q = +1 (what qr3 followed by the sign flips of mpm_utils.py:112-123 gives)."""
    d1, d2, d3 = d[..., 0], d[..., 1], d[..., 2]
    r00 = np.linalg.norm(d1, axis=-1)
    q1 = d1 / r00[..., None]
    r01 = (q1 * d2).sum(-1)
    u2 = d2 - r01[..., None] * q1
    r11 = np.linalg.norm(u2, axis=-1)
    q2 = u2 / r11[..., None]
    q3 = np.cross(q1, q2)
    Q = np.stack([q1, q2, q3], -1)
    R = np.zeros_like(d)
    R[..., 0, 0], R[..., 0, 1], R[..., 1, 1] = r00, r01, r11
    R[..., 0, 2], R[..., 1, 2], R[..., 2, 2] = (q1 * d3).sum(-1), (q2 * d3).sum(-1), (q3 * d3).sum(-1)
    return Q, R


def _arr(a, n):
    return np.array(np.broadcast_to(np.asarray(a, np.float64), (n,)))


# ------------------------------------------------------------------------------------------------ traditional particles
def trad_update(F_trial, material, mu, lam, ys, alpha=0.0, hardening=0.0, xi=0.0, plastic_viscosity=0.0, softening=0.1,
                dt=1e-4, info=None):
    """compute_stress_from_F_trial for traditional particles (mpm_utils.py:1047-1105) -> F, stress, mu, lam, ys.

    material: 0 jelly, 1 metal, 2 sand, 3 foam, 5 plasticine; 4, 6, 7 pass F_trial through with zero stress (quirk Q4).
    info (a dict, optional) receives the float64 branch variables of the return map."""
    Ft = np.array(F_trial, np.float64).reshape(-1, 3, 3)
    n = Ft.shape[0]
    mu, lam, ys = _arr(mu, n), _arr(lam, n), _arr(ys, n)
    info = {} if info is None else info
    if material not in (0, 1, 2, 3, 5):
        return Ft.copy(), np.zeros_like(Ft), mu, lam, ys
    F = Ft.copy()
    with np.errstate(all="ignore"):
        if material in (1, 5):      # von_mises_return_mapping (:212-255), .._with_damage (:258-311)
            U, s, V = svd_rot(Ft)
            eps = np.log(np.maximum(s, 0.01))
            tr = eps.sum(-1)
            tau = 2.0 * mu[:, None] * eps + (lam * tr)[:, None]
            cond = tau - tau.sum(-1, keepdims=True) / 3.0
            cn = np.linalg.norm(cond, axis=-1)
            y = cn > ys
            info["yield_fn"] = cn / np.where(ys != 0, ys, 1.0) - 1.0
            if material == 5:
                y &= ~(ys <= 0)     # :281-282
            eh = eps - tr[:, None] / 3.0
            ehn = np.linalg.norm(eh, axis=-1) + 1e-6
            dg = ehn - ys / (2.0 * mu)
            corr = (dg / ehn)[:, None] * eh
            Fy = _udv(U, np.exp(eps - corr), V)
            if material == 5:       # :287-292
                ys1 = ys - softening * np.linalg.norm(corr, axis=-1)
                info["softened"] = np.where(y, ys1 / np.where(ys != 0, ys, 1.0), np.nan)
                dead = y & (ys1 <= 0)
                ys = np.where(y, ys1, ys)
                mu, lam = np.where(dead, 0.0, mu), np.where(dead, 0.0, lam)
            if hardening == 1:      # :249-252, :305-308 (with the mu the damage model may just have zeroed)
                ys = np.where(y, ys + 2.0 * mu * xi * dg, ys)
            F = np.where(y[:, None, None], Fy, Ft)
            info["changed"] = y
        elif material == 3:         # viscoplasticity_return_mapping_with_StVK (:315-359)
            U, s, V = svd_rot(Ft)
            sc = np.maximum(s, 0.01)
            b = sc * sc
            eps = np.log(sc)
            tr = eps.sum(-1)
            eh = eps - tr[:, None] / 3.0
            st = 2.0 * mu[:, None] * eh
            stn = np.linalg.norm(st, axis=-1)
            yv = stn - np.sqrt(2.0 / 3.0) * ys
            y = yv > 0
            info["yield_fn"] = stn / np.where(ys != 0, np.sqrt(2.0 / 3.0) * ys, 1.0) - 1.0
            mu_hat = mu * b.sum(-1) / 3.0
            snn = stn - yv / (1.0 + plastic_viscosity / (2.0 * mu_hat * dt))
            sn = (snn / np.where(stn > 0, stn, 1.0))[:, None] * st
            Fy = _udv(U, np.exp(sn / (2.0 * mu[:, None]) + tr[:, None] / 3.0), V)
            F = np.where(y[:, None, None], Fy, Ft)
            info["changed"] = y
        elif material == 2:         # sand_return_mapping (:362-399)
            U, s, V = svd_rot(Ft)
            eps = np.log(np.maximum(np.abs(s), 1e-14))
            tr = eps.sum(-1)
            eh = eps - tr[:, None] / 3.0
            ehn = np.linalg.norm(eh, axis=-1)
            dg = ehn + (3.0 * lam + 2.0 * mu) / (2.0 * mu) * tr * alpha
            a = (dg > 0) & (tr > 0)
            bm = (dg > 0) & (tr <= 0)
            H = eps - eh * (dg / np.where(ehn > 0, ehn, 1.0))[:, None]
            F = np.where(a[:, None, None], _udv(U, np.ones_like(s), V), F)
            F = np.where(bm[:, None, None], _udv(U, np.exp(H), V), F)
            info.update(tr=tr, dg=dg, ehn=ehn, yield_fn=dg / np.where(ehn > 0, ehn, 1.0), changed=a | bm)
        # stress of the mapped F (:1072-1103): a second decomposition, as the reference does
        J = np.linalg.det(F)
        U, s, V = svd_rot(F)
        FT = np.swapaxes(F, -1, -2)
        if material in (0, 5):      # kirchoff_stress_FCR (:8-15)
            S = 2.0 * mu[:, None, None] * ((F - _udv(U, np.ones_like(s), V)) @ FT) + (lam * J * (J - 1.0))[:, None, None] * np.eye(3)
        elif material in (1, 3):    # kirchoff_stress_StVK (:50-66)
            e = np.log(np.maximum(s, 0.01))
            S = _udv(U, 2.0 * mu[:, None] * e + (lam * e.sum(-1))[:, None], V) @ FT
        else:                       # kirchoff_stress_drucker_prager (:69-84); log of a negative singular value: NaN (quirk Q10)
            ls = np.log(s)
            c = (2.0 * mu[:, None] * ls + (lam * ls.sum(-1))[:, None]) / s
            S = _udv(U, c, V) @ FT
            info["dp_amp"] = np.abs(c).max(-1) * _fro(F)     # the largest intermediate: center (divided by s) times F^T again
        S = 0.5 * (S + np.swapaxes(S, -1, -2))
    return F, S, mu, lam, ys


# ------------------------------------------------------------------------------------------------ cloth elements
def cloth_return_map(d, gamma, kappa, friction_coeff, info=None):
    """anisotropy_return_mapping (mpm_utils.py:179-209) -> d_new, Q, R with the mapped third column."""
    d = np.array(d, np.float64).reshape(-1, 3, 3)
    n = d.shape[0]
    gamma, kappa = _arr(gamma, n), _arr(kappa, n)
    Q, R = qr_closed(d)
    r02, r12, r22 = R[:, 0, 2].copy(), R[:, 1, 2].copy(), R[:, 2, 2].copy()
    over = r22 > 1.0                                            # :196-197
    fn = kappa * (1.0 - r22) ** 2                               # :199
    ff = gamma * np.sqrt(r02 * r02 + r12 * r12)                 # :200
    slide = (~over) & (ff > friction_coeff * fn)                # :201-202
    scale = np.where(slide, friction_coeff * fn / np.where(ff > 0, ff, 1.0), 1.0)
    if info is not None:
        thr = friction_coeff * fn
        info.update(r22=r22.copy(), over=over, slide=slide,
                    fric=np.where((~over) & (thr > 0), ff / np.where(thr > 0, thr, 1.0) - 1.0, np.nan))
    R = R.copy()
    R[:, 0, 2], R[:, 1, 2], R[:, 2, 2] = r02 * scale, r12 * scale, np.where(over, 1.0, r22)
    d_new = d.copy()
    d_new[:, :, 2] = np.einsum("nij,nj->ni", Q, R[:, :, 2])     # :206-207
    return d_new, Q, R


def cloth_stress(d_new, Q, R, R_inv, vol, mu, lam, gamma, kappa):
    """kirchoff_stress_Anisotropy (mpm_utils.py:101-177) of the mapped d, whose QR is (Q, R): d1, d2 are untouched by the
    return map, so Q and the first two columns of R are those of the input."""
    n = d_new.shape[0]
    R_inv = np.array(R_inv, np.float64).reshape(n, 3)
    vol, mu, lam, gamma, kappa = (_arr(a, n) for a in (vol, mu, lam, gamma, kappa))
    iD11, iD12, iD22 = R_inv[:, 0], R_inv[:, 1], R_inv[:, 2]
    F11 = R[:, 0, 0] * iD11
    F12 = R[:, 0, 0] * iD12 + R[:, 0, 1] * iD22
    F22 = R[:, 1, 1] * iD22
    th = np.arctan2(-F12, F11 + F22)    # U V^T of the zero-padded block (:133-141) = polar rotation of [[F11, F12], [0, F22]]
    c, s = np.cos(th), np.sin(th)
    J = F11 * F22
    lj = lam * (J - 1.0)
    dr = np.zeros((n, 3, 3))            # :144-156
    dr[:, 0, 0] = 2.0 * mu * (F11 - c) + lj * F22
    dr[:, 0, 1] = 2.0 * mu * (F12 + s)
    dr[:, 1, 1] = 2.0 * mu * (F22 - c) + lj * F11
    dr[:, 0, 2], dr[:, 1, 2] = gamma * R[:, 0, 2], gamma * R[:, 1, 2]
    dr[:, 2, 2] = np.where(R[:, 2, 2] > 1.0, 0.0, -kappa * (1.0 - R[:, 2, 2]) ** 2)
    RiDT = np.zeros((n, 3, 3))          # :130
    RiDT[:, 0, 0], RiDT[:, 1, 0], RiDT[:, 1, 1] = F11, F12, F22
    RiDT[:, 2, 0], RiDT[:, 2, 1], RiDT[:, 2, 2] = R[:, 0, 2], R[:, 1, 2], R[:, 2, 2]
    K3 = dr @ RiDT
    K3s = np.triu(K3) + np.swapaxes(np.triu(K3, 1), -1, -2)     # :158
    P = Q @ K3s @ np.linalg.inv(RiDT)
    f2 = -vol[:, None] * (iD11[:, None] * P[:, :, 0] + iD12[:, None] * P[:, :, 1])
    f3 = -vol[:, None] * iD22[:, None] * P[:, :, 1]
    f1 = -(f2 + f3)
    stress = vol[:, None, None] * np.einsum("ni,nj->nij", P[:, :, 2], d_new[:, :, 2])
    return stress, f1, f2, f3


def cloth_update(d, R_inv, vol, mu, lam, gamma, kappa, friction_coeff, info=None):
    """The element branch of compute_stress_from_F_trial (mpm_utils.py:1030-1045) -> d_new, stress, f1, f2, f3."""
    d_new, Q, R = cloth_return_map(d, gamma, kappa, friction_coeff, info)
    return (d_new,) + cloth_stress(d_new, Q, R, R_inv, vol, mu, lam, gamma, kappa)


# ------------------------------------------------------------------------------------------------ error norms
def _fro(a):
    return np.sqrt((np.asarray(a, np.float64) ** 2).reshape(len(a), -1).sum(-1))


def stress_scale(F, mu, lam, vol=1.0):
    """(2 mu + lam) max(1, |F|^2) [vol]: what a stress (or, for cloth, a vertex force) error is divided by."""
    return (2.0 * np.asarray(mu, np.float64) + np.asarray(lam, np.float64)) * np.maximum(1.0, _fro(F) ** 2) * vol


def cloth_F(d, R_inv):
    """F = d D^-1 of an element: D^-1 = [[iD11, iD12, 0], [0, iD22, 0], [0, 0, 1]]."""
    d, R_inv = np.asarray(d, np.float64), np.asarray(R_inv, np.float64)
    Di = np.zeros_like(d)
    Di[:, 0, 0], Di[:, 0, 1], Di[:, 1, 1], Di[:, 2, 2] = R_inv[:, 0], R_inv[:, 1], R_inv[:, 2], 1.0
    return d @ Di


def field_errors(got, want, scales):
    """{field: per-particle |got - want| / scale}; a non-finite `want` entry asks for a non-finite `got` entry (error 0 / inf)."""
    out = {}
    for k, w in want.items():
        g, w = np.asarray(got[k], np.float64).reshape(len(w), -1), np.asarray(w, np.float64).reshape(len(w), -1)
        fin = np.isfinite(w)
        mism = (fin != np.isfinite(g)).any(-1)
        diff = np.where(fin & np.isfinite(g), g - w, 0.0)
        out[k] = np.where(mism, np.inf, np.sqrt((diff ** 2).sum(-1)) / scales[k])
    return out


def by_family(err, family, names):
    return {nm: float(err[family == i].max()) for i, nm in enumerate(names) if (family == i).any()}


def bound(oracle_distance):
    return max(FACTOR * oracle_distance, FLOOR)


# Absolute statements -- what an fp32 evaluation of the update may be away from float64 whatever the yardstick says.  In the
# norms above everything is a few ulp, with two stated exceptions, each a property of the formula and not of an implementation:
#   * the Drucker-Prager stress (mpm_utils.py:69-84) forms center = (2 mu log s + lam tr) / s and multiplies U center V^T by
#     F^T again: the result is O(modulus), the intermediate product O(|center| |F|) -- cond(F) times larger for a compressed,
#     ill-conditioned F -- and every fp32 evaluation rounds at that size;
#   * a vertex force is a stress times D^-1 (one over an edge length; 20 ... 50 per metre here, 5000 in the 1:100 triangles),
#     and the norm divides it by a stress.
# `conditioning` returns that factor per case (1 everywhere else).  PIN (= FLOOR) times it bounds the reference's own fp32
# run (the fixture); ORACLE_CEILING times it bounds the yardstick itself, so that an error in this module cannot widen the
# bounds that are derived from the oracle's distance: 1e-4 is the project's blanket tolerance, 26 floors.
PIN = FLOOR
ORACLE_CEILING = 1e-4


def conditioning(tab, info, scales):
    """{field: per-case factor >= 1} for a table whose float64 evaluation left `info`."""
    n = len(tab["family"])
    out = {k: np.ones(n) for k in scales}
    if "dp_amp" in info:     # 4 ulp of the largest intermediate, in floors: 4 * 2^-24 / FLOOR = 1 / 16
        out["stress"] = np.maximum(1.0, np.where(np.isfinite(info["dp_amp"]), info["dp_amp"], 0.0) / (16.0 * scales["stress"]))
    if "R_inv" in tab:
        for k in ("f1", "f2", "f3"):
            out[k] = np.maximum(1.0, np.abs(np.asarray(tab["R_inv"], np.float64)).max(-1))
    return out


# ------------------------------------------------------------------------------------------------ the edge table
def _rotations(rng, n):
    Q = np.linalg.qr(rng.standard_normal((n, 3, 3)))[0]
    Q[np.linalg.det(Q) < 0, :, 2] *= -1.0
    return Q


def _signed_perms():
    import itertools
    out = []
    for p in itertools.permutations(range(3)):
        for sg in itertools.product((1.0, -1.0), repeat=3):
            M = np.zeros((3, 3))
            M[np.arange(3), list(p)] = sg
            if np.linalg.det(M) > 0:
                out.append(M)
    return np.array(out)   # the 24 proper ones


def _compose(rng, s):
    n = s.shape[0]
    return _udv(_rotations(rng, n), s, _rotations(rng, n))


def _lame(rng, n):
    E = rng.uniform(10.0, 100.0, n).astype(np.float32)
    nu = np.float32(0.3)
    one, two = np.float32(1.0), np.float32(2.0)
    return (E / (two * (one + nu))).astype(np.float32), (E * nu / ((one + nu) * (one - two * nu))).astype(np.float32)


LADDER = (1e-1, 1e-3, 1e-5)
TR_LADDER = (1e-1, 1e-2, 1e-3, 1e-4)
SOFTEN_LADDER = (1e-1, 1e-2, 1e-3)
CLOTH_LADDER = (1e-4, 1e-3, 1e-2, 1e-1, 0.5)
TRAD_PARAMS = {"hardening": 1.0, "xi": 0.2, "plastic_viscosity": 4e-5, "softening": 0.15, "dt": 1e-6, "friction_angle": 40.0}


def sand_alpha(angle):
    """mpm_solver.py:90-94 (with its 3.14159265)."""
    import math
    sin_phi = math.sin(angle / 180.0 * 3.14159265)
    return float(np.float32(math.sqrt(2.0 / 3.0) * 2.0 * sin_phi / (3.0 - sin_phi)))


def friction_coeff_of(angle):
    import math
    return float(np.float32(math.tan(angle / 180.0 * 3.14159265)))


def _dev_dirs(rng, n, lo, hi):
    """n deviatoric log-strain vectors of norm in [lo, hi]."""
    e = rng.standard_normal((n, 3))
    e -= e.mean(-1, keepdims=True)
    e /= np.linalg.norm(e, axis=-1, keepdims=True)
    return e * rng.uniform(lo, hi, (n, 1))


def trad_table(material, count=64, host_only=False):
    """The edge table of one traditional material (a name of TRAD_MATERIALS).  count: cases per family.  Returns a dict:
    F_trial [n,3,3], mu, lam, ys [n] (float32), family [n] (index into names), names, material (the integer), and the model
    scalars alpha, hardening, xi, plastic_viscosity, softening, dt.  host_only=True returns instead the inputs whose float64
    stress is not finite (inverted sand), which no GPU test is given."""
    m = TRAD_MATERIALS[material]
    rng = np.random.default_rng(1000 + m)
    N = count
    fams = []   # (name, F [N,3,3] float64, ys or None)
    lu = lambda lo, hi, *shape: np.exp(rng.uniform(np.log(lo), np.log(hi), shape))
    srt = lambda s: -np.sort(-s, axis=-1)

    if host_only:
        assert material == "sand"
        s = srt(lu(0.3, 2.0, N, 3))
        s[:, 2] *= -1.0
        fams.append(("inverted_sand", _compose(rng, s), None))
    else:
        fams.append(("sv_range", _compose(rng, srt(lu(SV_MIN, SV_MAX, N, 3))), None))
        fams.append(("identity", np.tile(np.eye(3), (N, 1, 1)), None))
        fams.append(("rotation", _rotations(rng, N), None))
        a, b = lu(0.8, 2.0, N), lu(0.2, 0.7, N)
        fams.append(("two_equal_large", _compose(rng, np.stack([a, a, b], -1)), None))
        fams.append(("two_equal_small", _compose(rng, np.stack([a, b, b], -1)), None))
        a = lu(0.5, 2.0, N)
        fams.append(("three_equal", _compose(rng, np.stack([a, a, a], -1)), None))
        fams.append(("near_equal_1e-5", _compose(rng, a[:, None] * (1.0 + 1e-5 * rng.uniform(-1, 1, (N, 3)))), None))
        fams.append(("compression", _compose(rng, rng.uniform(0.3, 0.9, (N, 1)) * (1.0 + 0.05 * rng.uniform(-1, 1, (N, 3)))), None))
        s = 1.0 + 0.05 * rng.uniform(-1, 1, (N, 3))
        s[:, 0] = rng.uniform(1.1, 3.0, N)
        fams.append(("stretch", _compose(rng, s), None))
        for c in (1e2, 1e4):
            top = lu(0.5, 2.0, N)
            fams.append((f"cond_{c:.0e}".replace("+0", ""), _compose(rng, np.stack([top, top * lu(1.0 / c, 1.0, N), top / c], -1)), None))
        for k in (1, 2, 3):
            s = lu(0.3, 2.0, N, 3)
            s[:, 3 - k:] = lu(0.002, 0.0095, N, k)
            fams.append((f"below_clamp_{k}", _compose(rng, srt(s)), None))
        s = lu(0.3, 2.0, N, 3)
        D = np.zeros((N, 3, 3))
        D[:, [0, 1, 2], [0, 1, 2]] = s
        fams.append(("diagonal", D, None))
        P = _signed_perms()
        fams.append(("signed_perm", P[np.arange(N) % len(P)], None))
        if material == "jelly":
            s = srt(lu(0.3, 2.0, N, 3))
            s[:, 2] *= -1.0
            fams.append(("inverted", _compose(rng, s), None))

    n_plain = len(fams)
    thr = []    # threshold families: (name, deviatoric log strain eh, volumetric tr, spec)
    if not host_only and material in ("metal", "foam", "plasticine"):
        for nm, sg in [(f"yield_in_{r:.0e}", -r) for r in LADDER] + [("yield_on", 0.0)] + [(f"yield_out_{r:.0e}", r) for r in LADDER]:
            thr.append((nm, _dev_dirs(rng, N, 0.05, 0.3), rng.uniform(-0.2, 0.2, N), ("yield", sg)))
        if material == "plasticine":
            for nm, sg in [(f"soften_live_{r:.0e}", r) for r in SOFTEN_LADDER] + [(f"soften_dead_{r:.0e}", -r) for r in SOFTEN_LADDER]:
                thr.append((nm, _dev_dirs(rng, N, 0.05, 0.3), rng.uniform(-0.2, 0.2, N), ("soften", sg)))
            thr.append(("ys_zero", _dev_dirs(rng, N, 0.05, 0.3), rng.uniform(-0.2, 0.2, N), ("ys", 0.0)))
            thr.append(("ys_negative", _dev_dirs(rng, N, 0.05, 0.3), rng.uniform(-0.2, 0.2, N), ("ys", -0.5)))
        if material == "metal":     # eps = 0 exactly and ys < 0: |dev tau| = 0 > ys "yields" with dev eps = 0 -- what the + 1e-6 is for
            Pm = np.concatenate([np.eye(3)[None], _signed_perms()])
            thr.append(("rest_ys_negative", Pm[np.arange(N) % len(Pm)], None, ("ys_draw", -lu(0.01, 1.0, N))))
    mu_all, lam_all = _lame(rng, (n_plain + len(thr) + 15) * N)
    alpha = sand_alpha(TRAD_PARAMS["friction_angle"])
    if not host_only and material == "sand":
        k0 = n_plain * N
        ca = lambda i: ((3.0 * lam_all[k0 + i * N:k0 + (i + 1) * N].astype(np.float64) + 2.0 * mu_all[k0 + i * N:k0 + (i + 1) * N])
                        / (2.0 * mu_all[k0 + i * N:k0 + (i + 1) * N]) * alpha)
        i = 0
        for nm, sg in [(f"yield_in_{r:.0e}", -r) for r in LADDER] + [("yield_on", 0.0)] + [(f"yield_out_{r:.0e}", r) for r in LADDER]:
            eh = _dev_dirs(rng, N, 0.05, 0.3)
            tr = -np.linalg.norm(eh, axis=-1) * (1.0 - sg) / ca(i)     # dg / |eh| = sg
            thr.append((nm, eh, tr, None)); i += 1
        for nm, t in [(f"tr_neg_{r:.0e}", -r) for r in TR_LADDER] + [(f"tr_pos_{r:.0e}", r) for r in TR_LADDER]:
            thr.append((nm, _dev_dirs(rng, N, 0.2, 0.4), np.full(N, t), None)); i += 1
    for nm, eh, tr, spec in thr:
        fams.append((nm, eh if tr is None else _compose(rng, np.exp(eh + tr[:, None] / 3.0)), spec))

    names = [f[0] for f in fams]
    F32 = np.concatenate([f[1] for f in fams], 0).astype(np.float32)
    n = F32.shape[0]
    family = np.repeat(np.arange(len(fams)), N)
    mu, lam = mu_all[:n].copy(), lam_all[:n].copy()
    ys = lu(0.05, 50.0, n) if material in ("metal", "foam", "plasticine") else np.zeros(n)
    P = TRAD_PARAMS
    if material == "sand" and not host_only:
        # away from the tr = 0 switch: a case of a plain family that lands within 10 margins of it is scaled by exp(+-2e-3)
        info = {}
        trad_update(F32, m, mu, lam, ys, alpha=alpha, info=info)
        near = (np.abs(info["tr"]) < 10 * MARGIN_TR) & (info["ehn"] + np.abs(info["tr"]) > REST_EPS) & (family < n_plain)
        F32[near] = (F32[near].astype(np.float64) * np.exp(np.where(info["tr"][near] < 0, -2e-3, 2e-3))[:, None, None]).astype(np.float32)
    if material == "plasticine":
        # away from the mu = lam = 0 switch: a plain case whose softened yield stress ends within 10 margins of zero gets 5 % more
        info = {}
        trad_update(F32, m, mu, lam, ys, hardening=P["hardening"], xi=P["xi"], softening=P["softening"], info=info)
        near = (np.abs(info["softened"]) < 10 * MARGIN_SOFTEN) & (family < n_plain)
        ys[near] *= 1.05
    # yield stresses of the threshold families, from the float64 branch variable of the fp32 input
    for i, (nm, _, spec) in enumerate(fams):
        if spec is None:
            continue
        sel = family == i
        s = np.linalg.svd(F32[sel].astype(np.float64), compute_uv=False)
        eps = np.log(np.maximum(s, 0.01))
        eh = eps - eps.mean(-1, keepdims=True)
        ehn = np.linalg.norm(eh, axis=-1)
        m2 = 2.0 * mu[sel].astype(np.float64)
        Y = m2 * ehn if material != "foam" else m2 * ehn / np.sqrt(2.0 / 3.0)      # ys at which the state sits on the surface
        kind, sg = spec
        if kind == "yield":
            ys[sel] = Y / (1.0 + sg)                 # yield function / ys - 1 = sg
        elif kind in ("ys", "ys_draw"):
            ys[sel] = sg
        else:                                        # softened ys = sg * ys:  ys (1 - sg + soft k / (2 mu)) = soft k (|eh| + 1e-6)
            k = ehn / (ehn + 1e-6)
            ys[sel] = P["softening"] * k * (ehn + 1e-6) / (1.0 - sg + P["softening"] * k / m2)
    return {"F_trial": F32, "mu": mu, "lam": lam, "ys": ys.astype(np.float32), "family": family, "names": names,
            "material": m, "alpha": alpha if material == "sand" else 0.0, "hardening": P["hardening"], "xi": P["xi"],
            "plastic_viscosity": P["plastic_viscosity"], "softening": P["softening"], "dt": P["dt"]}


def trad_reference(tab, F_trial=None, mu=None, lam=None, ys=None, info=None):
    """trad_update on a table (or on another state with the table's model scalars) -> dict of float64 fields."""
    F, S, mu_, lam_, ys_ = trad_update(tab["F_trial"] if F_trial is None else F_trial, tab["material"],
                                       tab["mu"] if mu is None else mu, tab["lam"] if lam is None else lam,
                                       tab["ys"] if ys is None else ys, tab["alpha"], tab["hardening"], tab["xi"],
                                       tab["plastic_viscosity"], tab["softening"], tab["dt"], info)
    return {"F": F, "stress": S, "mu": mu_, "lam": lam_, "ys": ys_}


def trad_scales(tab, F_trial=None, mu=None, lam=None):
    """Per-particle divisors of the error norms, from the INPUT state (the output mu, lam of dead plasticine are 0)."""
    F = np.asarray(tab["F_trial"] if F_trial is None else F_trial, np.float64)
    mu = np.asarray(tab["mu"] if mu is None else mu, np.float64)
    lam = np.asarray(tab["lam"] if lam is None else lam, np.float64)
    mod = 2.0 * mu + lam
    return {"F": _fro(F), "stress": stress_scale(F, mu, lam), "mu": mod, "lam": mod, "ys": mod}


LATTICE_H = 0.08      # spacing of the lattice the table's elements sit on (GPU scenes use the same positions)
LATTICE_0 = 0.4


def lattice(n, h=LATTICE_H, x0=LATTICE_0):
    """n points of a cubic lattice inside [x0, 2 - x0]^3 (the interior of the GPU scenes' 2 m box)."""
    side = int(np.floor((2.0 - 2.0 * x0) / h)) + 1
    assert n <= side ** 3, (n, side)
    i = np.arange(n)
    return (x0 + h * np.stack([i % side, (i // side) % side, i // (side * side)], -1)).astype(np.float32)


def cloth_table(count=64, friction_coeff=None):
    """The edge table of the cloth elements.  Returns a dict: d [n,3,3], verts [n,3,3] (fp32 positions of each element's own
    three vertices; d1 = verts[:,1] - verts[:,0], d2 = verts[:,2] - verts[:,0] exactly), R_inv [n,3], vol, mu, lam, gamma,
    kappa [n] (float32), family, names, friction_coeff."""
    rng = np.random.default_rng(77)
    N = count
    fc = friction_coeff_of(TRAD_PARAMS["friction_angle"]) if friction_coeff is None else float(friction_coeff)
    names = (["flat_exact", "general"] + [f"r22_over_{r:.0e}" for r in CLOTH_LADDER] + [f"r22_under_{r:.0e}" for r in CLOTH_LADDER]
             + [f"fric_in_{r:.0e}" for r in CLOTH_LADDER] + [f"fric_out_{r:.0e}" for r in CLOTH_LADDER] + ["gamma0", "aspect", "folded"])
    n = N * len(names)
    family = np.repeat(np.arange(len(names)), N)
    fam = lambda nm: family == names.index(nm)
    mu, lam = _lame(rng, n)
    gamma = rng.uniform(100.0, 500.0, n).astype(np.float32)
    kappa = rng.uniform(100.0, 500.0, n).astype(np.float32)
    gamma[fam("gamma0")] = 0.0
    # rest triangle D = [[a, b], [0, c]] and the in-plane deformation A (near the identity)
    a, c = rng.uniform(0.02, 0.05, n), rng.uniform(0.02, 0.05, n)
    asp = fam("aspect")
    k = asp.sum()
    c[asp] = a[asp] / np.exp(rng.uniform(0.0, np.log(100.0), k))
    swap = asp & (rng.uniform(size=n) < 0.5)
    a[swap], c[swap] = c[swap], a[swap]
    b = rng.uniform(-0.5, 0.5, n) * a
    flat = fam("flat_exact")
    A = np.tile(np.eye(2), (n, 1, 1)) + 0.15 * rng.uniform(-1, 1, (n, 2, 2))
    A[flat] = np.eye(2)
    D = np.zeros((n, 2, 2))
    D[:, 0, 0], D[:, 0, 1], D[:, 1, 1] = a, b, c
    E2 = A @ D                                   # in-plane edges, local frame
    d = np.zeros((n, 3, 3))
    d[:, :2, :2] = E2
    # the director in the local frame (normal = e_z): (shear_x, shear_y, r22), r22 and shear by family
    r22 = rng.uniform(0.7, 1.3, n)
    for r in CLOTH_LADDER:
        r22[fam(f"r22_over_{r:.0e}")] = 1.0 + r
        r22[fam(f"r22_under_{r:.0e}")] = 1.0 - r
    r22[np.abs(r22 - 1.0) < 20 * MARGIN_R22] = 1.002      # (general families: away from the switch)
    fric = np.zeros(n, bool)
    for r in CLOTH_LADDER:
        fric |= fam(f"fric_in_{r:.0e}") | fam(f"fric_out_{r:.0e}")
    r22[fric] = rng.uniform(0.5, 0.9, fric.sum())
    r22[fam("folded")] = -rng.uniform(0.1, 0.9, N)
    r22[flat] = 1.0
    # shear: as a multiple rho of the friction threshold fc fn / gamma where there is one, else a plain length
    phi = rng.uniform(0, 2 * np.pi, n)
    rho = np.where(rng.uniform(size=n) < 0.5, rng.uniform(0.1, 0.8, n), rng.uniform(1.25, 4.0, n))
    for r in CLOTH_LADDER:
        rho[fam(f"fric_in_{r:.0e}")] = 1.0 - r
        rho[fam(f"fric_out_{r:.0e}")] = 1.0 + r
    fn = kappa.astype(np.float64) * (1.0 - r22) ** 2
    has_thr = (r22 < 1.0) & (gamma > 0) & (fc > 0) & ~flat & ~fam("folded")
    sh = np.where(has_thr, rho * fc * fn / np.where(gamma > 0, gamma, 1.0), rng.uniform(0.0, 0.3, n))
    sh[flat] = np.where(np.arange(N) % 2 == 0, 0.0, rng.uniform(0.05, 0.3, N))
    d[:, 0, 2], d[:, 1, 2], d[:, 2, 2] = sh * np.cos(phi), sh * np.sin(phi), r22
    # (the in-plane QR of E2 turns the local frame about e_z: the director's shear keeps its length, r22 is unchanged)
    Rw = _rotations(rng, n)
    P = _signed_perms()
    Rw[flat] = P[np.arange(N) % len(P)]
    d = Rw @ d
    # vertices on the lattice: centroid at the lattice point, d1 and d2 re-read from the fp32 positions
    c0 = lattice(n).astype(np.float64)
    v0 = c0 - (d[:, :, 0] + d[:, :, 1]) / 3.0
    verts = np.stack([v0, v0 + d[:, :, 0], v0 + d[:, :, 1]], 1).astype(np.float32)
    d32 = d.astype(np.float32)
    d32[:, :, 0], d32[:, :, 1] = verts[:, 1] - verts[:, 0], verts[:, 2] - verts[:, 0]
    # the friction ladder is defined on the fp32 input: re-place the shear of those families from its float64 QR
    d32 = _replace_shear(d32, fric, rho, fc, gamma, kappa)
    iD = np.stack([1.0 / a, -b / (a * c), 1.0 / c], -1).astype(np.float32)
    vol = (0.25 * 1e-5 * 0.5 * a * c).astype(np.float32)
    return {"d": d32, "verts": verts, "R_inv": iD, "vol": vol, "mu": mu, "lam": lam, "gamma": gamma, "kappa": kappa,
            "family": family, "names": names, "friction_coeff": fc}


def _replace_shear(d32, sel, rho, fc, gamma, kappa):
    """Rescale the sheared part of the director of the selected elements so that ff = rho fc fn holds for the float64 QR of
    the fp32 input (two passes: the first rounding to fp32 moves r22 by an ulp, and fn with it)."""
    if fc <= 0 or not sel.any():
        return d32
    for _ in range(3):
        Q, R = qr_closed(d32[sel].astype(np.float64))
        fn = kappa[sel] * (1.0 - R[:, 2, 2]) ** 2
        want = rho[sel] * fc * fn / gamma[sel]
        have = np.sqrt(R[:, 0, 2] ** 2 + R[:, 1, 2] ** 2)
        R[:, 0, 2] *= want / have
        R[:, 1, 2] *= want / have
        d32[sel, :, 2] = np.einsum("nij,nj->ni", Q, R[:, :, 2]).astype(np.float32)
    return d32


def cloth_reference(tab, d=None, info=None):
    d_new, S, f1, f2, f3 = cloth_update(tab["d"] if d is None else d, tab["R_inv"], tab["vol"], tab["mu"], tab["lam"],
                                        tab["gamma"], tab["kappa"], tab["friction_coeff"], info)
    return {"d": d_new, "stress": S, "f1": f1, "f2": f2, "f3": f3}


def cloth_scales(tab, d=None):
    d = np.asarray(tab["d"] if d is None else d, np.float64)
    sc = stress_scale(cloth_F(d, tab["R_inv"]), tab["mu"], tab["lam"], np.asarray(tab["vol"], np.float64))
    return {"d": _fro(d), "stress": sc, "f1": sc, "f2": sc, "f3": sc}


def interleave(family):
    """A permutation that deals the families out round-robin, so that every run of 64 consecutive cases (a wavefront) mixes
    all of them: order[k] is the table index that sits at position k (families of equal size, as the tables have them)."""
    K = int(family.max()) + 1
    N = len(family) // K
    k = np.arange(len(family))
    return (k % K) * N + k // K
