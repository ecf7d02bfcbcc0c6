"""The whole appearance step without a GPU: the composite twin of tests/appearance_chain_cases.py (binding -> shading -> cat with the
extra rows -> rasteriser -> picture -> L1 + SSIM loss, in float64 and in float32) measured against itself.  E2E32 and V32, the
constants the GPU test's bounds are built on; the conditions every case must meet; a central-difference check that the composite
really is the derivative of its own loss; and the three seams between the modules shown to move the gradients far above the bound,
so that the GPU comparison would notice them.  Every figure is printed before it is asserted (run with -s)."""
import numpy as np
import pytest
import torch

import appearance_chain_cases as ac
import binding_grad_cases as bc


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------

def test_e2e32_is_the_measurement():
    worst_g = worst_v = 0.0
    for name in ac.CASES:
        t = ac.twins(name)
        errs = {k: ac.rel(t.g32[k], t.g64[k]) for k in t.names}
        v = abs(t.loss32 - t.loss64) / abs(t.loss64)
        print(name, "loss %.9g, float32 off by %.3g relative;" % (t.loss64, v), ", ".join("%s %.3g" % kv for kv in errs.items()))
        worst_g, worst_v = max(worst_g, max(errs.values())), max(worst_v, v)
    print("E2E32 measured %.4g, committed %.4g; V32 measured %.4g, committed %.4g" % (worst_g, ac.E2E32, worst_v, ac.V32))
    assert 0.5 * ac.E2E32 < worst_g <= ac.E2E32
    assert 0.5 * ac.V32 < worst_v <= ac.V32
    assert ac.BOUND_G == 10 * ac.E2E32 and ac.BOUND_V == 10 * max(ac.V32, 2.0 ** -24) and ac.MAX_LEFT_OUT_SHARE == 0.01


# ---- the conditions of the comparison ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ac.CASES)
def test_cases_meet_the_conditions(name):
    t = ac.twins(name)
    c = t.case
    h, w = c.cam.image_height, c.cam.image_width
    print(name, "%d x %d, %d of %d visible, %d culled, %d of %d bound rows with a zero gradient row, longest tile list %d, left out "
          "%.3f %% (%d pixels)" % (h, w, t.n_visible, c.n + c.m, int(t.culled.sum()), int(t.hidden.sum()), c.n, t.max_tile_entries,
                                   100 * t.left_out, int((~t.keep).sum())))
    print(name, "margins: quaternion branch %.3g, rasteriser clamps %.3g, shading's SH clamp %.3g; picture in [%.4g, %.4g]" %
          (t.quat_margin, t.clamp_margin, t.sh_margin, t.picture64.min(), t.picture64.max()))
    assert t.left_out <= ac.MAX_LEFT_OUT_SHARE and t.keep.shape == (h, w) and t.gt.shape == (3, h, w) and t.gt.dtype == np.float32
    assert np.array_equal(t.radii64, t.radii32) and t.radii64.shape == (c.n + c.m,)
    assert t.quat_margin >= bc.MIN_MARGIN
    assert t.clamp_margin >= ac.CLAMP_MARGIN and t.sh_margin >= ac.CLAMP_MARGIN
    assert t.max_tile_entries > 256                                   # more than one batch of the render kernel
    assert (h % 16 != 0 or w % 16 != 0) and (h > 16 or w > 16)
    assert set(t.names) == set(t.g64) == set(t.g32) and all(np.isfinite(g).all() for g in t.g64.values())
    assert all(np.abs(t.g64[k]).max() > 0 for k in t.names)           # every leaf is reached
    assert (t.g64["means2D"][:, 2] == 0).all()
    used = (c.degree + 1) ** 2
    assert (t.g64["_features_rest"][:, used - 1:] == 0).all() and (t.g64["_features_rest"][:, :used - 1] != 0).any()
    for k in ac.PER_GAUSSIAN + ("means2D",):                          # a culled Gaussian gets nothing
        assert (t.g64[k][:c.n][t.culled[:c.n]] == 0).all(), k
    if name == "close":
        assert t.culled.any() and not t.culled.all()
        assert c.n / 4 <= t.hidden.sum() < c.n
        assert c.clipped and (t.picture64 >= 0).all() and (t.picture64 <= 1).all()
    if name == "far":
        assert not t.culled.any()
    if name == "sh":
        assert not c.shaded and not c.extras and c.degree == 2


# ---- the composite is the derivative of its own loss ---------------------------------------------------------------------------------

FD_STEP = 1e-7


def test_composite_against_central_differences():
    """`far` (every leaf there is): the float64 loss at leaves +- FD_STEP * d for three seeded normal directions d over ALL leaves
    at once (the NDC leaf apart: it has no value to move) against the autograd directional derivative, to 1e-6 relative.  The step
    is 1e-7: at 1e-6 two Gaussians change places in the depth order.  At 1e-7 nothing discrete moves -- radii, tile rectangles and
    depth order are compared -- and on the kept pixels no decision is within reach: their margins are 1e-4 relative, the step moves
    a pixel centre by 1e-5 of a pixel at most.  Observed agreement: 2.6e-9, 6.9e-9, 3.2e-9."""
    t = ac.twins("far")
    c = t.case
    names = [k for k in t.names if k != "means2D"]
    base = {k: np.asarray(getattr(c, k), np.float64) for k in names}

    def loss_at(values):
        with torch.no_grad():
            f = ac.forward(c, ac.leaves_of(c, torch.float64, values))
            return float(ac.loss_of(f.picture, t.gt, t.keep)), f.r.base

    l0, b0 = loss_at(base)
    assert l0 == t.loss64
    rng = np.random.default_rng(7)
    for k in range(3):
        d = {n: rng.normal(size=base[n].shape) for n in names}
        want = sum(float((t.g64[n] * d[n]).sum()) for n in names)
        (up, bu), (down, bd) = (loss_at({n: base[n] + s * FD_STEP * d[n] for n in names}) for s in (1.0, -1.0))
        for b in (bu, bd):
            assert np.array_equal(b.radii, b0.radii) and np.array_equal(b.order, b0.order) and np.array_equal(b.splats.rect, b0.splats.rect)
        fd = (up - down) / (2 * FD_STEP)
        print("direction %d: autograd %.12g, central difference %.12g, relative %.3g" % (k, want, fd, abs(fd - want) / abs(want)))
        assert abs(fd - want) <= 1e-6 * abs(want)


# ---- the seams are visible above the bound ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seam", ["drop_shading_share", "extras_first", "xyzw"])
def test_seams_are_visible_above_the_bound(seam):
    """float64, twin only, on `far`: the shading's share of means3D dropped; the extra rows of the geometry put in front of the
    bound rows while the colours stay as torch.cat leaves them; the rotations handed to the rasteriser as XYZW.  Each moves some
    leaf's gradient by more than 100 * BOUND_G = 6.0e-3.  Observed, worst leaf: 0.058 (_xyz; verts 0.031), 2.9 (_features_rest), 1.15 (_features_rest)."""
    t = ac.twins("far")
    c = t.case
    leaves = ac.leaves_of(c, torch.float64)
    f = ac.forward(c, leaves, torch.float64, **{seam: True})
    g = ac.gradients(ac.loss_of(f.picture, t.gt, t.keep), leaves, f.r, t.names)
    if seam == "extras_first":                                        # the NDC leaf follows the geometry's rows
        g["means2D"] = np.concatenate([g["means2D"][c.m:], g["means2D"][:c.m]])
    moved = {k: float(np.abs(g[k] - t.g64[k]).max() / np.abs(t.g64[k]).max()) for k in t.names}
    print(seam, ", ".join("%s %.3g" % kv for kv in moved.items()), "; needed %.3g" % (100 * ac.BOUND_G))
    assert max(moved.values()) > 100 * ac.BOUND_G
    if seam == "drop_shading_share":                                  # it is the geometry that loses a share, not the colours' own leaves
        assert moved["verts"] > 100 * ac.BOUND_G and moved["_xyz"] > 100 * ac.BOUND_G
