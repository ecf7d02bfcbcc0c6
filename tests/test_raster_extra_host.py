"""The rasteriser's extra attribute channels without a GPU: mpmavatar_amd/csrc/raster_extra_math.hpp compiled with g++
(tests/hostraster_extra/hostraster_extra.cpp, a serial statement of both walks in the device's order) against the float64 torch
twin, forward and gradients; the measurement of G32X, the constant the device bound is built on; the composition rule the yardstick
rests on; the same loops as a stand-alone program under the sanitizers.  The cases and the yardstick: tests/raster_extra_cases.py."""
import subprocess

import numpy as np
import pytest

import raster_extra_cases as xc
import raster_grad_scenes as gs
import raster_scenes as rs
import raster_twin_torch as tt

IDS = lambda k: "-".join(map(str, k))


@pytest.fixture(scope="module")
def hx():
    return xc.host()


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------

def test_g32x_and_the_left_out_share():
    """G32X = worst relative error of the float32 twin's gradients of the combined loss against the float64 twin's over the
    committed scenes and the seeded [N, 2] table; the constant in raster_extra_cases.py is this measurement, rounded up.  It lies
    above the colour's G32, so BOUND_G is not reused.  At most 1 % of a scene's pixels carry no weight."""
    worst = 0.0
    for key in rs.COMPARED:
        c = xc.scene_case(key)
        errs = {k: gs.rel_err(c.g32[k], c.g64[k]) for k in c.g64 if np.abs(c.g64[k]).max() > 0}
        print(key, "left out %.2f %%;" % (100 * c.share), ", ".join("%s %.3g" % kv for kv in errs.items()))
        assert c.share <= gs.MAX_LEFT_OUT_SHARE
        assert "extra_attrs" in errs
        worst = max(worst, max(errs.values()))
    print("G32X measured %.4g, committed %.4g" % (worst, xc.G32X))
    assert 0.5 * xc.G32X < worst <= xc.G32X
    assert xc.BOUND_GX == 10 * xc.G32X and xc.G32X > gs.G32


def test_the_table_is_the_references_kind():
    t = xc.table(600, 2)
    assert t.dtype == np.float32 and set(np.unique(t[:, 0])) == {0.0, 1.0} and 0.3 < t[:, 0].mean() < 0.7
    assert [g.shape for g in xc.pad(xc.table(5, 8))] == [(5, 3)] * 3 and (xc.pad(xc.table(5, 8))[2][:, 2] == 0).all()


def test_the_composition_rule_in_float64():
    """One float64 render with the table's two channels and a zero third as ITS colours over a zero background, and a loss on all
    of its outputs, has the gradients the rule predicts: gradients() of a render is linear in the weights and the extras' padded
    render differs from the colour render only in colours and background.  Checked where both sides exist: the geometry gradients of
    L = sum Wx extra + sum Wa alpha from one render against the sum of an extras-only and an alpha-only render, to 1e-12 relative."""
    cam, sc, _, _ = rs.twins(*xc.OTHER_SCENE)
    n = sc["means3D"].shape[0]
    geometry = {k: v for k, v in sc.items() if k != "colors_precomp"}
    group = xc.pad(xc.table(n, 2))[0]
    h, w = cam.image_height, cam.image_width
    Wx = xc.pad(xc.weights_extra(2, h, w), axis=0)[0]
    Wa = gs.weights(h, w)[1]
    zero3, zero1 = np.zeros_like(Wx), np.zeros_like(Wa)
    render = lambda colours, bg: tt.render(cam, bg, dtype=np.float64, colors_precomp=colours, **geometry)
    whole = tt.gradients(render(group, np.zeros(3)), Wx, Wa)
    extras = tt.gradients(render(group, np.zeros(3)), Wx, zero1)
    alone = tt.gradients(render(sc["colors_precomp"], rs.BG), zero3, Wa)           # alpha does not depend on colours or background
    for k in ("means3D", "means2D", "opacities", "scales", "rotations"):
        err = np.abs(whole[k] - (extras[k] + alone[k])).max() / np.abs(whole[k]).max()
        print(k, "composition error %.3g" % err)
        assert err <= 1e-12, k
    assert np.abs(whole["colors_precomp"] - extras["colors_precomp"]).max() == 0.0


# ---- raster_extra_math.hpp on the host against the float64 twin ---------------------------------------------------------------------

def _check(hx, case, what):
    got, image, alpha, extra = xc.host_backward(hx, case)
    xc.check_forward(case, image, alpha, extra, what)
    xc.check_grads(got, case.g64, what)
    assert (extra[:, case.alpha64[0] == 0.0] == 0.0).all()                        # no background term
    return got, extra


@pytest.mark.parametrize("key", rs.COMPARED, ids=IDS)
def test_host_walks_against_float64(hx, key):
    case = xc.scene_case(key)
    got, extra = _check(hx, case, IDS(key))
    assert np.abs(case.g64["extra_attrs"]).max() > 0
    if key[0] == "front":
        assert (got["extra_attrs"][rs.n_front():] == 0).all()                      # the hidden layers: exactly zero


@pytest.mark.parametrize("E", xc.E_OTHER)
def test_host_walks_other_channel_counts(hx, E):
    case = xc.scene_case(xc.OTHER_SCENE, E)
    got, extra = _check(hx, case, f"E = {E}")
    assert extra.shape[0] == E and got["extra_attrs"].shape[1] == E and np.abs(got["extra_attrs"]).max(0).min() > 0


def test_host_walks_with_the_loss_on_the_extras_alone(hx):
    case = xc.scene_case(xc.OTHER_SCENE, xc.E_REF, ("extra",))
    got, _ = _check(hx, case, "extras alone")
    assert (got["colors_precomp"] == 0).all()


def test_three_channels_have_the_bits_of_three_colours(hx):
    """the operation order is blend()'s: a [N, 3] table blends to the very bits of the same values as colours over bg = 0"""
    case = xc.scene_case(xc.OTHER_SCENE, 3)
    as_colours = case._replace(sc=dict(case.sc, colors_precomp=case.extra))
    _, image, _, extra = xc.host_backward(hx, as_colours, bg=np.zeros(3, np.float32))
    assert np.array_equal(image, extra)


def test_channel_count_out_of_range_is_refused(hx):
    case = xc.scene_case(xc.OTHER_SCENE, 1)
    for E in (0, 9):
        bad = case._replace(extra=np.zeros((case.extra.shape[0], E), np.float32), Wx=np.zeros((E,) + case.Wx.shape[1:], np.float32))
        with pytest.raises(AssertionError):
            xc.host_backward(hx, bad)


# ---- the same loops as a stand-alone program under the sanitizers ---------------------------------------------------------------------

def test_stand_alone_program_under_sanitizers():
    """N = 0, one Gaussian, and 300 over one tile (a list longer than 256, the other tiles empty, lanes outside the image), for
    E = 1, 2, 3, 5, 8, on exactly sized buffers, as a stand-alone program built with -fsanitize=address,undefined: an index past
    a row, a plane or a table ends it with a report"""
    r = subprocess.run([xc.sanitizer_program()], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("ok") and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr
