"""The image loss without a GPU: mpmavatar_amd/csrc/image_loss_math.hpp compiled with g++ (tests/hostimage/hostimage.cpp, a
serial statement of forward and backward) against the reference's own float64 results (tests/golden/image_loss.npz); the
measurement of S32, the constant the bound is built on; the conditions the committed cases must meet;
torch.autograd.gradcheck of a float64 twin as an anchor independent of our derivation; known answers; and the flat-region
statement.  Every comparison prints its figures before it asserts (run with -s)."""
import numpy as np
import pytest
import torch

import image_loss_cases as ic


# ---- the yardstick and the conditions of the comparison -------------------------------------------------------------------------------

def test_s32_is_the_measurement():
    """S32 = worst error of the reference's float32 run against its float64 run over the five cases, rounded up"""
    worst = 0.0
    for name in ic.CASES:
        errs = {k: ic.rel_value(ic.ref(name, k, "32"), ic.ref(name, k)) for k in ic.value_keys(name)}
        errs["d_ssim"] = ic.rel_grad(ic.ref(name, "d_ssim", "32"), ic.ref(name, "d_ssim"))
        print(name, ", ".join("%s %.3g" % kv for kv in errs.items()))
        worst = max(worst, max(errs.values()))
    print("S32 measured %.4g, committed %.4g" % (worst, ic.S32))
    assert 0.5 * ic.S32 < worst <= ic.S32
    assert ic.BOUND == 10 * ic.S32


@pytest.mark.parametrize("name", ic.CASES)
def test_committed_cases_meet_the_conditions(name):
    """the shapes of the table; every |img - gt| exactly 0 or at least 1e-4 (sign cannot flip with rounding), with exact ties
    present; the fixture's gradient covers every pixel, so no pixel is left out of any comparison"""
    img, gt = ic.case(name)
    assert img.shape == gt.shape == ic.SHAPES[name] and img.dtype == gt.dtype == np.float32
    d = np.abs(img.astype(np.float64) - gt.astype(np.float64))
    assert ((d == 0) | (d >= ic.MIN_DIFF)).all()
    assert (d[..., :2, :3] == 0).all() and (d > 0).any()
    for tag in ("64", "32"):
        g = ic.ref(name, "d_ssim", tag)
        assert g.shape == img.shape and np.isfinite(g).all()
    assert ic.ref(name, "psnr").shape == (img.shape[0], 1)
    assert ("ssim_per_item" in ic.value_keys(name)) == (img.ndim == 4)


def test_window_table_is_the_references():
    w = np.empty(11, np.float32)
    ic.host_lib().hi_window(w.ctypes.data_as(ic.fp))
    want = ic.GOLD["window"]
    assert want.dtype == np.float32 and want.shape == (11,)
    ulps = np.abs(w.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    print("window: ulps from gaussian(11, 1.5)", ulps, "sum", w.astype(np.float64).sum())
    assert ulps.max() <= 1 and (w == w[::-1]).all()


# ---- image_loss_math.hpp on the host against the reference's float64 run ------------------------------------------------------------------

@pytest.mark.parametrize("name", ic.CASES)
def test_host_values_against_float64(name):
    img, gt = ic.case(name)
    means, maps, smap = ic.host_forward(img, gt)
    assert np.isfinite(means).all() and np.isfinite(maps).all() and np.isfinite(smap).all()
    got = ic.values_from_means(means, img.shape)
    for k in ic.value_keys(name):
        err = ic.rel_value(got[k], ic.ref(name, k))
        print(name, k, "%.3g of bound %.3g" % (err, ic.BOUND))
        assert err <= ic.BOUND, k
    quiet, none, _ = ic.host_forward(img, gt, want_maps=False)
    assert none is None and np.array_equal(quiet, means)


@pytest.mark.parametrize("name", ic.CASES)
def test_host_gradients_against_float64(name):
    img, gt = ic.case(name)
    planes = int(np.prod(img.shape[:-2]))
    _, maps, _ = ic.host_forward(img, gt)
    g_ssim = ic.host_backward(img, gt, maps, 0.0, 0.0, 1.0 / planes)
    err = ic.rel_grad(g_ssim, ic.ref(name, "d_ssim"))
    print(name, "d ssim %.3g of bound %.3g" % (err, ic.BOUND))
    assert err <= ic.BOUND
    g_loss = ic.host_backward(img, gt, maps, (1.0 - ic.LAMBDA) / planes, 0.0, -ic.LAMBDA / planes)
    err = ic.rel_grad(g_loss, ic.d_loss_64(name))
    print(name, "d loss %.3g" % err)
    assert err <= ic.BOUND
    g_mse = ic.host_backward(img, gt, maps, 0.0, 1.0 / planes, 0.0)
    want = 2.0 * (img.astype(np.float64) - gt.astype(np.float64)) / img.size
    assert ic.rel_grad(g_mse, want) <= ic.BOUND
    g_l1 = ic.host_backward(img, gt, maps, 1.0 / planes, 0.0, 0.0)
    assert ic.rel_grad(g_l1, ic.d_l1(img, gt)) <= ic.BOUND
    assert (g_l1[..., :2, :3] == 0).all()                                   # the exact ties: sign(0) = 0


# ---- anchors independent of our derivation --------------------------------------------------------------------------------------------------

def test_float64_twin_is_the_reference_and_passes_gradcheck():
    """the twin returns the fixture's float64 ssim and gradient on every case, and torch.autograd.gradcheck (finite
    differences of its own forward) accepts its gradient on `tiny`"""
    for name in ic.CASES:
        img, gt = ic.case(name)
        a = torch.tensor(img, dtype=torch.float64, requires_grad=True)
        s = ic.twin_ssim(a, torch.tensor(gt, dtype=torch.float64))
        (g,) = torch.autograd.grad(s, a)
        assert abs(float(s.detach()) - float(ic.ref(name, "ssim"))) < 1e-12
        assert ic.rel_grad(g.numpy(), ic.ref(name, "d_ssim")) < 1e-10
    img, gt = ic.case("tiny")
    a = torch.tensor(img, dtype=torch.float64, requires_grad=True)
    b = torch.tensor(gt, dtype=torch.float64)
    assert torch.autograd.gradcheck(lambda t: ic.twin_ssim(t, b), (a,), eps=1e-6, atol=1e-8, rtol=1e-5)


def test_identical_images():
    img, _ = ic.case("ragged")
    means, maps, _ = ic.host_forward(img, img)
    v = ic.values_from_means(means, img.shape)
    assert v["l1"] == 0.0 and (means[:, 1] == 0).all()
    assert abs(1.0 - v["ssim"]) <= 1e-6
    assert (ic.host_backward(img, img, maps, 1.0 / 3, 0.0, 0.0) == 0).all()   # the L1 gradient: sign(0) = 0 everywhere


def test_psnr_of_a_constant_offset_is_20_db():
    gt = np.full((3, 20, 24), 0.4, np.float32)
    img = gt + np.float32(0.1)
    means, _, _ = ic.host_forward(img, gt, want_maps=False)
    psnr = ic.values_from_means(means, img.shape)["psnr"]
    assert psnr.shape == (3, 1) and np.abs(psnr - 20.0).max() <= 1e-5


# ---- the flat-region statement: documented, not bounded -----------------------------------------------------------------------------------

def test_flat_region_is_finite_and_near_one():
    """a constant image with a 1e-3 bump: E[x^2] - mu^2 cancels in fp32, in the reference as here"""
    img, gt = ic.GOLD["flat_img"], ic.GOLD["flat_gt"]
    means, maps, smap = ic.host_forward(img, gt)
    s = float(means[0, 2])
    print("flat: host %.7f, reference fp32 %.7f, fp64 %.7f" % (s, float(ic.GOLD["flat_ssim_32"]), float(ic.GOLD["flat_ssim_64"])))
    assert np.isfinite(means).all() and np.isfinite(maps).all() and np.isfinite(smap).all()
    assert 0.9999 < s <= 1.0
