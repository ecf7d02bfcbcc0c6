"""Cases, yardstick and helpers shared by tests/test_image_loss_host.py and tests/test_gpu_image_loss.py.  The cases come from
tests/golden/image_loss.npz (tests/golden/make_golden_image_loss.py: the reference's own utils/loss_utils.py and
utils/image_utils.py on the CPU, in float64 and in float32); nothing here modifies them.  Test infrastructure only.

  case       shape         what it catches
  tiny       1x5x7         image smaller than the window and the tile: every tap hits padding
  one_tile   3x16x16       exactly one tile per plane, no ragged edge
  ragged     3x37x53       3 x 4 tiles, ragged in both directions, halos that cross tile edges
  batch      2x3x33x17     plane indexing, per-item size_average=False, 4-D psnr
  wide       1x17x270      more than 16 tiles in a row, width beyond 256
"""
import ctypes as C
import os

import numpy as np

import hostbuild

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = np.load(os.path.join(HERE, "golden", "image_loss.npz"))
CASES = ("tiny", "one_tile", "ragged", "batch", "wide")
SHAPES = {"tiny": (1, 5, 7), "one_tile": (3, 16, 16), "ragged": (3, 37, 53), "batch": (2, 3, 33, 17), "wide": (1, 17, 270)}
VALUES = ("l1", "ssim", "psnr", "ssim_per_item")
MIN_DIFF = 1e-4            # every |img - gt| of the cases is exactly 0 or at least this
LAMBDA = 0.2               # opt.lambda_dssim of the reference's arguments

# Measured on the CPU over the five cases (tests/test_image_loss_host.py::test_s32_is_the_measurement asserts it): S32 = the
# worst error of the reference's OWN float32 run against its own float64 run -- relative for the values (l1, ssim, psnr),
# max |g32 - g64| / max |g64| for d ssim / d img.  Our code must lie within BOUND = 10 * S32 of the float64 run: the factor
# covers a different summation order (a separable window, FMAs, fp64 tile sums), the project's margin for that.
S32 = 6.6e-6   # measured 6.594e-6 (d ssim / d img of `batch`); the other gradients 0.7e-6 .. 3.1e-6, every value below 1.2e-7
BOUND = 10 * S32


def case(name):
    """(img, gt) float32, read-only"""
    img, gt = GOLD[f"{name}_img"], GOLD[f"{name}_gt"]
    img.setflags(write=False)
    gt.setflags(write=False)
    return img, gt


def ref(name, key, tag="64"):
    return GOLD[f"{name}_{key}_{tag}"]


def value_keys(name):
    return [k for k in VALUES if f"{name}_{k}_64" in GOLD.files]


def rel_value(got, want):
    """worst relative error over the elements of a value"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.max(np.abs(got - want) / np.abs(want)))


def rel_grad(g, g64):
    """max |g - g64| / max |g64| over EVERY pixel"""
    g, g64 = np.asarray(g, np.float64), np.asarray(g64, np.float64)
    assert g.shape == g64.shape, (g.shape, g64.shape)
    return float(np.abs(g - g64).max() / np.abs(g64).max())


def d_l1(img, gt):
    """d mean |img - gt| / d img in float64: sign / n, sign(0) = 0 (exact: the differences are 0 or >= MIN_DIFF)"""
    return np.sign(img.astype(np.float64) - gt.astype(np.float64)) / img.size


def loss_value_64(name, lam=LAMBDA):
    return (1.0 - lam) * float(ref(name, "l1")) + lam * (1.0 - float(ref(name, "ssim")))


def d_loss_64(name, lam=LAMBDA):
    """gradient of (1 - lam) l1 + lam (1 - ssim) from the fixture's float64 d ssim / d img and the closed form of l1"""
    img, gt = case(name)
    return (1.0 - lam) * d_l1(img, gt) - lam * ref(name, "d_ssim")


# ---- the host build of image_loss_math.hpp ------------------------------------------------------------------------------

fp = C.POINTER(C.c_float)


def host_lib():
    return hostbuild.host_lib("hostimage")


def _p(a):
    return None if a is None else a.ctypes.data_as(fp)


def host_forward(img, gt, want_maps=True):
    """-> (means [planes, 3]: mean |d|, mean d^2, mean ssim map; maps [planes, 3, H, W] or None; ssim map [planes, H, W])"""
    H, W = img.shape[-2:]
    a, b = (np.ascontiguousarray(t, np.float32).reshape(-1, H, W) for t in (img, gt))
    planes = a.shape[0]
    maps = np.full((planes, 3, H, W), np.nan, np.float32) if want_maps else None
    smap, means = np.full((planes, H, W), np.nan, np.float32), np.full((planes, 3), np.nan, np.float32)
    host_lib().hi_forward(_p(a), _p(b), planes, H, W, _p(maps), _p(smap), _p(means))
    return means, maps, smap


def host_backward(img, gt, maps, g_l1, g_mse, g_ssim):
    """-> d_img with the shape of img; g_* are per-plane upstream gradients"""
    H, W = img.shape[-2:]
    a, b = (np.ascontiguousarray(t, np.float32).reshape(-1, H, W) for t in (img, gt))
    planes = a.shape[0]
    g = [np.ascontiguousarray(np.broadcast_to(np.float32(v), (planes,))) for v in (g_l1, g_mse, g_ssim)]
    out = np.full(a.shape, np.nan, np.float32)
    host_lib().hi_backward(_p(a), _p(b), planes, H, W, _p(maps), _p(g[0]), _p(g[1]), _p(g[2]), _p(out))
    return out.reshape(img.shape)


def values_from_means(means, shape):
    """the reference's l1, ssim, psnr (and per-item ssim of a 4-D input) from per-plane means, in float64"""
    m = np.asarray(means, np.float64).reshape(tuple(shape[:-2]) + (3,))
    out = {"l1": m[..., 0].mean(), "ssim": m[..., 2].mean()}
    mse = m[..., 1] if len(shape) == 3 else m[..., 1].mean(1)
    with np.errstate(divide="ignore"):
        out["psnr"] = (20 * np.log10(1.0 / np.sqrt(mse)))[:, None]
    if len(shape) == 4:
        out["ssim_per_item"] = m[..., 2].mean(1)
    return out


# ---- a float64 torch twin, for gradcheck and for measuring on inputs the fixture does not hold ----------------------------

def twin_ssim(img, gt):
    """A restatement of the reference's ssim (size_average=True) in torch, any dtype: the 11 x 11 window as one grouped conv2d
    with zero padding of 5, variances as E[x^2] - mu^2."""
    import math

    import torch
    import torch.nn.functional as F
    g = torch.tensor([math.exp(-(i - 5) ** 2 / (2 * 1.5 ** 2)) for i in range(11)], dtype=torch.float32)
    g = g / g.sum()                                   # the reference builds its window in float32 whatever the images are
    a, b = (t if t.dim() == 4 else t[None] for t in (img, gt))
    ch = a.shape[1]
    w = (g[:, None] * g[None, :]).to(img.dtype).expand(ch, 1, 11, 11).contiguous()
    conv = lambda t: F.conv2d(t, w, padding=5, groups=ch)
    mu1, mu2 = conv(a), conv(b)
    s1, s2, s12 = conv(a * a) - mu1 * mu1, conv(b * b) - mu2 * mu2, conv(a * b) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return (((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))).mean()
