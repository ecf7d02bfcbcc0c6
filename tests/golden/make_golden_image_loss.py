"""Golden vectors for the image loss FROM THE REFERENCE ITSELF: utils/loss_utils.py and utils/image_utils.py need only
torch and are imported unchanged, by file path, on the CPU; their outputs on seeded images, in float64 and in float32, and
the gradient autograd takes of ssim pin mpmavatar_amd/csrc/image_loss_math.hpp (host build) and the kernels of
csrc/image_loss.hip.  Run in the build container (needs /root/reference):
    python tests/golden/make_golden_image_loss.py
The fixture holds inputs and results only.  The gradients of l1_loss and of the mean squared error are closed forms; the
tests compute them."""
import importlib.util
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/utils"

# name -> shape: the smallest shapes at which a tile, halo or indexing mistake shows (tests/image_loss_cases.py says which)
CASES = {"tiny": (1, 5, 7), "one_tile": (3, 16, 16), "ragged": (3, 37, 53), "batch": (2, 3, 33, 17), "wide": (1, 17, 270)}
MIN_DIFF = 1e-4     # every |img - gt| is exactly 0 or at least this: sign(img - gt) cannot flip with rounding


def load(name):
    spec = importlib.util.spec_from_file_location("reference_" + name, os.path.join(REF, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_inputs(shape, rng):
    """gt: a smooth sinusoid pattern per channel in [0.1, 0.9]; img = clip(gt + 0.15 noise, 0, 1) with a 2 x 3 corner copied
    from gt (exact L1 ties); a difference below MIN_DIFF that is not a tie is made one."""
    H, W = shape[-2:]
    planes = int(np.prod(shape[:-2]))
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    gt = np.empty((planes, H, W))
    for p in range(planes):
        fy, fx, ph = rng.uniform(0.15, 0.6), rng.uniform(0.15, 0.6), rng.uniform(0, 2 * np.pi)
        gt[p] = 0.5 + 0.4 * np.sin(fy * yy + ph) * np.cos(fx * xx - 0.5 * ph)
    gt = gt.astype(np.float32)
    img = np.clip(gt + np.float32(0.15) * rng.standard_normal(gt.shape).astype(np.float32), 0.0, 1.0).astype(np.float32)
    img[:, :2, :3] = gt[:, :2, :3]
    close = np.abs(img - gt) < MIN_DIFF
    img[close] = gt[close]
    return img.reshape(shape), gt.reshape(shape)


def run(lu, iu, img, gt, dtype):
    a = torch.tensor(img, dtype=dtype, requires_grad=True)
    b = torch.tensor(gt, dtype=dtype)
    s = lu.ssim(a, b)
    (g,) = torch.autograd.grad(s, a)
    out = dict(l1=lu.l1_loss(a, b), ssim=s, psnr=iu.psnr(a, b), d_ssim=g)
    if a.dim() == 4:
        out["ssim_per_item"] = lu.ssim(a, b, size_average=False)
    return {k: v.detach().numpy() for k, v in out.items()}


def main():
    lu, iu = load("loss_utils"), load("image_utils")
    rng = np.random.default_rng(20)
    out = {"window": lu.gaussian(11, 1.5).numpy()}
    for name, shape in CASES.items():
        img, gt = make_inputs(shape, rng)
        d = np.abs(img - gt)
        assert ((d == 0) | (d >= MIN_DIFF)).all() and (d == 0).sum() >= 6 and (d > 0).mean() > 0.8
        out[f"{name}_img"], out[f"{name}_gt"] = img, gt
        for tag, dtype in (("64", torch.float64), ("32", torch.float32)):
            for k, v in run(lu, iu, img, gt, dtype).items():
                out[f"{name}_{k}_{tag}"] = v
        print(name, shape, "l1 %.6f ssim %.6f psnr %s" % (out[f"{name}_l1_64"], out[f"{name}_ssim_64"], out[f"{name}_psnr_64"].ravel()))
    # the flat-region statement: a constant image with a 1e-3 bump, outside the bounded comparison
    flat = np.full((1, 32, 32), 0.5, np.float32)
    bump = flat.copy()
    bump[0, 12:20, 12:20] += np.float32(1e-3)
    out["flat_img"], out["flat_gt"] = bump, flat
    for tag, dtype in (("64", torch.float64), ("32", torch.float32)):
        out[f"flat_ssim_{tag}"] = lu.ssim(torch.tensor(bump, dtype=dtype), torch.tensor(flat, dtype=dtype)).numpy()
    print("flat: ssim fp32 %.7f, fp64 %.7f" % (out["flat_ssim_32"], out["flat_ssim_64"]))
    path = os.path.join(HERE, "image_loss.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
