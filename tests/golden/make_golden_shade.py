"""Golden vectors for the colour path of the appearance loop FROM THE REFERENCE'S OWN FUNCTIONS (tests/golden/shade.npz).

What train_appearance.py:120-123 computes per iteration,

    shadow = F.grid_sample(shadow_map, uv_coord, mode='bilinear', align_corners=False).squeeze()[..., None][binding]
    colors = shadow * convert_SH(get_features, cam, gaussians, get_xyz)

with ``convert_SH`` (train_appearance.py:31-47) and ``eval_sh`` (utils/sh_utils.py:26-112) cut out of the reference's files with
``ast`` at generation time and executed unchanged on a ``SimpleNamespace`` camera and model, and torch's own ``F.grid_sample``; this
script contains none of their text.  Evaluated in float64 on the float32 inputs of the `main` case of tests/shade_cases.py, at the
active degrees 0..3: the colours and the four gradients of sum(w * colors).  Data only: inputs and expected outputs.  The gradient
of features_rest is stored for the coefficients in use (above the active degree the reference gives exact zeros, which is asserted
here before they are dropped) and for every third Gaussian (``rest_stride``): float64 noise does not compress, and the file has to
stay under 200 KB.  Every other tensor is stored in full.
    python tests/golden/make_golden_shade.py        (needs the reference checkout that make_golden_raster.py names)"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import shade_cases as sc  # noqa: E402
from make_golden_raster import REF, cut  # noqa: E402


def main():
    sh = cut(os.path.join(REF, "utils", "sh_utils.py"), ["C0", "C1", "C2", "C3", "C4", "eval_sh"], {"torch": torch})
    ns = cut(os.path.join(REF, "train_appearance.py"), ["convert_SH"], {"torch": torch, "eval_sh": sh["eval_sh"], "MeshGaussianModel": object})
    c = sc.case("main")
    out = {k: np.asarray(v) for k, v in c.items()}
    K = 1 + c["features_rest"].shape[1]
    f64 = lambda k: torch.tensor(c[k], dtype=torch.float64)
    binding = torch.from_numpy(c["binding"].astype(np.int64))
    uv_coord = f64("face_uv")[None, None]                                     # [1, 1, F, 2], scene/mesh_gaussian_model.py:109-111
    cam = SimpleNamespace(camera_center=f64("campos"))
    out["rest_stride"] = np.int32(3)
    for deg in range(4):
        dc, rest, means, smap = [f64(k).requires_grad_(True) for k in ("features_dc", "features_rest", "means3D", "shadow_map")]
        pc = SimpleNamespace(max_sh_degree=int(round(K ** 0.5)) - 1, active_sh_degree=deg)
        shadow = F.grid_sample(smap[None, None], uv_coord, mode="bilinear", align_corners=False).squeeze()[..., None][binding]
        colors = shadow * ns["convert_SH"](torch.cat((dc, rest), dim=1), cam, pc, means)
        leaves = [dc, rest, means, smap]
        grads = torch.autograd.grad((f64("w") * colors).sum(), leaves, allow_unused=True)      # degree 0 does not read means3D
        grads = [torch.zeros_like(t) if g is None else g for t, g in zip(leaves, grads)]
        used = (deg + 1) ** 2
        assert (grads[1][:, used - 1:] == 0).all()
        out[f"deg{deg}_colors"] = colors.detach().numpy()
        out[f"deg{deg}_d_features_dc"] = grads[0].numpy()
        out[f"deg{deg}_d_features_rest_used"] = grads[1][::3, :used - 1].numpy()
        out[f"deg{deg}_d_means3D"] = grads[2].numpy()
        out[f"deg{deg}_d_shadow_map"] = grads[3].numpy()
    path = os.path.join(HERE, "shade.npz")
    np.savez_compressed(path, **out)
    print("shade.npz: %d bytes" % os.path.getsize(path), {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
