"""Golden vectors for the forward rasteriser FROM THE REFERENCE'S OWN CAMERA AND SH FUNCTIONS (tests/golden/raster.npz).

The rasteriser itself (diff_gauss) is not vendored in the reference, so nothing here renders.  What the reference does have is
what the rasteriser is fed and one thing it computes:
  * the camera matrices: ``getWorld2View2`` / ``getProjectionMatrix`` (utils/graphics_utils.py:38-71) and the ``Camera`` class with
    its off-centre projection (scene/cameras.py:11-39);
  * SH -> RGB: ``eval_sh`` (utils/sh_utils.py:26-112), followed by the ``clamp_min(. + 0.5, 0)`` of gaussian_renderer/__init__.py:78.
The functions are cut out of the reference's files with ``ast`` at generation time (the modules themselves pull in packages that
are not needed here) and executed unchanged; this script contains none of their text.  Data only: inputs and expected outputs.
    python tests/golden/make_golden_raster.py        (build container: needs /root/reference)"""
import ast
import math
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
H, W = 40, 56


def cut(path, names, ns):
    """exec the top-level functions / classes / assignments called `names` of the reference file `path` into ns"""
    src = open(path).read()
    for node in ast.parse(src).body:
        name = getattr(node, "name", None)
        if name is None and isinstance(node, ast.Assign) and isinstance(node.targets[0], ast.Name):
            name = node.targets[0].id
        if name in names:
            exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    missing = [n for n in names if n not in ns]
    assert not missing, missing
    return ns


def rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def main():
    rng = np.random.default_rng(41)
    gu = cut(os.path.join(REF, "utils", "graphics_utils.py"), ["getWorld2View2", "getProjectionMatrix"],
             {"np": np, "torch": torch, "math": math})
    cams = cut(os.path.join(REF, "scene", "cameras.py"), ["fov2focal", "focal2fov", "Camera"],
               {"torch": torch, "math": math, "nn": torch.nn})
    sh = cut(os.path.join(REF, "utils", "sh_utils.py"), ["C0", "C1", "C2", "C3", "C4", "eval_sh"], {"torch": torch})
    out = {"image_height": np.int32(H), "image_width": np.int32(W)}

    # camera 0: centred principal point, the Inria construction the reference's graphics_utils serve
    R, t = rotation(rng), rng.normal(0, 0.3, 3)
    fovx = 2 * math.atan(0.45)
    fovy = 2 * math.atan(0.45 * H / W)
    wvt = torch.tensor(gu["getWorld2View2"](R, t)).transpose(0, 1)
    proj = gu["getProjectionMatrix"](znear=0.01, zfar=100.0, fovX=fovx, fovY=fovy).transpose(0, 1)
    full = wvt.unsqueeze(0).bmm(proj.unsqueeze(0)).squeeze(0)
    out.update(cam0_world_view_transform=wvt.contiguous().numpy(), cam0_full_proj_transform=full.numpy(),
               cam0_camera_center=wvt.inverse()[3, :3].numpy(), cam0_tanfovx=math.tan(fovx * 0.5), cam0_tanfovy=math.tan(fovy * 0.5))

    # camera 1: scene/cameras.py with an off-centre principal point
    R, t = rotation(rng), rng.normal(0, 0.3, 3)
    w2c = np.eye(4)
    w2c[:3, :3], w2c[:3, 3] = R, t
    k = [[70.0, 0.0, 0.5 * W + 5.5], [0.0, 66.0, 0.5 * H - 3.25], [0.0, 0.0, 1.0]]
    cam = cams["Camera"](1, W, H, k, w2c.tolist(), near=1, far=10, data_device="cpu")
    out.update(cam1_world_view_transform=cam.world_view_transform.contiguous().numpy(),
               cam1_full_proj_transform=cam.full_proj_transform.contiguous().numpy(), cam1_camera_center=cam.camera_center.numpy(),
               cam1_tanfovx=math.tan(cam.FoVx * 0.5), cam1_tanfovy=math.tan(cam.FoVy * 0.5), cam1_w2c=w2c, cam1_k=np.array(k))

    # SH -> RGB, degrees 0-3, evaluated by the reference in float64 on float32 inputs
    n = 300
    coeffs = rng.normal(0, 0.6, (n, 16, 3)).astype(np.float32)          # coefficient-major, as GaussianModel.get_features
    pos = rng.normal(0, 2.0, (n, 3)).astype(np.float32)
    campos = out["cam0_camera_center"].astype(np.float32)
    d = torch.from_numpy(pos).double() - torch.from_numpy(campos).double()
    d = d / d.norm(dim=1, keepdim=True)
    shs_view = torch.from_numpy(coeffs).double().transpose(1, 2)        # [n, 3, 16] (gaussian_renderer/__init__.py:74)
    out.update(sh_coeffs=coeffs, sh_positions=pos, sh_campos=campos)
    for deg in range(4):
        out[f"sh_colors_deg{deg}"] = torch.clamp_min(sh["eval_sh"](deg, shs_view, d) + 0.5, 0.0).numpy()
    np.savez_compressed(os.path.join(HERE, "raster.npz"), **out)
    print("raster.npz:", {k: getattr(v, "shape", v) for k, v in out.items()})


if __name__ == "__main__":
    main()
