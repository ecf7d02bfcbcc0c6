"""Every module of the appearance chain launches on the CURRENT torch stream: the shared call path (mpmavatar_amd/_call.py) is
the one place a wrong stream would come from.  One case per module, each the smallest case of the module's own tests, run once
on the default stream and once under ``torch.cuda.stream(side)``.  Every one of these paths documents the same bits from run to
run, so the outputs and, where the module is differentiable, the gradients must be ``torch.equal``."""
import numpy as np
import pytest
import torch

import binding_grad_cases as bc
import image_loss_cases as ic
import raster_scenes as rs
import shade_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    return torch.tensor(np.asarray(a), device=DEV)          # a copy: the shared cases are read-only


def _leaf(t):
    return t.detach().clone().requires_grad_(True)


def _binding():
    """the smaller binding case (`render`: 198 faces, 413 Gaussians) through set_mesh_by_verts and render_inputs"""
    from mpmavatar_amd.mesh_frames import MeshFrames
    from mpmavatar_amd.render_inputs import BoundGaussians
    c = bc.case("render")
    base = {k: _t(c[k]) for k in bc.NAMES}
    faces, binding, w = _t(c["faces"]), _t(c["binding"]), {k: _t(c["w_" + k]) for k in bc.OUTS}
    n = c["binding"].shape[0]
    dc, rest = torch.zeros(n, 1, 3, device=DEV), torch.zeros(n, 0, 3, device=DEV)

    def run():
        t = {k: _leaf(v) for k, v in base.items()}
        fr = MeshFrames(faces)
        fr.set_mesh_by_verts(t["verts"])
        args = BoundGaussians(t["_xyz"], t["_rotation"], t["_scaling"], t["_opacity"], dc, rest, binding).render_inputs(fr)
        sum((w[k] * args[k]).sum() for k in bc.OUTS).backward()
        return [args[k].detach() for k in bc.OUTS + ("means2D",)] + [t[k].grad for k in bc.NAMES]
    return run


def _image():
    """the `ragged` image case (3 x 37 x 53) through image_loss and its backward"""
    from mpmavatar_amd.image_loss import image_loss
    img, gt = (_t(a) for a in ic.case("ragged"))

    def run():
        a = _leaf(img)
        out = image_loss(a, gt, ic.LAMBDA)
        out[0].backward()
        return [t.detach() for t in out] + [a.grad]
    return run


def _raster():
    """the odd 33 x 17 scene (two tile columns with a ragged edge) through the rasteriser and its backward; the side stream gets
    a handle of its own"""
    from mpmavatar_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    cam, sc, _, _ = rs.twins("odd", 33, 17)
    base = {k: _t(np.asarray(v, np.float32)) for k, v in sc.items() if v is not None}
    st = GaussianRasterizationSettings(image_height=cam.image_height, image_width=cam.image_width, tanfovx=cam.tanfovx,
                                       tanfovy=cam.tanfovy, bg=_t(rs.BG), scale_modifier=1.0, viewmatrix=_t(cam.viewmatrix),
                                       projmatrix=_t(cam.projmatrix), sh_degree=0, campos=_t(np.asarray(cam.campos, np.float32)),
                                       prefiltered=False, debug=False)
    h, w = cam.image_height, cam.image_width
    wi = torch.linspace(-1.0, 1.0, 3 * h * w, device=DEV).reshape(3, h, w)
    wa = torch.linspace(0.5, -0.5, h * w, device=DEV).reshape(1, h, w)

    def run():
        t = {k: _leaf(v) for k, v in base.items()}
        m2 = torch.zeros_like(t["means3D"], requires_grad=True)
        image, _, _, alpha, radii, _ = GaussianRasterizer(raster_settings=st)(means2D=m2, **t)
        ((wi * image).sum() + (wa * alpha).sum()).backward()
        return [image.detach(), alpha.detach(), radii, m2.grad] + [t[k].grad for k in sorted(t)]
    return run


def _nearest():
    """1,025 source points against 300 targets: two query tiles of 256 x 4"""
    from mpmavatar_amd.geo_metrics import nearest_dist2
    g = torch.Generator().manual_seed(11)
    src, dst = torch.rand(1025, 3, generator=g).to(DEV), torch.rand(300, 3, generator=g).to(DEV)
    return lambda: list(nearest_dist2(src, dst, return_index=True))


def _shading():
    """the smallest shading case (`k4`: 53 Gaussians on 11 faces, a 3 x 4 map, degree 1) through shaded_colors and its backward"""
    from mpmavatar_amd.shading import ShadowSampler, shaded_colors
    c = sc.case("k4")
    base = {k: _t(c[k]) for k in sc.GRADS}
    binding, campos, w = _t(c["binding"]), _t(c["campos"]), _t(c["w"])
    H, W = c["shadow_map"].shape
    sampler = ShadowSampler(_t(c["face_uv"]), H, W)

    def run():
        t = {k: _leaf(v) for k, v in base.items()}
        colors = shaded_colors(t["features_dc"], t["features_rest"], 1, t["means3D"], campos, binding=binding, shadow_map=t["shadow_map"],
                               sampler=sampler)
        (w * colors).sum().backward()
        return [colors.detach()] + [t[k].grad for k in sc.GRADS]
    return run


CASES = {"mesh_frames+render_inputs": _binding, "image_loss": _image, "rasterizer": _raster, "geo_metrics": _nearest, "shading": _shading}


@pytest.mark.parametrize("module", sorted(CASES))
def test_launches_on_the_current_stream(module):
    run = CASES[module]()
    want = run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = run()
    side.synchronize()
    assert len(got) == len(want) and len(want) >= 2
    for k, (a, b) in enumerate(zip(want, got)):
        assert a is not None and b is not None and torch.equal(a, b), (module, k)
