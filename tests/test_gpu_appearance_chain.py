"""The whole appearance step on the GPU, loss to leaves, against the composite float64 twin (tests/appearance_chain_cases.py):

    MeshFrames.set_mesh_by_verts(verts + offset) -> BoundGaussians.render_inputs(extra=...) + shaded_colors (ShadowSampler)
    -> GaussianRasterizer -> picture -> torch.where(keep, picture, gt) -> image_loss(...)[0].backward()

Radii equal to the twin's; the loss within BOUND_V; the picture on the kept pixels and the gradient of EVERY leaf (vertices, the six
parameter tensors of the model, the shadow map, the five ``extra`` tensors, means2D) within BOUND_G = 10 * E2E32, both measured on the
CPU from the twin alone; exact zeros where the twin has them; the same bits from run to run and on a side stream.

The colours reach the render call in the two ways a trainer can write it.  `far`: the reference's (train_appearance.py:120-123) --
colours from ``get_xyz``, then ``render_inputs(override_color=colours, extra=...)``, so the package's own ``torch.cat`` orders the
colour rows and ``_xyz`` / the frames collect from two autograd nodes.  `close`: the example's -- ``render_inputs`` first, then
``shaded_colors(args["means3D"][:n], ...)`` in place of the bound colour rows, so ONE means3D tensor feeds the rasteriser and the
shading at once.  `sh`: ``override_color=None``, the rasteriser's own SH path.  Every figure is printed before it is asserted (-s)."""
import numpy as np
import pytest
import torch

import appearance_chain_cases as ac
import raster_scenes as rs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    return torch.tensor(np.asarray(a), device=DEV)          # a copy: the shared cases are read-only


def _step(name, private_scratch=False):
    """one forward and backward of the case on the device -> dict: loss (0-d tensor), picture, radii, grads {leaf: tensor}"""
    from mpmavatar_amd.image_loss import image_loss
    from mpmavatar_amd.mesh_frames import MeshFrames
    from mpmavatar_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    from mpmavatar_amd.render_inputs import BoundGaussians
    from mpmavatar_amd.shading import ShadowSampler
    tw = ac.twins(name)
    c, cam = tw.case, tw.case.cam
    t = {k: _t(getattr(c, k)).requires_grad_(True) for k in tw.names if k != "means2D"}
    n = c.n
    binding, campos = _t(c.binding), _t(np.asarray(cam.campos, np.float32))
    fr = MeshFrames(_t(c.faces))
    fr.set_mesh_by_verts(t["verts"] + _t(c.offset))
    bg = BoundGaussians(t["_xyz"], t["_rotation"], t["_scaling"], t["_opacity"], t["_features_dc"], t["_features_rest"], binding)
    extra = [t[k] for k in ac.EXTRA] if c.extras else None
    if not c.shaded:
        args = bg.render_inputs(fr)
        assert args["colors_precomp"] is None and args["shs"].shape == (n, ac.K, 3)
    else:
        sampler = ShadowSampler(_t(c.face_uv)[None, None], ac.MAP_H, ac.MAP_W)
        shade = lambda means: bg.shaded_colors(means, campos, c.degree, shadow_map=t["shadow_map"], sampler=sampler)
        if name == "far":
            seen = fr.get_xyz(binding, t["_xyz"])
            args = bg.render_inputs(fr, override_color=shade(seen), extra=extra)
            assert torch.equal(seen, args["means3D"][:n])                       # the shading saw the rasteriser's positions
        else:
            args = bg.render_inputs(fr, override_color=torch.zeros(n, 3, device=DEV), extra=extra)
            args["colors_precomp"] = torch.cat([shade(args["means3D"][:n]), args["colors_precomp"][n:]])
        assert args["shs"] is None and args["colors_precomp"].shape == (n + c.m, 3)
    assert args["means3D"].shape == (n + c.m, 3) and args["rotations"].shape == (n + c.m, 4)
    args["means2D"].requires_grad_(True)
    st = GaussianRasterizationSettings(image_height=cam.image_height, image_width=cam.image_width, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy,
                                       bg=_t(rs.BG), scale_modifier=1.0, viewmatrix=_t(cam.viewmatrix), projmatrix=_t(cam.projmatrix),
                                       sh_degree=c.degree, campos=campos, prefiltered=False, debug=False)
    image, _, _, alpha, radii, _ = GaussianRasterizer(raster_settings=st, private_scratch=private_scratch)(**args)
    picture = (image * alpha).clip(0.0, 1.0) if c.clipped else image
    gt = _t(tw.gt)
    loss = image_loss(torch.where(_t(tw.keep)[None], picture, gt), gt, ac.LAMBDA)[0]
    loss.backward()
    grads = {k: v.grad for k, v in t.items()}
    grads["means2D"] = args["means2D"].grad
    return {"loss": loss.detach(), "picture": picture.detach(), "radii": radii, "grads": grads}


@pytest.mark.parametrize("name", ac.CASES)
def test_against_the_twin(name):
    tw = ac.twins(name)
    c = tw.case
    out = _step(name)
    radii = out["radii"].cpu().numpy()
    loss, picture = float(out["loss"]), out["picture"].cpu().numpy().astype(np.float64)
    got = {k: (None if g is None else g.cpu().numpy()) for k, g in out["grads"].items()}
    # ---- the figures ----
    v = abs(loss - tw.loss64) / abs(tw.loss64)
    p = float(np.abs(picture - tw.picture64)[:, tw.keep].max())
    print(name, "radii equal: %s; loss %.9g (twin %.9g), relative %.3g of bound %.3g; picture on kept pixels %.3g of bound %.3g" %
          (np.array_equal(radii, tw.radii64), loss, tw.loss64, v, ac.BOUND_V, p, ac.BOUND_G))
    errs, zeros_kept = {}, {}
    for k in tw.names:
        assert got[k] is not None and got[k].shape == tw.g64[k].shape and np.isfinite(got[k]).all(), k
        top = np.abs(tw.g64[k]).max()
        errs[k] = float(np.abs(got[k] - tw.g64[k]).max() / top) if top > 0 else float(np.abs(got[k]).max())
        rows = lambda a: np.asarray(a).reshape(a.shape[0], -1)
        zero = (rows(tw.g64[k]) == 0).all(1) & (rows(tw.g32[k]) == 0).all(1)      # identically zero in both runs of the twin
        zeros_kept[k] = (int((rows(got[k])[zero] != 0).any(1).sum()), int(zero.sum()))
        print(name, "%-16s max |g - g64| / max |g64| = %.3g of bound %.3g; rows zero in the twin %d, of them non-zero here %d" %
              (k, errs[k], ac.BOUND_G, zeros_kept[k][1], zeros_kept[k][0]))
    # ---- the assertions ----
    assert np.array_equal(radii, tw.radii64)
    assert v <= ac.BOUND_V
    assert p <= ac.BOUND_G
    for k in tw.names:
        assert errs[k] <= ac.BOUND_G, (k, errs[k])
        if np.abs(tw.g64[k]).max() == 0:
            assert (got[k] == 0).all(), k
    culled = radii == 0
    assert np.array_equal(culled, tw.culled)
    for k in ac.PER_GAUSSIAN:                                         # a culled Gaussian gets nothing, through three backward passes
        assert (got[k][culled[:c.n]] == 0).all(), k
    assert (got["means2D"][culled] == 0).all()
    for k in ac.EXTRA if c.extras else ():
        assert (got[k][culled[c.n:]] == 0).all(), k
    for k in tw.names:                                                # hidden and culled Gaussians, vertices that carry only such
        assert zeros_kept[k][0] == 0, (k, zeros_kept[k])
    assert (got["means2D"][:, 2] == 0).all()


def test_same_bits_from_run_to_run_and_on_a_side_stream():
    a, b = _step("far"), _step("far")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s = _step("far", private_scratch=True)
    side.synchronize()
    for other, tag in ((b, "second run"), (s, "side stream")):
        assert torch.equal(a["loss"], other["loss"]) and torch.equal(a["picture"], other["picture"]) and torch.equal(a["radii"], other["radii"]), tag
        assert set(a["grads"]) == set(other["grads"]) == set(ac.twins("far").names)
        for k, g in a["grads"].items():
            assert g is not None and torch.isfinite(g).all() and (g != 0).any() and torch.equal(g, other["grads"][k]), (tag, k)
