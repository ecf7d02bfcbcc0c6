"""The colour path of the appearance loop on the GPU: mpmavatar_amd.shading.shaded_colors / BoundGaussians.shaded_colors under torch
autograd (csrc/shade.hip) against the float64 twin (tests/shade_twin_torch.py) within BOUND = 10 * S32 (tests/shade_cases.py, measured
on the CPU), and the properties the path promises: the NULL forms, exact zeros, the same bits on every run, the graph rules, the sum
of two gradients on means3D, and the example training colours too.  Every comparison prints its figures before it asserts (-s)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import binding_grad_cases as bc
import binding_twin_torch as btw
import shade_cases as sc
import shade_twin_torch as tw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAIRS = [(name, deg) for name in sc.CASES for deg in sc.DEGREES[name]]


def _leaves(c, grad=sc.GRADS):
    return {k: torch.tensor(np.asarray(c[k]), device=DEV).requires_grad_(k in grad) for k in sc.GRADS}


def _sampler(c):
    from mpmavatar_amd.shading import ShadowSampler
    H, W = c["shadow_map"].shape
    return ShadowSampler(torch.tensor(c["face_uv"], device=DEV)[None, None], H, W)


def _run(c, deg, grad=sc.GRADS, features=True, shadow=True, backward=True):
    """-> (dict over TENSORS of numpy arrays, None where a leaf got no gradient; the colours tensor)"""
    from mpmavatar_amd.shading import shaded_colors
    t = _leaves(c, grad)
    colors = shaded_colors(t["features_dc"] if features else None, t["features_rest"] if features else None, deg, t["means3D"],
                           torch.tensor(c["campos"], device=DEV), binding=torch.tensor(c["binding"], device=DEV),
                           shadow_map=t["shadow_map"] if shadow else None, sampler=_sampler(c) if shadow else None)
    if backward:
        (torch.tensor(c["w"], device=DEV) * colors).sum().backward()
    out = {k: (None if v.grad is None else v.grad.cpu().numpy()) for k, v in t.items()}
    out["colors"] = colors.detach().cpu().numpy()
    return out, colors


def _assert_within_bound(got, want, tag):
    for k in sc.TENSORS:
        if want[k] is None:
            assert got[k] is None, (tag, k)
            continue
        err = sc.rel(got[k], want[k])
        print(tag, k, "%.3g of bound %.3g" % (err, sc.BOUND))
        assert np.isfinite(got[k]).all() and err <= sc.BOUND, (tag, k, err)


# ---- 1. every case and degree against the twin ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,deg", PAIRS)
def test_against_the_twin(name, deg):
    c = sc.case(name)
    got, colors = _run(c, deg)
    assert colors.grad_fn is not None and colors.shape == (c["binding"].shape[0], 3)
    _assert_within_bound(got, sc.t64(name, deg), f"{name} degree {deg}")
    quiet, colors0 = _run(c, deg, grad=(), backward=False)                       # the same launch, the same bits, no graph
    assert colors0.grad_fn is None and np.array_equal(quiet["colors"], got["colors"])


def test_map_shapes_and_the_model_method():
    """[H, W], [1, H, W] and [1, 1, H, W] maps; BoundGaussians.shaded_colors uses the model's own tensors: the same bits"""
    from mpmavatar_amd.render_inputs import BoundGaussians
    from mpmavatar_amd.shading import shaded_colors
    c = sc.case("main")
    want, _ = _run(c, 3)
    n = c["binding"].shape[0]
    sampler, campos = _sampler(c), torch.tensor(c["campos"], device=DEV)
    for lead in ((), (1,), (1, 1)):
        t = _leaves(c)
        smap = t["shadow_map"].detach().reshape(*lead, 5, 7).requires_grad_(True)
        colors = shaded_colors(t["features_dc"], t["features_rest"], 3, t["means3D"], campos, binding=torch.tensor(c["binding"], device=DEV),
                               shadow_map=smap, sampler=sampler)
        (torch.tensor(c["w"], device=DEV) * colors).sum().backward()
        assert smap.grad.shape == smap.shape and np.array_equal(smap.grad.reshape(5, 7).cpu().numpy(), want["shadow_map"])
    t = _leaves(c)
    z = lambda w: torch.zeros(n, w, device=DEV)
    bg = BoundGaussians(z(3), z(4), z(3), z(1), t["features_dc"], t["features_rest"], torch.tensor(c["binding"], device=DEV))
    colors = bg.shaded_colors(t["means3D"], campos, 3, shadow_map=t["shadow_map"], sampler=sampler)
    (torch.tensor(c["w"], device=DEV) * colors).sum().backward()
    assert bg._gtable._t is not None                                                # the model's own face -> Gaussian table
    for k in sc.GRADS:
        assert np.array_equal(t[k].grad.cpu().numpy(), want[k]), k
    assert np.array_equal(colors.detach().cpu().numpy(), want["colors"])


# ---- 2. the NULL forms --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("features,shadow", [(True, False), (False, True)], ids=["no_shadow_map", "no_features"])
def test_null_forms(features, shadow):
    c = sc.case("main")
    grad = tuple(k for k in sc.GRADS if (shadow if k == "shadow_map" else features))
    got, _ = _run(c, 3, grad=grad, features=features, shadow=shadow)
    _assert_within_bound(got, sc.twin(c, 3, features=features, shadow=shadow), "no shadow map" if features else "no features")
    from mpmavatar_amd.shading import shaded_colors
    with pytest.raises(RuntimeError):
        shaded_colors(None, None, 0, None, None)


# ---- 3. exact zeros -----------------------------------------------------------------------------------------------------------------

def test_exact_zeros():
    c = sc.case("main")
    H, W = c["shadow_map"].shape
    sampler = _sampler(c)
    untapped = (np.diff(sampler.texel_start.cpu().numpy()) == 0)
    start, items = sc.brute_force_texel_table(c["face_uv"], H, W)
    assert np.array_equal(sampler.texel_start.cpu().numpy(), start) and np.array_equal(sampler.texel_items.cpu().numpy(), items)
    on_outside = c["binding"] == 4
    assert untapped.any() and on_outside.any()
    for deg in range(4):
        r, used = _run(c, deg)[0], (deg + 1) ** 2
        assert (r["shadow_map"].reshape(-1)[untapped] == 0).all() and (r["shadow_map"].reshape(-1)[~untapped] != 0).any()
        assert (r["features_rest"][:, used - 1:] == 0).all() and (used == 1 or (r["features_rest"][:, :used - 1] != 0).any())
        assert (r["colors"][on_outside] == 0).all() and (r["features_dc"][on_outside] == 0).all()
        assert (r["means3D"] == 0).all() == (deg == 0)
    # the face without a Gaussian contributes nothing: wherever its uv lies, every output is the same
    base, moved = _run(c, 3)[0], dict(c)
    moved["face_uv"] = c["face_uv"].copy()
    moved["face_uv"][0] = (-0.35, 0.45)
    again = _run(moved, 3)[0]
    for k in sc.TENSORS:
        assert np.array_equal(again[k], base[k]), k
    # n = 0: an empty result, and zeros for the whole map
    from mpmavatar_amd.shading import shaded_colors
    smap = torch.tensor(c["shadow_map"], device=DEV).requires_grad_(True)
    e = lambda *s: torch.zeros(0, *s, device=DEV)
    colors = shaded_colors(e(1, 3), e(15, 3), 3, e(3), torch.tensor(c["campos"], device=DEV), binding=torch.zeros(0, dtype=torch.int32, device=DEV),
                           shadow_map=smap, sampler=sampler)
    assert colors.shape == (0, 3)
    colors.sum().backward()
    assert smap.grad.shape == (H, W) and (smap.grad == 0).all()


# ---- 4. determinism ---------------------------------------------------------------------------------------------------------------

def test_two_runs_give_the_same_bits():
    """n = 20,000 on 8,000 faces and an 8 x 8 map: a texel's list has hundreds of taps, a face's segment several Gaussians"""
    from mpmavatar_amd.shading import ShadowSampler, shaded_colors
    n, n_f = 20000, 8000
    rng = np.random.default_rng(11)
    f32 = lambda a: torch.tensor(a.astype(np.float32), device=DEV)
    sampler = ShadowSampler(f32(rng.uniform(-1.05, 1.05, (n_f, 2))), 8, 8)
    binding = torch.tensor(rng.integers(0, n_f, n).astype(np.int32), device=DEV)
    per_texel, per_face = np.diff(sampler.texel_start.cpu().numpy()), np.bincount(binding.cpu().numpy(), minlength=n_f)
    assert per_texel.min() >= 200 and per_face.max() >= 5
    data = [f32(rng.normal(0, 0.5, (n, 1, 3))), f32(rng.normal(0, 0.3, (n, 15, 3))), f32(rng.normal(0, 1.0, (n, 3))), f32(rng.uniform(0.2, 1, (8, 8)))]
    campos, w = f32(np.array([0.2, -0.1, 4.0])), f32(rng.normal(size=(n, 3)))

    def once():
        dc, rest, means, smap = [t.clone().requires_grad_(True) for t in data]
        colors = shaded_colors(dc, rest, 3, means, campos, binding=binding, shadow_map=smap, sampler=sampler)
        (w * colors).sum().backward()
        return [colors.detach(), dc.grad, rest.grad, means.grad, smap.grad]

    a, b = once(), once()
    for x, y in zip(a, b):
        assert torch.isfinite(x).all() and (x != 0).any() and torch.equal(x, y)
    # and the map's gradient is the twin's, in float64 on the same inputs
    dc, rest, means, smap = [t.detach().cpu().double() for t in data]
    smap.requires_grad_(True)
    ref = tw.shaded(3, dc, rest, means, campos.cpu().double(), smap, sampler.face_uv.cpu().double(), binding.cpu().long())
    g, = torch.autograd.grad((w.cpu().double() * ref).sum(), smap)
    err = sc.rel(a[4].cpu().numpy(), g.numpy())
    print("d shadow_map at n = 20,000: %.3g of bound %.3g" % (err, sc.BOUND))
    assert err <= sc.BOUND


# ---- 5. the graph rules -------------------------------------------------------------------------------------------------------------

def test_graph_rules():
    c = sc.case("main")
    with torch.no_grad():
        _, colors = _run(c, 3, backward=False)
    assert colors.grad_fn is None and not colors.requires_grad
    _, colors = _run(c, 3, grad=(), backward=False)
    assert colors.grad_fn is None and not colors.requires_grad
    want = sc.t64("main", 3)
    for k in sc.GRADS:                                                           # one leaf at a time: None for the others
        got, colors = _run(c, 3, grad=(k,))
        assert colors.grad_fn is not None
        assert all(got[o] is None for o in sc.GRADS if o != k)
        err = sc.rel(got[k], want[k])
        print(k, "alone %.3g of bound %.3g" % (err, sc.BOUND))
        assert err <= sc.BOUND
    # an output that takes no part in the loss: no upstream gradient, no launch, no gradients
    t = _leaves(c)
    from mpmavatar_amd.shading import shaded_colors
    colors = shaded_colors(t["features_dc"], t["features_rest"], 3, t["means3D"], torch.tensor(c["campos"], device=DEV))
    (colors.sum() * 0 + t["means3D"].sum()).backward()
    assert (t["means3D"].grad == 1).all()
    # a binding entry outside the faces: NaN in the forward, an error where the table is built
    bad = dict(c)
    bad["binding"] = c["binding"].copy()
    bad["binding"][5] = 37
    t = _leaves(bad)
    colors = shaded_colors(t["features_dc"], t["features_rest"], 3, t["means3D"], torch.tensor(c["campos"], device=DEV),
                           binding=torch.tensor(bad["binding"], device=DEV), shadow_map=t["shadow_map"], sampler=_sampler(c))
    assert torch.isnan(colors[5]).all() and torch.isfinite(colors[:5]).all() and torch.isfinite(colors[6:]).all()
    with pytest.raises(RuntimeError, match="out of range"):
        colors.sum().backward()


# ---- 6. means3D from render_inputs: the rasteriser's gradient and this one add up ---------------------------------------------------------

def test_means3D_gets_both_gradients():
    """BoundGaussians.render_inputs -> means3D -> (a weighted sum standing for the rasteriser) + shaded_colors: the raw _xyz and the
    vertices receive the sum of both paths, against binding_twin_torch chained into shade_twin_torch in float64"""
    from mpmavatar_amd.mesh_frames import MeshFrames
    from mpmavatar_amd.render_inputs import BoundGaussians
    from mpmavatar_amd.shading import ShadowSampler
    b = bc.case("main")
    n, n_f = b["binding"].shape[0], b["faces"].shape[0]
    rng = np.random.default_rng(5)
    extra = {"features_dc": rng.normal(0, 0.5, (n, 1, 3)), "features_rest": rng.normal(0, 0.3, (n, 15, 3)),
             "face_uv": rng.uniform(-1.1, 1.1, (n_f, 2)), "shadow_map": rng.uniform(0.2, 1.0, (6, 5)), "w": rng.normal(size=(n, 3)),
             "campos": np.array([0.3, 0.2, -3.0])}
    extra = {k: v.astype(np.float32) for k, v in extra.items()}

    def chain(leaf, f, render_inputs, shaded):
        out = render_inputs(leaf)
        colors = shaded(out["means3D"], leaf)
        return (f(b["w_means3D"]) * out["means3D"]).sum() + (f(extra["w"]) * colors).sum()

    # ours
    dev = lambda a: torch.tensor(a, device=DEV)
    t = {k: dev(b[k]).requires_grad_(True) for k in bc.NAMES}
    t.update({k: dev(extra[k]).requires_grad_(True) for k in ("features_dc", "features_rest", "shadow_map")})
    fr = MeshFrames(dev(b["faces"]))
    bg = BoundGaussians(t["_xyz"], t["_rotation"], t["_scaling"], t["_opacity"], t["features_dc"], t["features_rest"], dev(b["binding"]))
    sampler = ShadowSampler(dev(extra["face_uv"]), 6, 5)

    def ours_inputs(_):
        fr.set_mesh_by_verts(t["verts"])
        return bg.render_inputs(fr)

    loss = chain(t, dev, ours_inputs, lambda m, _: bg.shaded_colors(m, dev(extra["campos"]), 3, shadow_map=t["shadow_map"], sampler=sampler))
    loss.backward()
    # the twins, float64
    d = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    u = {k: d(b[k]).requires_grad_(True) for k in bc.NAMES}
    u.update({k: d(extra[k]).requires_grad_(True) for k in ("features_dc", "features_rest", "shadow_map")})
    faces64, binding64 = torch.tensor(b["faces"].astype(np.int64)), torch.tensor(b["binding"].astype(np.int64))
    ref = chain(u, d, lambda x: btw.render_inputs(x["verts"], faces64, binding64, x["_xyz"], x["_rotation"], x["_scaling"], x["_opacity"]),
                lambda m, x: tw.shaded(3, x["features_dc"], x["features_rest"], m, d(extra["campos"]), x["shadow_map"], d(extra["face_uv"]),
                                       binding64))
    ref.backward()
    bound = max(sc.BOUND, bc.BOUND)
    for k in ("verts", "_xyz", "features_dc", "features_rest", "shadow_map"):
        err = sc.rel(t[k].grad.cpu().numpy(), u[k].grad.numpy())
        print(k, "%.3g of bound %.3g" % (err, bound))
        assert err <= bound, k
    # and the shading's share is really in there: without it the gradient of _xyz is another one
    only_raster = torch.autograd.grad((d(b["w_means3D"]) * btw.render_inputs(u["verts"], faces64, binding64, u["_xyz"], u["_rotation"], u["_scaling"],
                                                                            u["_opacity"])["means3D"]).sum(), u["_xyz"])[0]
    assert sc.rel(only_raster.numpy(), u["_xyz"].grad.numpy()) > 1e-3


# ---- 7. the example with trained colours ------------------------------------------------------------------------------------------------

def test_colors_demo_lowers_its_loss():
    path = os.path.join(bc.ROOT, "examples", "appearance_step_demo.py")
    spec = importlib.util.spec_from_file_location("appearance_step_demo", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    losses = mod.main(["--colors", "--size", "32", "--steps", "30"])
    print("loss %.6f -> %.6f" % (losses[0], losses[-1]))
    assert len(losses) == 31 and np.isfinite(losses).all() and losses[-1] < losses[0]
