"""The rasteriser's backward pass on the GPU (mpmavatar_amd/csrc/raster_backward.hip through mpmavatar_amd.rasterizer and
loss.backward()) against the gradient autograd takes of the float64 torch twin (tests/raster_twin_torch.py), with the loss
L = sum Wi image + sum Wa alpha of tests/raster_grad_scenes.py.  Every gradient tensor must lie within
raster_grad_scenes.BOUND_G = 10 * G32 of the twin's (max |g - g64| / max |g64|); G32 and the conditions that make the comparison
meaningful are measured and asserted on the CPU in tests/test_raster_grad_host.py.  Every comparison prints its figures before it
asserts (run with -s)."""
import ctypes as C

import numpy as np
import pytest

import raster_grad_scenes as gs
import raster_scenes as rs
import raster_twin as tw

pytestmark = pytest.mark.gpu

FLOAT_INPUTS = ("means3D", "opacities", "shs", "colors_precomp", "scales", "rotations", "cov3Ds_precomp")
IDS = lambda k: "-".join(map(str, k))


def _dev():
    import torch
    return torch.device("cuda:0")


def _t(a):
    import torch
    return None if a is None else torch.tensor(np.asarray(a), device=_dev())          # a copy: the shared twins are read-only


def settings(cam, bg=rs.BG, sh_degree=0, scale_modifier=1.0):
    from mpmavatar_amd.rasterizer import GaussianRasterizationSettings
    return GaussianRasterizationSettings(image_height=cam.image_height, image_width=cam.image_width, tanfovx=cam.tanfovx,
                                         tanfovy=cam.tanfovy, bg=_t(np.asarray(bg, np.float32)), scale_modifier=scale_modifier,
                                         viewmatrix=_t(cam.viewmatrix), projmatrix=_t(cam.projmatrix), sh_degree=sh_degree,
                                         campos=_t(np.asarray(cam.campos, np.float32)), prefiltered=False, debug=False)


def leaves(sc, requires_grad=True):
    import torch
    args = {k: (_t(np.asarray(sc[k], np.float32)).requires_grad_(requires_grad) if sc.get(k) is not None else None) for k in FLOAT_INPUTS}
    args["means2D"] = torch.zeros_like(args["means3D"], requires_grad=True)       # as the reference passes it
    return args


def render(cam, args, rasterizer=None, **kw):
    from mpmavatar_amd.rasterizer import GaussianRasterizer
    r = rasterizer or GaussianRasterizer(raster_settings=settings(cam, **kw))
    out = r(**args)
    assert len(out) == 6 and out[1] is None and out[2] is None and out[5] is None
    return out[0], out[3], out[4], r


def loss_of(image, alpha, Wi, Wa):
    total = 0
    if Wi is not None:
        total = total + (_t(Wi) * image).sum()
    if Wa is not None:
        total = total + (_t(Wa) * alpha).sum()
    return total


def grads_of(args):
    return {k: v.grad.detach().cpu().numpy() for k, v in args.items() if v is not None and v.grad is not None}


def gpu_grads(cam, sc, Wi, Wa, **kw):
    """forward through GaussianRasterizer, backward of the loss -> (gradients by input name, image, alpha, radii), NumPy"""
    import torch
    args = leaves(sc)
    image, alpha, radii, _ = render(cam, args, **kw)
    assert image.grad_fn is not None and alpha.grad_fn is not None and not radii.requires_grad and radii.dtype == torch.int32
    loss_of(image, alpha, Wi, Wa).backward()
    got = grads_of(args)
    assert set(got) == {k for k, v in args.items() if v is not None}
    for k, g in got.items():
        assert g.shape == tuple(args[k].shape), k
    assert (got["means2D"][:, 2] == 0).all()
    return got, image.detach().cpu().numpy(), alpha.detach().cpu().numpy(), radii.cpu().numpy()


# ---- against the float64 twin ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", rs.COMPARED, ids=IDS)
def test_committed_scene_gradients_against_the_twin(key):
    """the four random scenes (one tile list longer than 256: the reverse batch loop runs more than once, a partial batch first),
    thin (700 entries, three batches, T never saturates), front (early exit) and the two odd shapes (lanes outside the image)"""
    cam, sc, Wi, Wa, g64, g32, share, r64, r32 = gs.scene_grads(*key)
    got, image, alpha, radii = gpu_grads(cam, sc, Wi, Wa)
    assert np.array_equal(radii, r64.base.radii)
    gs.check_grads(got, g64, IDS(key))
    if key[0] == "front":
        for k, g in got.items():
            assert (g[rs.n_front():] == 0.0).all(), k                    # the 700 hidden layers: exactly zero in every tensor
            if k != "colors_precomp":
                assert (g[0] == 0.0).all(), k                            # clamped at 0.99 on all 256 pixels: a colour gradient only
        assert np.abs(got["colors_precomp"][0]).max() > 0


def test_equal_depths_go_by_index():
    cam = tw.simple_camera(16, 16)
    mean = np.array([[0.05, -0.03, 2.0]], np.float32)
    # anisotropic scales: with isotropic ones the rotation gradient is zero up to float64 rounding, and a relative error means nothing
    sc = dict(means3D=np.concatenate([mean, mean]), opacities=np.full((2, 1), 0.8, np.float32),
              scales=np.tile(np.array([[0.3, 0.2, 0.25]], np.float32), (2, 1)),
              rotations=np.tile(np.array([[1, 0.1, -0.2, 0.3]], np.float32), (2, 1)),
              colors_precomp=np.array([[1, 0, 0], [0, 0, 1]], np.float32))
    Wi, Wa, g64, g32, share, r64, r32 = gs.grad_twins(cam, sc)
    assert share <= gs.MAX_LEFT_OUT_SHARE
    got, *_ = gpu_grads(cam, sc, Wi, Wa)
    gs.check_grads(got, g64, "ties")
    assert np.abs(got["opacities"][0] - got["opacities"][1]).max() > 1e-3          # the order matters to the gradient


def test_all_culled_and_empty_scenes_give_zero_gradients():
    cam = tw.simple_camera(16, 16)
    iso = lambda v: [v, 0, 0, v, 0, v]
    means = np.array([[0, 0, 0.2], [0, 0, 0.1], [0, 0, -3], [40, 0, 2], [0, -40, 2], [0, 0, 2]], np.float32)
    cov = np.array([iso(0.01)] * 5 + [[2.0 ** 34, 2.0 ** 34, 0, 2.0 ** 34, 0, 0]], np.float32)      # the last: det == 0 in fp32
    sc = dict(means3D=means, opacities=np.ones((6, 1), np.float32), colors_precomp=np.ones((6, 3), np.float32), cov3Ds_precomp=cov)
    Wi, Wa = (w.astype(np.float32) for w in gs.weights(16, 16))
    for scene in (sc, {k: v[:0] for k, v in sc.items()}):
        got, image, alpha, radii = gpu_grads(cam, scene, Wi, Wa)
        n = scene["means3D"].shape[0]
        assert (radii == 0).all() and (alpha == 0).all()
        assert got["means3D"].shape == (n, 3) and got["cov3Ds_precomp"].shape == (n, 6) and got["opacities"].shape == (n, 1)
        for k, g in got.items():
            assert (g == 0.0).all(), k


def test_cov3d_precomp_path():
    cam, sc, Wi, Wa, g64, g32, share, r64, r32 = gs.precomp_grads()
    got, *_ = gpu_grads(cam, sc, Wi, Wa)
    gs.check_grads(got, g64, "cov3Ds_precomp")


@pytest.mark.parametrize("deg", (0, 1, 2, 3))
def test_sh_path(deg):
    """gradients to shs (zero above the degree) and the view-direction term of means3D"""
    cam, sc, Wi, Wa, g64, g32, share, r64, r32 = gs.sh_grads(deg)
    got, *_ = gpu_grads(cam, sc, Wi, Wa, sh_degree=deg)
    gs.check_grads(got, g64, f"sh degree {deg}")
    assert (got["shs"][:, (deg + 1) ** 2:] == 0).all()


@pytest.mark.parametrize("use", ("image", "alpha"))
def test_only_one_output_used(use):
    """the other output's incoming gradient is None; the image's arrives non-contiguous (through a permute)"""
    cam, sc, _, _ = rs.twins("odd", 33, 17)
    Wi, Wa, g64, g32, share, r64, r32 = gs.grad_twins(cam, sc, use_image=use == "image", use_alpha=use == "alpha")
    args = leaves(sc)
    image, alpha, _, _ = render(cam, args)
    if use == "image":
        loss = (image.permute(1, 2, 0) * _t(np.ascontiguousarray(Wi.transpose(1, 2, 0)))).sum()
    else:
        loss = loss_of(image, alpha, None, Wa)
    loss.backward()
    gs.check_grads(grads_of(args), g64, f"only {use}")


# ---- reproducibility and who owns a frame's state ----------------------------------------------------------------------------------

def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_backward_is_bitwise_reproducible():
    import torch
    cam, sc, Wi, Wa, *_ = gs.scene_grads("random", 0, 0)
    args = leaves(sc)
    image, alpha, _, _ = render(cam, args)
    loss = loss_of(image, alpha, Wi, Wa)
    order = [k for k, v in args.items() if v is not None]
    first = torch.autograd.grad(loss, [args[k] for k in order], retain_graph=True)
    second = torch.autograd.grad(loss, [args[k] for k in order])
    for k, a, b in zip(order, first, second):
        assert torch.equal(a, b), k                                       # two passes over one graph
    fresh = [gpu_grads(cam, sc, Wi, Wa)[0] for _ in range(2)]
    _same(fresh[0], fresh[1])                                             # two fresh graphs
    _same(fresh[0], {k: g.cpu().numpy() for k, g in zip(order, first)})


def test_a_frame_owns_its_state():
    """forward A, forward B on the shared handle, backward A: the same bits as backward straight after forward A"""
    cam, sc, Wi, Wa, *_ = gs.scene_grads("random", 0, 0)
    alone = gpu_grads(cam, sc, Wi, Wa)[0]
    args = leaves(sc)
    image, alpha, _, _ = render(cam, args)
    cam_b, sc_b, *_ = rs.twins("odd", 9, 70)
    for requires_grad in (True, False):                                   # a differentiable frame and a plain one in between
        image_b, *_ = render(cam_b, leaves(sc_b, requires_grad))
        assert (image_b.grad_fn is not None) == requires_grad
    loss_of(image, alpha, Wi, Wa).backward()
    _same(grads_of(args), alone)


def test_no_graph_unless_an_input_other_than_means2d_asks():
    import torch
    from mpmavatar_amd.rasterizer import GaussianRasterizer
    cam, sc, *_ = rs.twins("random", 1, 0)
    one = GaussianRasterizer(settings(cam), private_scratch=True)
    plain = render(cam, leaves(sc, requires_grad=False), rasterizer=one)  # means2D alone requires grad: the eval loop's call
    assert plain[0].grad_fn is None and not plain[0].requires_grad and plain[1].grad_fn is None
    before = one.stats()
    with torch.no_grad():
        quiet = render(cam, leaves(sc), rasterizer=one)
    assert quiet[0].grad_fn is None and quiet[1].grad_fn is None
    assert one.stats() == before                                          # scratch_bytes did not grow: nothing new was allocated
    graph = render(cam, leaves(sc), rasterizer=one)
    assert graph[0].grad_fn is not None and graph[1].grad_fn is not None and not graph[2].requires_grad
    for a, b, c in zip(plain[:3], quiet[:3], graph[:3]):                  # image, alpha and radii: the same bits all three ways
        assert torch.equal(a, b) and torch.equal(a, c.detach())
    st = one.stats()
    assert st["scratch_bytes"] > before["scratch_bytes"] and {k: v for k, v in st.items() if k != "scratch_bytes"} == \
        {k: v for k, v in before.items() if k != "scratch_bytes"}


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------

def test_abi_error_paths_return_invalid_and_write_nothing():
    import torch
    from mpmavatar_amd import _lib as L
    lib = L.load()
    cam, sc, *_ = rs.twins("odd", 9, 70)
    d = {k: _t(v) for k, v in sc.items()}
    n, dev = d["means3D"].shape[0], _dev()
    st = settings(cam)
    cs = L.RasterSettings(9, 70, cam.tanfovx, cam.tanfovy, L.f3(0, 0, 0), 1.0, 0, st.viewmatrix.data_ptr(), st.projmatrix.data_ptr(),
                          st.campos.data_ptr())
    image, alpha = torch.empty(3, 9, 70, device=dev), torch.empty(1, 9, 70, device=dev)
    radii = torch.empty(n, dtype=torch.int32, device=dev)
    h = L.vp()
    assert lib.mpmhip_raster_create(0, None, C.byref(h)) == L.OK
    size, entries = C.c_int64(), C.c_int64()
    fwd = (h, C.byref(cs), n, d["means3D"].data_ptr(), None, 0, d["colors_precomp"].data_ptr(), d["opacities"].data_ptr(),
           d["scales"].data_ptr(), d["rotations"].data_ptr(), None, image.data_ptr(), alpha.data_ptr(), radii.data_ptr())
    assert lib.mpmhip_raster_forward(*fwd) == L.OK
    assert lib.mpmhip_raster_saved_bytes(h, C.byref(size), C.byref(entries)) == L.ERR_STATE      # a plain frame saved nothing
    assert lib.mpmhip_raster_forward_grad(*fwd) == L.OK
    assert lib.mpmhip_raster_saved_bytes(h, C.byref(size), C.byref(entries)) == L.OK and size.value > 0 and entries.value > 0
    saved = torch.full((size.value,), 0x5a, dtype=torch.uint8, device=dev)
    assert lib.mpmhip_raster_save(h, saved.data_ptr(), size.value - 1) == L.ERR_INVALID
    assert lib.mpmhip_raster_save(h, None, size.value) == L.ERR_INVALID
    torch.cuda.synchronize()
    assert (saved == 0x5a).all()
    assert lib.mpmhip_raster_save(h, saved.data_ptr(), size.value) == L.OK
    g_image, g_alpha = torch.ones(3, 9, 70, device=dev), torch.ones(1, 9, 70, device=dev)
    shs, cov = torch.zeros(n, 16, 3, device=dev), torch.zeros(n, 6, device=dev)
    out = {k: torch.full(s, -7.0, device=dev) for k, s in (("means3D", (n, 3)), ("means2D", (n, 3)), ("shs", (n, 16, 3)), ("colors", (n, 3)),
                                                           ("opac", (n, 1)), ("scales", (n, 3)), ("rots", (n, 4)), ("cov", (n, 6)))}
    p = lambda t: None if t is None else t.data_ptr()

    def backward(n_=n, settings_=cs, saved_=saved, bytes_=size.value, entries_=None, shs_=None, n_sh=0, colors=d["colors_precomp"],
                 scales=d["scales"], rots=d["rotations"], cov_=None, gi=g_image, ga=g_alpha, drop=(), handle=h):
        o = {k: (None if k in drop else v) for k, v in out.items()}
        return lib.mpmhip_raster_backward(handle, C.byref(settings_), n_, d["means3D"].data_ptr(), p(shs_), n_sh, p(colors),
                                          d["opacities"].data_ptr(), p(scales), p(rots), p(cov_), p(saved_), bytes_,
                                          entries.value if entries_ is None else entries_, p(gi), p(ga), p(o["means3D"]), p(o["means2D"]),
                                          p(o["shs"]), p(o["colors"]), p(o["opac"]), p(o["scales"]), p(o["rots"]), p(o["cov"]))

    other = L.RasterSettings(9, 71, cam.tanfovx, cam.tanfovy, L.f3(0, 0, 0), 1.0, 0, st.viewmatrix.data_ptr(), st.projmatrix.data_ptr(),
                             st.campos.data_ptr())
    bad = [dict(handle=None), dict(saved_=None), dict(bytes_=size.value - 8), dict(bytes_=size.value + 16), dict(n_=n - 1), dict(n_=-1),
           dict(entries_=entries.value - 1), dict(entries_=-1), dict(settings_=other), dict(shs_=shs, n_sh=16), dict(colors=None),
           dict(cov_=cov), dict(scales=None, rots=None), dict(rots=None), dict(drop=("means3D",)), dict(drop=("means2D",)),
           dict(drop=("opac",)), dict(drop=("colors",)), dict(drop=("scales",)), dict(drop=("rots",)),
           dict(colors=None, shs_=shs, n_sh=16, drop=("shs",)), dict(scales=None, rots=None, cov_=cov, drop=("cov",))]
    for kw in bad:
        assert backward(**kw) == L.ERR_INVALID, kw
    torch.cuda.synchronize()
    for k, v in out.items():
        assert (v == -7).all(), k                                         # nothing was launched
    assert backward() == L.OK and backward(gi=None) == L.OK and backward(ga=None) == L.OK     # the controls; NULL = zeros
    torch.cuda.synchronize()
    for k in ("means3D", "means2D", "colors", "opac", "scales", "rots"):
        assert torch.isfinite(out[k]).all() and (out[k] != -7).all(), k
    assert (out["shs"] == -7).all() and (out["cov"] == -7).all()          # not this frame's alternatives
    lib.mpmhip_raster_destroy(h)


# ---- it trains ---------------------------------------------------------------------------------------------------------------------

def test_a_small_fit_halves_its_loss():
    """32 x 32, 30 Adam steps on colours, opacities and scales towards an image rendered from perturbed parameters, with the
    reference's loss term (train_appearance.py:137-140: L1 of (image * mask).clip(0, 1))"""
    import torch
    cam = tw.simple_camera(32, 32)
    rng = np.random.default_rng(21)
    n = 24
    z = np.linspace(1.5, 3.0, n)
    means = np.stack([rng.uniform(-0.4, 0.4, n) * z, rng.uniform(-0.4, 0.4, n) * z, z], 1).astype(np.float32)
    rots = rng.normal(size=(n, 4)).astype(np.float32)
    truth = dict(col=rng.uniform(0, 1, (n, 3)), op=rng.uniform(-1, 2, (n, 1)), sc=np.log(rng.uniform(0.08, 0.3, (n, 3))))
    start = dict(col=np.full((n, 3), 0.5), op=np.zeros((n, 1)), sc=truth["sc"] + rng.normal(0, 0.4, (n, 3)))
    r = render
    fixed = dict(means3D=_t(means), rotations=_t(rots), shs=None, cov3Ds_precomp=None)

    def picture(par):
        args = dict(fixed, means2D=torch.zeros(n, 3, device=_dev(), requires_grad=True), colors_precomp=par["col"],
                    opacities=torch.sigmoid(par["op"]), scales=torch.exp(par["sc"]))
        image, mask, _, _ = r(cam, args)
        return (image * mask).clip(0, 1), args["means2D"]

    with torch.no_grad():
        target, _ = picture({k: _t(v.astype(np.float32)) for k, v in truth.items()})
    par = {k: _t(v.astype(np.float32)).requires_grad_(True) for k, v in start.items()}
    opt = torch.optim.Adam(list(par.values()), lr=0.05)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        pic, m2 = picture(par)
        loss = (pic - target).abs().mean()
        loss.backward()
        assert m2.grad is not None and torch.isfinite(m2.grad).all()     # what the densification statistics read
        opt.step()
        losses.append(float(loss.detach()))
    print("fit: loss %.4g -> %.4g" % (losses[0], losses[-1]))
    assert losses[-1] <= 0.5 * losses[0]
