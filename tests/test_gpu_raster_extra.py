"""The rasteriser's extra attribute channels on the GPU (mpmavatar_amd/csrc/raster_extra.hip through
mpmavatar_amd.rasterizer.GaussianRasterizer(...)(..., extra_attrs=table) and loss.backward()) against the float64 torch twin, in
which the extras are colours over a zero background (tests/raster_extra_cases.py).  The forward lies within raster_scenes.BOUND, every
gradient tensor within raster_extra_cases.BOUND_GX = 10 * G32X; G32X and the conditions that make the comparison meaningful are
measured and asserted on the CPU in tests/test_raster_extra_host.py.  Every comparison prints its figures before it asserts (-s)."""
import ctypes as C

import numpy as np
import pytest

import raster_extra_cases as xc
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
    return None if a is None else torch.tensor(np.asarray(a), device=_dev())          # a copy: the shared cases are read-only


def settings(cam, bg=rs.BG, sh_degree=0):
    from mpmavatar_amd.rasterizer import GaussianRasterizationSettings
    return GaussianRasterizationSettings(image_height=cam.image_height, image_width=cam.image_width, tanfovx=cam.tanfovx,
                                         tanfovy=cam.tanfovy, bg=_t(np.asarray(bg, np.float32)), scale_modifier=1.0,
                                         viewmatrix=_t(cam.viewmatrix), projmatrix=_t(cam.projmatrix), sh_degree=sh_degree,
                                         campos=_t(np.asarray(cam.campos, np.float32)), prefiltered=False, debug=False)


def leaves(sc, extra=None, geometry_grad=True, table_grad=True):
    import torch
    args = {k: (_t(np.asarray(sc[k], np.float32)).requires_grad_(geometry_grad) if sc.get(k) is not None else None) for k in FLOAT_INPUTS}
    args["means2D"] = torch.zeros_like(args["means3D"], requires_grad=True)       # as the reference passes it
    if extra is not None:
        args["extra_attrs"] = _t(extra).requires_grad_(table_grad)
    return args


def render(cam, args, rasterizer=None, **kw):
    """-> image, alpha, radii, slot 5, the rasteriser"""
    from mpmavatar_amd.rasterizer import GaussianRasterizer
    r = rasterizer or GaussianRasterizer(raster_settings=settings(cam, **kw))
    out = r(**args)
    assert len(out) == 6 and out[1] is None and out[2] is None
    assert (out[5] is None) == (args.get("extra_attrs") is None)
    return out[0], out[3], out[4], out[5], r


def loss_of(image, alpha, extra, Wi, Wa, Wx):
    total = 0
    for W, out in ((Wi, image), (Wa, alpha), (Wx, extra)):
        if W is not None:
            total = total + (_t(W) * out).sum()
    return total


def grads_of(args):
    return {k: v.grad.detach().cpu().numpy() for k, v in args.items() if v is not None and v.grad is not None}


def gpu_grads(case, Wi="case", Wa="case", Wx="case", extra=True, **kw):
    """forward with the case's table, backward of the loss -> (gradients by argument name, image, alpha, radii, slot 5), NumPy.
    A weight given as None leaves that output out of the graph's loss: its upstream gradient arrives as None."""
    import torch
    pick = lambda W, own: own if isinstance(W, str) else W
    args = leaves(case.sc, case.extra if extra else None)
    image, alpha, radii, blended, _ = render(case.cam, args, **kw)
    assert image.grad_fn is not None and alpha.grad_fn is not None and not radii.requires_grad and radii.dtype == torch.int32
    if extra:
        assert blended.grad_fn is not None and tuple(blended.shape) == (case.extra.shape[1],) + tuple(image.shape[1:])
    loss_of(image, alpha, blended, pick(Wi, case.Wi), pick(Wa, case.Wa), pick(Wx, case.Wx) if extra else None).backward()
    got = grads_of(args)
    for k, g in got.items():
        assert g.shape == tuple(args[k].shape), k
    host = lambda t: None if t is None else t.detach().cpu().numpy()
    return got, host(image), host(alpha), host(radii), host(blended)


def _same(a, b, but=()):
    assert set(a) - set(but) == set(b) - set(but)
    for k in a:
        if k not in but:
            assert np.array_equal(a[k], b[k]), k


# ---- the forward pass --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", rs.COMPARED, ids=IDS)
def test_slot_five_against_the_twin(key):
    import torch
    case = xc.scene_case(key)
    with torch.no_grad():
        image, alpha, radii, blended, _ = render(case.cam, leaves(case.sc, case.extra))
    assert blended.grad_fn is None and blended.dtype == torch.float32 and tuple(blended.shape) == (2, case.cam.image_height, case.cam.image_width)
    assert np.array_equal(radii.cpu().numpy(), case.radii)
    xc.check_forward(case, image.cpu().numpy(), alpha.cpu().numpy(), blended.cpu().numpy(), IDS(key))
    assert (blended[:, alpha[0] == 0] == 0).all()                         # no background term


@pytest.mark.parametrize("key", rs.COMPARED, ids=IDS)
def test_the_other_outputs_are_unchanged(key):
    """image, alpha and radii: the bits of the same call without extra_attrs, with and without a graph"""
    import torch
    case = xc.scene_case(key)
    for graph in (False, True):
        plain = render(case.cam, leaves(case.sc, None, geometry_grad=graph))
        with_x = render(case.cam, leaves(case.sc, case.extra, geometry_grad=graph, table_grad=False))
        assert (with_x[0].grad_fn is not None) == graph and (with_x[3].grad_fn is not None) == graph
        for a, b in zip(plain[:3], with_x[:3]):
            assert torch.equal(a.detach(), b.detach())


@pytest.mark.parametrize("key", rs.COMPARED, ids=IDS)
def test_two_call_composition(key):
    """what a user could do before: the table, padded to three channels, as colors_precomp of a second call over a zero background"""
    import torch
    case = xc.scene_case(key)
    with torch.no_grad():
        blended = render(case.cam, leaves(case.sc, case.extra))[3]
        second = render(case.cam, leaves(dict(case.sc, colors_precomp=xc.pad(case.extra)[0])), bg=np.zeros(3, np.float32))[0]
    diff = float((blended - second[:2]).abs().max())
    print(IDS(key), "max |fused - second call| = %.3g (bound %.3g); bit-equal: %s" % (diff, rs.BOUND, torch.equal(blended, second[:2])))
    assert diff <= rs.BOUND and (second[2] == 0).all()


# ---- gradients against the float64 twin ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", rs.COMPARED, ids=IDS)
def test_gradients_of_every_input_and_the_table(key):
    """loss on image, alpha and slot 5.  thin: 700 entries in one tile, three backward batches; front: early exit, the extras of
    the 700 hidden layers get exactly zero; the two odd shapes: lanes outside the image"""
    case = xc.scene_case(key)
    got, image, alpha, radii, blended = gpu_grads(case)
    assert set(got) == {"means3D", "means2D", "opacities", "colors_precomp", "scales", "rotations", "extra_attrs"}
    assert np.array_equal(radii, case.radii) and (got["means2D"][:, 2] == 0).all()
    xc.check_forward(case, image, alpha, blended, IDS(key))
    xc.check_grads(got, case.g64, IDS(key))
    if key[0] == "front":
        assert (got["extra_attrs"][rs.n_front():] == 0.0).all() and np.abs(got["extra_attrs"][:rs.n_front()]).max() > 0
    if key[0] == "thin":
        assert len(case.sc["means3D"]) > 2 * 256 and (radii > 0).all()    # one tile, every Gaussian in its list: three batches


def test_loss_on_slot_five_alone():
    """the upstream gradients of image and alpha arrive as None"""
    case = xc.scene_case(xc.OTHER_SCENE, xc.E_REF, ("extra",))
    got, *_ = gpu_grads(case, Wi=None, Wa=None)
    xc.check_grads(got, case.g64, "slot 5 alone")
    assert (got["colors_precomp"] == 0).all()


def test_constant_table_and_geometry_with_grad():
    """the reference's case: variables['cloth_mask'] is data"""
    case = xc.scene_case(xc.OTHER_SCENE)
    args = leaves(case.sc, case.extra, table_grad=False)
    image, alpha, _, blended, _ = render(case.cam, args)
    assert blended.grad_fn is not None
    loss_of(image, alpha, blended, case.Wi, case.Wa, case.Wx).backward()
    got = grads_of(args)
    assert "extra_attrs" not in got and args["extra_attrs"].grad is None
    xc.check_grads(got, {k: v for k, v in case.g64.items() if k != "extra_attrs"}, "constant table")


def test_table_with_grad_alone():
    case = xc.scene_case(xc.OTHER_SCENE)
    args = leaves(case.sc, case.extra, geometry_grad=False)
    args["means2D"].requires_grad_(False)
    image, alpha, _, blended, _ = render(case.cam, args)
    assert blended.grad_fn is not None
    loss_of(image, alpha, blended, case.Wi, case.Wa, case.Wx).backward()
    got = grads_of(args)
    assert set(got) == {"extra_attrs"}
    xc.check_grads(got, {"extra_attrs": case.g64["extra_attrs"]}, "table alone")


@pytest.mark.parametrize("E", (1, 3, 8))
def test_other_channel_counts(E):
    case = xc.scene_case(xc.OTHER_SCENE, E)
    got, image, alpha, _, blended = gpu_grads(case)
    assert blended.shape[0] == E and got["extra_attrs"].shape == case.extra.shape
    xc.check_forward(case, image, alpha, blended, f"E = {E}")
    xc.check_grads(got, case.g64, f"E = {E}")


def test_cov3d_precomp_path():
    case = xc.precomp_case()
    got, image, alpha, _, blended = gpu_grads(case)
    xc.check_forward(case, image, alpha, blended, "cov3Ds_precomp")
    xc.check_grads(got, case.g64, "cov3Ds_precomp")


def test_sh_path():
    case = xc.sh_case(2)
    got, image, alpha, _, blended = gpu_grads(case, sh_degree=2)
    xc.check_forward(case, image, alpha, blended, "shs")
    xc.check_grads(got, case.g64, "shs")


def test_all_culled_and_empty_scenes():
    cam = tw.simple_camera(16, 16)
    iso = lambda v: [v, 0, 0, v, 0, v]
    means = np.array([[0, 0, 0.2], [0, 0, 0.1], [0, 0, -3], [40, 0, 2], [0, -40, 2], [0, 0, 2]], np.float32)
    cov = np.array([iso(0.01)] * 5 + [[2.0 ** 34, 2.0 ** 34, 0, 2.0 ** 34, 0, 0]], np.float32)      # the last: det == 0 in fp32
    sc = dict(means3D=means, opacities=np.ones((6, 1), np.float32), colors_precomp=np.ones((6, 3), np.float32), cov3Ds_precomp=cov)
    rng = np.random.default_rng(1)
    Wi, Wa, Wx = (rng.normal(size=(c, 16, 16)).astype(np.float32) for c in (3, 1, 2))
    for scene in (sc, {k: v[:0] for k, v in sc.items()}):
        n = scene["means3D"].shape[0]
        args = leaves(scene, np.ones((n, 2), np.float32))
        image, alpha, radii, blended, _ = render(cam, args)
        assert tuple(blended.shape) == (2, 16, 16) and (blended == 0).all() and (radii == 0).all() and (alpha == 0).all()
        loss_of(image, alpha, blended, Wi, Wa, Wx).backward()
        got = grads_of(args)
        assert got["extra_attrs"].shape == (n, 2) and got["means3D"].shape == (n, 3)
        for k, g in got.items():
            assert (g == 0.0).all(), k


# ---- bits: an unused slot, reproducibility, who owns a frame's state ------------------------------------------------------------------

def test_unused_slot_five_leaves_the_bits_of_a_call_without_extras():
    """its gradient arrives as None: the extra tile pass and the gather are skipped"""
    case = xc.scene_case(("random", 0, 0))
    without = gpu_grads(case, extra=False)[0]
    args = leaves(case.sc, case.extra)
    image, alpha, _, blended, _ = render(case.cam, args)
    loss_of(image, alpha, None, case.Wi, case.Wa, None).backward()
    got = grads_of(args)
    assert "extra_attrs" not in got
    _same(got, without)
    used = gpu_grads(case)[0]
    assert not np.array_equal(used["means3D"], without["means3D"])        # ... and a used one does change them


def test_backward_is_bitwise_reproducible():
    import torch
    case = xc.scene_case(("random", 0, 0))
    args = leaves(case.sc, case.extra)
    image, alpha, _, blended, _ = render(case.cam, args)
    loss = loss_of(image, alpha, blended, case.Wi, case.Wa, case.Wx)
    order = [k for k, v in args.items() if v is not None]
    first = torch.autograd.grad(loss, [args[k] for k in order], retain_graph=True)
    second = torch.autograd.grad(loss, [args[k] for k in order])
    for k, a, b in zip(order, first, second):
        assert torch.equal(a, b), k                                       # two passes over one graph
    fresh = [gpu_grads(case)[0] for _ in range(2)]
    _same(fresh[0], fresh[1])                                             # two fresh graphs
    _same(fresh[0], {k: g.cpu().numpy() for k, g in zip(order, first)})


def test_a_frame_owns_its_state():
    """forward A with extras, forward B with and without extras on the shared handle, backward A: the bits of A alone"""
    case = xc.scene_case(("random", 0, 0))
    alone = gpu_grads(case)[0]
    args = leaves(case.sc, case.extra)
    image, alpha, _, blended, _ = render(case.cam, args)
    other = xc.scene_case(("odd", 9, 70))
    for table in (other.extra, None):
        for requires_grad in (True, False):                               # differentiable frames and plain ones in between
            out = render(other.cam, leaves(other.sc, table, geometry_grad=requires_grad, table_grad=False))
            assert (out[0].grad_fn is not None) == requires_grad
    loss_of(image, alpha, blended, case.Wi, case.Wa, case.Wx).backward()
    _same(grads_of(args), alone)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------

def test_bad_tables_raise_before_any_launch():
    import torch
    from mpmavatar_amd.rasterizer import GaussianRasterizer
    case = xc.scene_case(xc.OTHER_SCENE)
    n = case.extra.shape[0]
    one = GaussianRasterizer(settings(case.cam), private_scratch=True)
    good = torch.zeros(n, 2, device=_dev())
    bad = {"E = 9": torch.zeros(n, 9, device=_dev()), "E = 0": torch.zeros(n, 0, device=_dev()), "[N]": torch.zeros(n, device=_dev()),
           "float64": good.double(), "CPU": good.cpu(), "N mismatch": torch.zeros(n + 1, 2, device=_dev()), "a list": [[0.0, 1.0]] * n,
           "not contiguous": torch.zeros(2, n, device=_dev()).t()}
    for what, table in bad.items():
        args = leaves(case.sc)
        args["extra_attrs"] = table
        with pytest.raises(RuntimeError, match="extra_attrs"):
            one(**args)
        assert one._last is None and not one._handles, what               # not even a handle was made
    assert one(**dict(leaves(case.sc), extra_attrs=good))[5].shape == (2, case.cam.image_height, case.cam.image_width)


def test_abi_error_paths_write_nothing_and_state_is_checked():
    import torch
    from mpmavatar_amd import _lib as L
    lib = L.load()
    case = xc.scene_case(("odd", 9, 70))
    cam = case.cam
    d = {k: _t(v) for k, v in case.sc.items()}
    n, dev = d["means3D"].shape[0], _dev()
    table = _t(case.extra)
    st = settings(cam)
    mk = lambda h, w: L.RasterSettings(h, w, cam.tanfovx, cam.tanfovy, L.f3(0, 0, 0), 1.0, 0, st.viewmatrix.data_ptr(), st.projmatrix.data_ptr(),
                                       st.campos.data_ptr())
    cs, other = mk(9, 70), mk(9, 71)
    image, alpha = torch.empty(3, 9, 70, device=dev), torch.empty(1, 9, 70, device=dev)
    radii = torch.empty(n, dtype=torch.int32, device=dev)
    out_x = torch.full((2, 9, 70), -7.0, device=dev)
    h = L.vp()
    assert lib.mpmhip_raster_create(0, None, C.byref(h)) == L.OK
    fwd = (h, C.byref(cs), n, d["means3D"].data_ptr(), None, 0, d["colors_precomp"].data_ptr(), d["opacities"].data_ptr(),
           d["scales"].data_ptr(), d["rotations"].data_ptr(), None, image.data_ptr(), alpha.data_ptr(), radii.data_ptr())
    xf = lambda handle=h, s=cs, n_=n, t=table.data_ptr(), E=2, o=out_x.data_ptr(): lib.mpmhip_raster_extra_forward(handle, C.byref(s), n_, t, E, o)
    assert xf() == L.ERR_STATE                                             # nothing rendered yet
    assert lib.mpmhip_raster_forward(*fwd) == L.OK
    assert xf() == L.ERR_STATE                                             # a plain frame recorded no stopping positions
    assert lib.mpmhip_raster_forward_grad(*fwd) == L.OK
    for kw in (dict(handle=None), dict(t=None), dict(o=None), dict(E=0), dict(E=9), dict(E=-1), dict(n_=-1)):
        assert xf(**kw) == L.ERR_INVALID, kw
    for kw in (dict(n_=n - 1), dict(s=other)):
        assert xf(**kw) == L.ERR_STATE, kw                                 # another n or image size than the frame's
    torch.cuda.synchronize()
    assert (out_x == -7).all()
    assert xf() == L.OK
    torch.cuda.synchronize()
    assert torch.isfinite(out_x).all() and (out_x != -7).all()
    size, entries = C.c_int64(), C.c_int64()
    assert lib.mpmhip_raster_saved_bytes(h, C.byref(size), C.byref(entries)) == L.OK
    saved = torch.empty(size.value, dtype=torch.uint8, device=dev)
    assert lib.mpmhip_raster_save(h, saved.data_ptr(), size.value) == L.OK
    assert lib.mpmhip_raster_forward(*fwd) == L.OK and xf() == L.ERR_STATE   # the frame is no longer the newest
    g_image, g_alpha, g_x = torch.ones(3, 9, 70, device=dev), torch.ones(1, 9, 70, device=dev), torch.ones(2, 9, 70, device=dev)
    out = {k: torch.full(s, -7.0, device=dev) for k, s in (("means3D", (n, 3)), ("means2D", (n, 3)), ("colors", (n, 3)), ("opac", (n, 1)),
                                                           ("scales", (n, 3)), ("rots", (n, 4)), ("extra", (n, 2)))}
    p = lambda t: None if t is None else t.data_ptr()

    def backward(E=2, t=table, gx=g_x, bytes_=size.value, entries_=None, drop=(), handle=h, settings_=cs):
        o = {k: (None if k in drop else v) for k, v in out.items()}
        return lib.mpmhip_raster_backward_extra(handle, C.byref(settings_), n, d["means3D"].data_ptr(), None, 0, d["colors_precomp"].data_ptr(),
                                                d["opacities"].data_ptr(), d["scales"].data_ptr(), d["rotations"].data_ptr(), None,
                                                saved.data_ptr(), bytes_, entries.value if entries_ is None else entries_, p(g_image),
                                                p(g_alpha), p(o["means3D"]), p(o["means2D"]), None, p(o["colors"]), p(o["opac"]),
                                                p(o["scales"]), p(o["rots"]), None, p(t), E, p(gx), p(o["extra"]))

    for kw in (dict(E=0), dict(E=9), dict(t=None), dict(drop=("extra",)), dict(drop=("means3D",)), dict(bytes_=size.value - 8),
               dict(entries_=entries.value - 1), dict(handle=None), dict(settings_=other)):
        assert backward(**kw) == L.ERR_INVALID, kw
    torch.cuda.synchronize()
    for k, v in out.items():
        assert (v == -7).all(), k                                         # nothing was launched
    assert backward(gx=None) == L.OK                                       # NULL = zeros
    torch.cuda.synchronize()
    assert (out["extra"] == 0).all() and (out["means3D"] != -7).all()
    assert backward() == L.OK
    torch.cuda.synchronize()
    for k, v in out.items():
        assert torch.isfinite(v).all() and (v != -7).all(), k
    assert out["extra"].abs().max() > 0
    lib.mpmhip_raster_destroy(h)


# ---- it trains ---------------------------------------------------------------------------------------------------------------------

def test_a_small_fit_halves_its_mask_loss():
    """32 x 32, a 0 / 1 table over two groups of Gaussians, 30 Adam steps on means3D alone towards a mask rendered from shifted
    means, with the reference's term (train_mesh_lbs_4ddress.py:306: the L1 of slot 5 against the data's garment mask)"""
    import torch
    cam = tw.simple_camera(32, 32)
    rng = np.random.default_rng(33)
    n = 24
    z = np.linspace(1.5, 3.0, n)
    means = np.stack([rng.uniform(-0.3, 0.3, n) * z, rng.uniform(-0.3, 0.3, n) * z, z], 1).astype(np.float32)
    shift = np.array([[0.12, -0.08, 0.0]], np.float32) * z[:, None].astype(np.float32)
    table = np.zeros((n, 2), np.float32)
    table[: n // 2, 0] = 1.0
    table[n // 2:, 1] = 1.0
    fixed = dict(opacities=_t(np.full((n, 1), 0.7, np.float32)), scales=_t(np.full((n, 3), 0.12, np.float32)),
                 rotations=_t(np.tile(np.array([[1, 0, 0, 0]], np.float32), (n, 1))), colors_precomp=_t(np.full((n, 3), 0.5, np.float32)),
                 shs=None, cov3Ds_precomp=None, extra_attrs=_t(table))

    def mask(m):
        return render(cam, dict(fixed, means3D=m, means2D=torch.zeros(n, 3, device=_dev(), requires_grad=True)))[3]

    with torch.no_grad():
        target = mask(_t(means + shift))
    m = _t(means).requires_grad_(True)
    opt = torch.optim.Adam([m], lr=0.01)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        loss = (mask(m) - target).abs().mean()
        loss.backward()
        assert torch.isfinite(m.grad).all()
        opt.step()
        losses.append(float(loss.detach()))
    print("fit: mask L1 %.4g -> %.4g" % (losses[0], losses[-1]))
    assert losses[-1] <= 0.5 * losses[0]
