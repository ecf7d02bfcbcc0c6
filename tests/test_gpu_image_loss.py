"""The image loss on the GPU (mpmavatar_amd/csrc/image_loss.hip through mpmavatar_amd.image_loss) against the reference's own
float64 results (tests/golden/image_loss.npz).  Every value and every gradient must lie within image_loss_cases.BOUND =
10 * S32 of the float64 run; S32 and the conditions that make the comparison meaningful are measured and asserted on the CPU in
tests/test_image_loss_host.py.  Every comparison prints its figures before it asserts (run with -s).

Worst figures measured on an MI355X: see DESIGN.md section 14."""
import ctypes as C

import numpy as np
import pytest

import image_loss_cases as ic
import raster_scenes as rs

pytestmark = pytest.mark.gpu


def _dev():
    import torch
    return torch.device("cuda:0")


def _t(a, requires_grad=False):
    import torch
    return torch.tensor(np.asarray(a), device=_dev(), requires_grad=requires_grad)     # a copy: the shared cases are read-only


def _n(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def il():
    import mpmavatar_amd.image_loss as m
    return m


# ---- against the reference's float64 run ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ic.CASES)
def test_values_against_float64(il, name):
    img, gt = (_t(a) for a in ic.case(name))
    loss, Ll1, s = il.image_loss(img, gt, ic.LAMBDA)
    got = {"l1": il.l1_loss(img, gt), "ssim": il.ssim(img, gt), "psnr": il.psnr(img, gt)}
    assert got["l1"].shape == got["ssim"].shape == loss.shape == Ll1.shape == s.shape == () and got["psnr"].shape == (img.shape[0], 1)
    if img.dim() == 4:
        got["ssim_per_item"] = il.ssim(img, gt, size_average=False)
        assert got["ssim_per_item"].shape == (img.shape[0],)
    else:
        with pytest.raises(IndexError):
            il.ssim(img, gt, size_average=False)
    assert set(got) == set(ic.value_keys(name))
    for k, v in got.items():
        err = ic.rel_value(_n(v), ic.ref(name, k))
        print(name, k, "%.3g of bound %.3g" % (err, ic.BOUND))
        assert err <= ic.BOUND, k
    import torch
    assert torch.equal(Ll1, got["l1"]) and torch.equal(s, got["ssim"])              # one launch or two: the same bits
    err = ic.rel_value(_n(loss), ic.loss_value_64(name))
    print(name, "loss %.3g" % err)
    assert err <= ic.BOUND


@pytest.mark.parametrize("name", ic.CASES)
def test_gradients_against_float64(il, name):
    img, gt = ic.case(name)
    a = _t(img, requires_grad=True)
    loss, _, _ = il.image_loss(a, _t(gt), ic.LAMBDA)
    loss.backward()
    assert a.grad.shape == a.shape
    err = ic.rel_grad(_n(a.grad), ic.d_loss_64(name))
    print(name, "d loss %.3g of bound %.3g" % (err, ic.BOUND))
    assert err <= ic.BOUND
    b = _t(img, requires_grad=True)
    il.ssim(b, _t(gt)).backward()
    err = ic.rel_grad(_n(b.grad), ic.ref(name, "d_ssim"))
    print(name, "d ssim %.3g" % err)
    assert err <= ic.BOUND
    c = _t(img, requires_grad=True)
    il.l1_loss(c, _t(gt)).backward()
    assert ic.rel_grad(_n(c.grad), ic.d_l1(img, gt)) <= ic.BOUND
    assert (_n(c.grad)[..., :2, :3] == 0).all()                                       # the exact ties: sign(0) = 0
    d = _t(img, requires_grad=True)
    il.psnr(d, _t(gt)).sum().backward()                                               # through log10 and sqrt of the per-item mse
    x, y = img.astype(np.float64), gt.astype(np.float64)
    mse = ((x - y) ** 2).reshape(img.shape[0], -1).mean(1)
    want = -10.0 / np.log(10.0) * 2.0 * (x - y) / ((x - y)[0].size * mse.reshape((-1,) + (1,) * (img.ndim - 1)))
    assert ic.rel_grad(_n(d.grad), want) <= ic.BOUND


def test_against_the_host_build(il):
    """the kernels and the serial host statement of the same header: far closer to each other than to float64"""
    img, gt = ic.case("ragged")
    means, maps, _ = ic.host_forward(img, gt)
    got = np.stack([_n(m) for m in il.plane_means(_t(img), _t(gt))], 1)
    print("means: worst |gpu - host| / host %.3g" % np.max(np.abs(got - means) / np.abs(means)))
    assert np.max(np.abs(got - means) / np.abs(means)) <= 4 * 2.0 ** -24
    a = _t(img, requires_grad=True)
    il.ssim(a, _t(gt)).backward()
    host = ic.host_backward(img, gt, maps, 0.0, 0.0, 1.0 / 3)
    print("d ssim: gpu against host %.3g" % ic.rel_grad(_n(a.grad), host))
    assert ic.rel_grad(_n(a.grad), host) <= ic.S32


# ---- reproducibility, the no-grad path, inputs ----------------------------------------------------------------------------------------

def _run(il, img, gt):
    a = _t(img, requires_grad=True)
    out = il.image_loss(a, _t(gt), ic.LAMBDA)
    out[0].backward()
    return [t.detach() for t in out] + [a.grad]


def test_two_runs_give_identical_bits(il):
    import torch
    for name in ("ragged", "wide"):
        first, second = _run(il, *ic.case(name)), _run(il, *ic.case(name))
        for x, y in zip(first, second):
            assert torch.equal(x, y)


def test_no_grad_path_same_bits_and_no_maps(il):
    import torch
    img, gt = (_t(a) for a in ic.case("ragged"))
    maps_bytes = img.numel() * 3 * 4                                                  # one plane-set of maps
    a = img.clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with_graph = il.plane_means(a, gt)
    grown_graph = torch.cuda.max_memory_allocated() - before
    assert all(t.grad_fn is not None for t in with_graph) and grown_graph >= maps_bytes   # the measurement sees the maps
    del with_graph
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with torch.no_grad():
        quiet = il.plane_means(a, gt)
    grown = torch.cuda.max_memory_allocated() - before
    print("peak growth: %d B with a graph, %d B without, maps %d B" % (grown_graph, grown, maps_bytes))
    assert grown < maps_bytes
    plain = il.plane_means(img, gt)                                                   # grad mode on, nothing requires grad
    graph = il.plane_means(a, gt)
    for q, p, g in zip(quiet, plain, graph):
        assert q.grad_fn is None and p.grad_fn is None and g.grad_fn is not None
        assert torch.equal(q, p) and torch.equal(q, g.detach())


def test_non_contiguous_inputs_and_another_stream(il):
    import torch
    img, gt = ic.case("ragged")
    want = _run(il, img, gt)
    a = _t(np.ascontiguousarray(img.transpose(0, 2, 1))).transpose(1, 2).requires_grad_(True)
    b = _t(np.ascontiguousarray(gt.transpose(0, 2, 1))).transpose(1, 2)
    assert not a.is_contiguous() and not b.is_contiguous()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = il.image_loss(a, b, ic.LAMBDA)
        out[0].backward()
    side.synchronize()
    for x, y in zip(want, [t.detach() for t in out] + [a.grad]):
        assert torch.equal(x, y)


# ---- the chain render -> loss -> backward ---------------------------------------------------------------------------------------------------

def test_chain_with_the_rasteriser(il):
    """image_loss on (render * mask).clip(0, 1) and one backward() against two explicit steps: d_img from image_loss on the
    detached image, then torch.autograd.grad of the image with it.  The smallest scene of tests/raster_scenes.py."""
    import torch
    from mpmavatar_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    cam, sc, r64, r32 = rs.twins("odd", 33, 17)
    rng = np.random.default_rng(4)
    gt = _t(np.clip(r32.image + 0.1 * rng.standard_normal(r32.image.shape), 0, 1).astype(np.float32))
    st = GaussianRasterizationSettings(image_height=cam.image_height, image_width=cam.image_width, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy,
                                       bg=_t(rs.BG), scale_modifier=1.0, viewmatrix=_t(cam.viewmatrix), projmatrix=_t(cam.projmatrix),
                                       sh_degree=0, campos=_t(np.asarray(cam.campos, np.float32)), prefiltered=False, debug=False)

    def picture():
        args = {k: _t(np.asarray(sc[k], np.float32), requires_grad=True) for k in ("means3D", "opacities", "colors_precomp", "scales", "rotations")}
        args.update(means2D=torch.zeros_like(args["means3D"], requires_grad=True), shs=None, cov3Ds_precomp=None)
        out = GaussianRasterizer(raster_settings=st)(**args)
        return (out[0] * out[3]).clip(0.0, 1.0), args

    pic, args = picture()
    assert tuple(pic.shape) == tuple(gt.shape) == (3, 33, 17)
    il.image_loss(pic, gt, ic.LAMBDA)[0].backward()
    one = args["means3D"].grad
    pic2, args2 = picture()
    assert torch.equal(pic, pic2)
    leaf = pic2.detach().requires_grad_(True)
    il.image_loss(leaf, gt, ic.LAMBDA)[0].backward()
    (two,) = torch.autograd.grad(pic2, args2["means3D"], grad_outputs=leaf.grad)
    assert torch.isfinite(one).all() and one.abs().max() > 0
    assert torch.equal(one, two)


# ---- the evaluation loop --------------------------------------------------------------------------------------------------------------------

def test_app_eval_over_three_frames(il, tmp_path):
    img, gt = ic.case("ragged")
    H, W = img.shape[-2:]
    yy, xx = np.mgrid[0:H, 0:W]
    mask = _t((0.5 + 0.5 * np.cos(0.1 * yy) * np.sin(0.07 * xx))[None].astype(np.float32))
    frames = [_t(np.roll(img, k, axis=-1)) for k in range(3)]
    g = _t(gt)
    ev = il.AppEval()
    for f in frames:
        pair = ev.add_frame(f, g, mask)
        assert pair[0].is_cuda and pair[0].shape == () and pair[1].shape == ()
    path = ev.save(str(tmp_path))
    assert path.endswith("app_metric.npz")
    z = np.load(path, allow_pickle=False)
    assert sorted(z.files) == ["PSNR", "SSIM"] and z["PSNR"].shape == z["SSIM"].shape == (3,)
    for k, f in enumerate(frames):
        a, b = (f * mask).unsqueeze(0), (g * mask).unsqueeze(0)                      # eval.py:86-87
        assert z["PSNR"][k] == float(il.psnr(a, b)) and z["SSIM"][k] == float(il.ssim(a, b))
    assert z["PSNR"][0] > z["PSNR"][1]                                                # the frames differ
    assert ev.means() == (float(z["PSNR"].mean()), float(z["SSIM"].mean()))
    plain = il.AppEval()
    plain.add_frame(frames[0], g)                                                     # no mask
    assert plain.results()["SSIM"][0] == float(il.ssim(frames[0].unsqueeze(0), g.unsqueeze(0)))


# ---- errors ---------------------------------------------------------------------------------------------------------------------------------

def test_bad_inputs_raise(il):
    import torch
    img, gt = ic.case("one_tile")
    a, b = _t(img), _t(gt)
    for fn in (il.l1_loss, il.ssim, il.psnr, il.image_loss):
        with pytest.raises(RuntimeError):
            fn(torch.tensor(img), torch.tensor(gt))                                   # CPU tensors
        with pytest.raises(RuntimeError):
            fn(a.double(), b.double())                                                # fp64
        with pytest.raises(RuntimeError):
            fn(a, b.clone().requires_grad_(True))                                     # no silent None for the second argument
        with pytest.raises(RuntimeError):
            fn(a, b[:, :8])                                                           # shapes differ
    with pytest.raises(ValueError):
        il.ssim(a, b, window_size=7)


def test_abi_refuses_null_and_empty(il):
    """valid calls that are refused: MPMHIP_ERR_INVALID and nothing launched"""
    import torch
    from mpmavatar_amd import _lib as L
    lib = L.load()
    img, gt = (_t(a) for a in ic.case("one_tile"))
    planes, H, W = img.shape
    dev = _dev()
    scratch = torch.full((il.scratch_doubles(planes, H, W),), -7.0, dtype=torch.float64, device=dev)
    out = torch.full((planes, 3), -7.0, device=dev)
    maps = torch.full((planes, 3, H, W), -7.0, device=dev)
    d_img = torch.full((planes, H, W), -7.0, device=dev)
    g = torch.ones(planes, device=dev)
    p = lambda t: None if t is None else t.data_ptr()

    def fwd(img_=img, gt_=gt, planes_=planes, H_=H, W_=W, maps_=maps, scratch_=scratch, out_=out):
        return lib.mpmhip_image_loss_forward(0, None, p(img_), p(gt_), planes_, H_, W_, p(maps_), p(scratch_), p(out_))

    def bwd(img_=img, gt_=gt, planes_=planes, H_=H, W_=W, maps_=maps, g1=g, g2=g, g3=g, d_=d_img):
        return lib.mpmhip_image_loss_backward(0, None, p(img_), p(gt_), planes_, H_, W_, p(maps_), p(g1), p(g2), p(g3), p(d_))

    for kw in (dict(img_=None), dict(gt_=None), dict(scratch_=None), dict(out_=None), dict(H_=0), dict(W_=0), dict(planes_=0), dict(H_=-1),
               dict(planes_=2 ** 15, H_=2 ** 8, W_=2 ** 8)):
        assert fwd(**kw) == L.ERR_INVALID, kw
    for kw in (dict(img_=None), dict(gt_=None), dict(maps_=None), dict(g1=None), dict(g2=None), dict(g3=None), dict(d_=None), dict(H_=0),
               dict(planes_=2 ** 15, H_=2 ** 8, W_=2 ** 8)):
        assert bwd(**kw) == L.ERR_INVALID, kw
    torch.cuda.synchronize()
    for t in (scratch, out, maps, d_img):
        assert (t == -7).all()                                                        # nothing was launched
    assert fwd() == L.OK and bwd() == L.OK and fwd(maps_=None) == L.OK                # the controls; maps may be NULL
    torch.cuda.synchronize()
    for t in (out, maps, d_img):
        assert torch.isfinite(t).all() and (t != -7).all()


# ---- the flat-region statement: documented, not bounded ---------------------------------------------------------------------------------------

def test_flat_region_agrees_with_the_host(il):
    import torch
    img, gt = ic.GOLD["flat_img"], ic.GOLD["flat_gt"]
    a = _t(img, requires_grad=True)
    s = il.ssim(a, _t(gt))
    s.backward()
    host = float(ic.host_forward(img, gt, want_maps=False)[0][0, 2])
    print("flat: gpu %.7f, host %.7f, reference fp32 %.7f, fp64 %.7f" % (float(s), host, float(ic.GOLD["flat_ssim_32"]), float(ic.GOLD["flat_ssim_64"])))
    assert torch.isfinite(s) and torch.isfinite(a.grad).all()
    assert 0.9999 < float(s) <= 1.0
    assert abs(float(s) - host) <= 1e-5
