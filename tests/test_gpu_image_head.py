"""The image head on the GPU (mpmavatar_amd/image_head.py over csrc/image_head.hip) against the float64 twin of
tests/image_head_twin_torch.py on the cases of tests/image_head_cases.py, within BOUND = 10 * S32 on the image and all four
gradients; the quiet run; each input alone; the same bits twice; the evaluation side against float64 / numpy, exactly; the chain
rasteriser -> camera_image -> image_loss -> backward(); FusedAdam over [cam_m, cam_c]; and the example with --image-head.  Every
comparison prints its figures before it asserts (run with -s)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import image_head_cases as ic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = [(name, False) for name in ic.CASES] + [("last", True)]       # (case, cam_m and cam_c given as [3] with camera_idx None)
IDS = [name + ("_as_row" if row else "") for name, row in VARIANTS]


def _dev():
    import torch
    return torch.device("cuda:0")


def _leaves(c, as_row=False, requires=ic.GRADS):
    """the case's four tensors on the GPU (copies: the shared cases are read-only) and the camera index"""
    import torch
    t = {k: torch.tensor(np.asarray(c[k]), device=_dev()) for k in ic.GRADS}
    cam = c["cam"]
    if as_row:
        t["cam_m"], t["cam_c"], cam = t["cam_m"][cam].clone(), t["cam_c"][cam].clone(), None
    for k in requires:
        t[k].requires_grad_(True)
    return t, cam


def _run(c, as_row=False, requires=ic.GRADS):
    """forward and backward of sum(w * image) -> dict over TENSORS (numpy; None for a tensor that did not require grad)"""
    import torch
    from mpmavatar_amd.image_head import camera_image
    t, cam = _leaves(c, as_row, requires)
    image = camera_image(t["render"], t["mask"], t["cam_m"], t["cam_c"], cam)
    assert image.grad_fn is not None and image.is_contiguous() and image.shape == t["render"].shape
    (torch.tensor(c["w"], device=_dev()) * image).sum().backward()
    out = {"image": image.detach().cpu().numpy()}
    out.update({k: (None if t[k].grad is None else t[k].grad.cpu().numpy()) for k in ic.GRADS})
    return out


@pytest.mark.parametrize("name,as_row", VARIANTS, ids=IDS)
def test_against_the_float64_twin(name, as_row):
    import torch
    from mpmavatar_amd.image_head import camera_image
    c, want = ic.case(name), ic.t64(name)
    got = _run(c, as_row)
    for k in ic.TENSORS:
        w = want[k][c["cam"]] if as_row and k in ("cam_m", "cam_c") else want[k]
        err = ic.rel(got[k], w)
        print(name, k, "%.3g of bound %.3g" % (err, ic.BOUND))
        assert np.isfinite(got[k]).all() and err <= ic.BOUND, k
    if name == "edges":
        for y, x in ic.EDGE_ZERO + ic.EDGE_ONE:
            assert got["render"][0, y, x] != 0, (y, x)                  # the gradient passes at v == 0 and at v == 1
    if name == "dark":
        assert (got["image"] == 0).all() and (got["render"] == 0).all() and (got["mask"] != 0).any()
        assert (got["cam_m"] == 0).all() and (got["cam_c"] == 0).all()
    if name == "main":
        dark = c["mask"] == 0
        assert (got["render"][:, dark] == 0).all() and (got["mask"][dark] != 0).all()
    # the quiet runs: grad mode off, and nothing requiring grad -- the same bits, no graph
    t, cam = _leaves(c, as_row)
    with torch.no_grad():
        quiet = camera_image(t["render"], t["mask"], t["cam_m"], t["cam_c"], cam)
    t2, _ = _leaves(c, as_row, requires=())
    plain = camera_image(t2["render"], t2["mask"], t2["cam_m"], t2["cam_c"], cam)
    for im in (quiet, plain):
        assert im.grad_fn is None and not im.requires_grad and np.array_equal(im.cpu().numpy(), got["image"])


@pytest.mark.parametrize("name", ["main", "vec"])
def test_each_input_alone(name):
    """one input requiring grad: the others get None, the wanted one the bits of the run of all four"""
    c = ic.case(name)
    full = _run(c)
    for k in ic.GRADS:
        alone = _run(c, requires=(k,))
        assert all(alone[o] is None for o in ic.GRADS if o != k), k
        assert np.array_equal(alone[k], full[k]), k
        assert np.array_equal(alone["image"], full["image"])


@pytest.mark.parametrize("name", ["main", "vec"])
def test_same_bits_twice_and_dense_camera_gradients(name):
    c = ic.case(name)
    a, b = _run(c), _run(c)
    for k in ic.TENSORS:
        assert np.array_equal(a[k], b[k]), k
    n_cam, cam = c["cam_m"].shape[0], c["cam"]
    off = np.arange(n_cam) != cam
    for k in ("cam_m", "cam_c"):
        assert a[k].shape == (n_cam, 3) and (a[k][off] == 0).all() and (a[k][cam] != 0).all(), k


def test_arguments():
    import torch
    from mpmavatar_amd.image_head import camera_image
    t, cam = _leaves(ic.case("last"), requires=())
    r, m, cm, cc = t["render"], t["mask"], t["cam_m"], t["cam_c"]
    base = camera_image(r, m, cm, cc, cam)
    # mask as [1, H, W]; camera_idx as a CPU tensor; non-contiguous render and mask: the same bits, a contiguous result
    assert torch.equal(camera_image(r, m[None], cm, cc, torch.tensor(cam)), base)
    wide_r, wide_m = torch.zeros(3, 16, 40, device=_dev()), torch.zeros(16, 40, device=_dev())
    wide_r[:, :, ::2], wide_m[:, ::2] = r, m
    out = camera_image(wide_r[:, :, ::2], wide_m[:, ::2], cm, cc, cam)
    assert out.is_contiguous() and torch.equal(out, base)
    with pytest.raises(TypeError):
        camera_image(r, m, cm, cc, torch.tensor(cam, device=_dev()))
    for bad in (lambda: camera_image(r.double(), m, cm, cc, cam), lambda: camera_image(r.cpu(), m, cm, cc, cam),
                lambda: camera_image(r, m[:-1], cm, cc, cam), lambda: camera_image(r[:2], m, cm, cc, cam),
                lambda: camera_image(r, m, cm, cc[:-1], cam), lambda: camera_image(r, m, cm, cc, cm.shape[0]),
                lambda: camera_image(r, m, cm, cc, -1), lambda: camera_image(r, m, cm, cc, None),
                lambda: camera_image(r, m, cm[0], cc[0], 0), lambda: camera_image(r, m, cm, cc, 1.0)):
        with pytest.raises(RuntimeError):
            bad()
    nan = camera_image(torch.full_like(r, float("nan")), m, cm, cc, cam)
    assert torch.isnan(nan[:, m > 0]).all()


@pytest.mark.parametrize("name", ic.BYTE_CASES)
def test_frame_bytes(name):
    """every byte equals the floor of the float64 value, for both backgrounds, with the affine and without"""
    import torch
    from mpmavatar_amd.image_head import frame_bytes
    c = ic.case(name)
    t, cam = _leaves(c, requires=())
    for affine, white in ic.FRAME_FORMS:
        a = (t["cam_m"], t["cam_c"], cam) if affine else (None, None, None)
        got = frame_bytes(t["render"], t["mask"], *a, white)
        want = ic.bytes64(c, affine, white)
        assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape and got.is_contiguous()
        differ = int((got.cpu().numpy() != want).sum())
        print(name, "affine" if affine else "identity", "white" if white else "black", "%d of %d bytes differ" % (differ, want.size))
        assert differ == 0


@pytest.mark.parametrize("H,W", [(9, 7), (16, 16)], ids=["scalar", "vec"])
def test_compose_gt_and_eval_inputs_against_numpy(H, W):
    import torch
    from mpmavatar_amd.image_head import compose_gt, eval_inputs
    rng = np.random.default_rng(3)
    rgb, msk = rng.uniform(0, 1, (3, H, W)).astype(np.float32), rng.uniform(0, 1, (1, H, W)).astype(np.float32)
    for white in (False, True):
        got = compose_gt(torch.tensor(rgb, device=_dev()), torch.tensor(msk, device=_dev()), white)
        assert got.shape == (3, H, W) and not got.requires_grad and np.array_equal(got.cpu().numpy(), ic.numpy_compose(rgb, msk, white))
    pred, gt, mask = ic.eval_frames(H, W)
    if (H, W) == (16, 16):                                # all 256 byte values, in both images: the true division by 255
        pred = (np.arange(256 * 3).reshape(16, 16, 3) % 256).astype(np.uint8)
        gt = pred[::-1].copy()
    for remove_white in (False, True):
        a, b = eval_inputs(torch.tensor(pred, device=_dev()), torch.tensor(gt, device=_dev()), torch.tensor(mask, device=_dev()), remove_white)
        want_a, want_b = ic.numpy_eval_pair(pred, gt, mask, remove_white)
        assert a.shape == b.shape == (1, 3, H, W) and a.is_contiguous() and b.is_contiguous()
        assert np.array_equal(a[0].cpu().numpy(), want_a) and np.array_equal(b[0].cpu().numpy(), want_b)
    ones = torch.ones(16, 16, device=_dev())
    if (H, W) == (16, 16):
        a, _ = eval_inputs(torch.tensor(pred, device=_dev()), torch.tensor(gt, device=_dev()), ones, False)
        assert np.array_equal(a[0].cpu().numpy(), pred.astype(np.float32).transpose(2, 0, 1) / np.float32(255.))


def test_eval_inputs_feed_app_eval():
    """frame_bytes -> eval_inputs -> AppEval.add_frame, nothing leaving the device: finite metrics, the PSNR of a frame against
    itself infinite"""
    import torch
    from mpmavatar_amd.image_head import eval_inputs, eval_mask, frame_bytes
    from mpmavatar_amd.image_loss import AppEval
    c = ic.case("vec")
    t, cam = _leaves(c, requires=())
    pred = frame_bytes(t["render"], t["mask"], t["cam_m"], t["cam_c"], cam, True)
    gt = frame_bytes(t["render"].clamp(0, 1), t["mask"], None, None, None, True)
    solid = torch.zeros_like(t["mask"])
    solid[4:44, 6:58] = 1.0                                 # a solid region: five erosions leave its inside
    m = eval_mask(solid)
    assert m.shape == t["mask"].shape and m.is_cuda and float(m.max()) == 1.0 and float(m[0, 0]) == 0.0
    ev = AppEval()
    psnr, ssim = ev.add_frame(*eval_inputs(pred, gt, m, True))
    same = ev.add_frame(*eval_inputs(pred, pred, m, True))
    assert torch.isfinite(psnr) and 0 < float(ssim) < 1 and torch.isinf(same[0]) and abs(float(same[1]) - 1) < 1e-6


# ---- the chain: rasteriser -> camera_image -> image_loss -> backward() -----------------------------------------------------------------

def _chain(detach_alpha=False):
    import torch
    import raster_scenes as rs
    import raster_twin as rtw
    from mpmavatar_amd.image_head import camera_image
    from mpmavatar_amd.image_loss import image_loss
    from mpmavatar_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    dev = _dev()
    cam = rtw.simple_camera(32, 32)
    sc = rs.random_scene(cam, 0, n=50, centre=(16.0, 16.0))
    f = lambda a: torch.tensor(np.asarray(a, np.float32), device=dev)
    st = GaussianRasterizationSettings(image_height=32, image_width=32, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=f(rs.BG), scale_modifier=1.0,
                                       viewmatrix=f(cam.viewmatrix), projmatrix=f(cam.projmatrix), sh_degree=0, campos=f(cam.campos),
                                       prefiltered=False, debug=False)
    args = {k: f(v).requires_grad_(True) for k, v in sc.items()}
    args["means2D"] = torch.zeros_like(args["means3D"], requires_grad=True)
    image, _, _, alpha, radii, _ = GaussianRasterizer(raster_settings=st)(**args)
    image.retain_grad()
    alpha.retain_grad()
    cam_m = torch.tensor([[0.0, 0.0, 0.0], [0.9, 0.8, 1.0]], device=dev, requires_grad=True)
    cam_c = torch.tensor([[0.0, 0.0, 0.0], [0.02, -0.01, 0.03]], device=dev, requires_grad=True)
    head = camera_image(image, alpha.detach() if detach_alpha else alpha, cam_m, cam_c, 1)
    head.retain_grad()
    gt = f(np.random.default_rng(9).uniform(0, 1, (3, 32, 32)))
    loss = image_loss(head, gt, 0.2)[0]
    loss.backward()
    return dict(image=image, alpha=alpha, head=head, cam_m=cam_m, cam_c=cam_c, opacities=args["opacities"], loss=loss)


def test_chain_through_the_rasteriser_and_the_image_loss():
    import torch
    import image_head_twin_torch as tw
    a, b, d = _chain(), _chain(), _chain(detach_alpha=True)
    for k in ("image", "alpha", "cam_m", "cam_c", "opacities"):
        assert torch.equal(a[k].grad, b[k].grad), k                      # two runs: the same bits
    assert torch.equal(a["head"], b["head"]) and torch.equal(a["loss"], b["loss"])
    # the head's own gradients against the twin, fed the same inputs and the same upstream
    t = {k: a[k].detach().double().cpu().requires_grad_(True) for k in ("image", "alpha", "cam_m", "cam_c")}
    v = tw.unclipped(t["image"], t["alpha"], t["cam_m"], t["cam_c"], 1)
    vn, an = v.detach().numpy(), a["alpha"].detach().cpu().numpy()
    exact = np.broadcast_to(an == 0, vn.shape) & (vn == 0)
    dist = np.minimum(np.abs(vn), np.abs(vn - 1))[~exact].min()
    print("closest v to a clip bound %.3g; above 1: %.1f %%; alpha == 0 on %.1f %% of the pixels" % (dist, 100 * (vn > 1).mean(), 100 * (an == 0).mean()))
    assert dist > ic.CLIP_MARGIN and (vn > 1).any() and ((vn > 0) & (vn < 1)).any()
    want = torch.autograd.grad((a["head"].grad.double().cpu() * v.clip(0., 1.)).sum(), [t[k] for k in ("image", "alpha", "cam_m", "cam_c")])
    for k, w in zip(("image", "alpha", "cam_m", "cam_c"), want):
        err = ic.rel(a[k].grad.cpu().numpy(), w.numpy())
        print("chain", k, "%.3g of bound %.3g" % (err, ic.BOUND))
        assert err <= ic.BOUND, k
    assert ic.rel(a["head"].detach().cpu().numpy(), v.clip(0., 1.).detach().numpy()) <= ic.BOUND
    # the second path of the rasteriser's alpha
    g, g_detached = a["opacities"].grad, d["opacities"].grad
    assert torch.isfinite(g).all() and (g != 0).any() and torch.isfinite(g_detached).all() and not torch.equal(g, g_detached)
    assert d["alpha"].grad is None and torch.equal(d["head"], a["head"])


def test_fused_adam_moves_the_camera_row_only():
    import torch
    from mpmavatar_amd.optim import FusedAdam
    r = _chain()
    cam_m, cam_c = r["cam_m"], r["cam_c"]
    before = (cam_m.detach().clone(), cam_c.detach().clone())
    opt = FusedAdam([{"params": [cam_m, cam_c], "lr": 1e-3, "name": "cams"}], lr=0.0, eps=1e-15)
    opt.step()
    for p, b in zip((cam_m, cam_c), before):
        assert torch.equal(p.detach()[0], b[0]) and (p.detach()[1] != b[1]).all()
        st = opt.state[p]
        assert (st["exp_avg"][0] == 0).all() and (st["exp_avg_sq"][0] == 0).all() and (st["exp_avg"][1] != 0).all() and (st["exp_avg_sq"][1] != 0).all()


def test_example_with_the_image_head():
    """examples/appearance_train_demo.py --image-head --steps 5 --size 32 runs and prints a falling loss"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "appearance_train_demo.py"), "--image-head", "--steps", "5", "--size", "32"],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0, r.stderr[-3000:]
    losses = [float(line.split("loss")[1].split()[0]) for line in r.stdout.splitlines() if line.startswith("iteration")]
    assert len(losses) == 5 and all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert "camera_image" in r.stdout
