"""LPIPS on the GPU: mpmavatar_amd.lpips.LPIPS under torch autograd (csrc/lpips.hip) against the fixture of the reference's own class
(tests/golden/lpips.npz) within BOUND = 10 * S32 per case and quantity (tests/lpips_cases.py, measured on the CPU), and the
properties the module promises: the same bits on every run, the graph rules, the input forms, the sum over the batch, the state dict,
the evaluation's third key and the chain with image_loss.  Every comparison prints its figures before it asserts (-s).

Against the host restatement (tests/hostlpips/hostlpips.cpp), which walks K in the kernel's order with fmaf: on the MI355X `out` and
`dx` of all three cases came out bit for bit equal to it, so test_device_equals_the_host_restatement asserts that."""
import numpy as np
import pytest
import torch

import lpips_cases as lc
import lpips_twin_torch as tw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def net():
    from mpmavatar_amd.lpips import LPIPS
    m = LPIPS("vgg")
    m.load_state_dict({k: torch.tensor(v) for k, v in lc.weights().items()})
    return m.to(DEV)


def _run(net, name, images=None):
    """-> ({"out", "dx"} as numpy, the output tensor)"""
    c = lc.case(name)
    sel = slice(None) if images is None else images
    x = torch.tensor(c["x"][sel], device=DEV, requires_grad=True)
    out = net(x, torch.tensor(c["y"][sel], device=DEV))
    out.sum().backward()
    return {"out": out.detach().cpu().numpy(), "dx": x.grad.cpu().numpy()}, out


@pytest.fixture(scope="module")
def runs(net):
    """one run of every case, shared by the tests that only compare"""
    return {name: _run(net, name) for name in lc.CASES}


@pytest.mark.parametrize("name", lc.CASES)
def test_against_the_fixture(runs, name):
    got, out = runs[name]
    assert out.shape == (1, 1, 1, 1) and out.grad_fn is not None and got["dx"].shape == lc.case(name)["x"].shape
    lc.report(name, got, lc.fixture(name), "gpu")


@pytest.mark.parametrize("name", lc.CASES)
def test_device_equals_the_host_restatement(runs, name):
    """the MFMA is an fmaf chain in k order, and the restatement walks K in that order"""
    got, host = runs[name][0], lc.host_run(name)
    for q in ("out", "dx"):
        same = np.array_equal(got[q], host[q])
        print(name, q, "device == host restatement:", same, "" if same else "largest difference %.3g" % lc.rel(got[q], host[q]))
    assert all(np.array_equal(got[q], host[q]) for q in ("out", "dx"))


@pytest.mark.parametrize("name", ["odd", "tiles"])
def test_two_runs_give_the_same_bits(net, runs, name):
    again, _ = _run(net, name)
    for q in ("out", "dx"):
        assert np.array_equal(again[q], runs[name][0][q]), q


def test_graph_rules_and_input_forms(net, runs):
    name = "tiny"
    c, base = lc.case(name), runs[name][0]
    x, y = torch.tensor(c["x"], device=DEV), torch.tensor(c["y"], device=DEV)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with torch.no_grad():
        quiet = net(x.clone().requires_grad_(True), y)
    torch.cuda.synchronize()
    assert quiet.grad_fn is None and not quiet.requires_grad and np.array_equal(quiet.cpu().numpy(), base["out"])
    assert torch.cuda.memory_allocated() - before <= 512          # the output alone: no workspace is retained
    plain = net(x, y)                                             # an x that needs no grad
    assert plain.grad_fn is None and np.array_equal(plain.cpu().numpy(), base["out"])
    x3 = x[0].clone().requires_grad_(True)                        # [3, H, W] counts as N = 1
    out3 = net(x3, y[0])
    out3.sum().backward()
    assert out3.shape == (1, 1, 1, 1) and np.array_equal(out3.detach().cpu().numpy(), base["out"])
    assert np.array_equal(x3.grad.cpu().numpy(), base["dx"][0])
    with pytest.raises(RuntimeError, match="y must not require grad"):
        net(x, y.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="16 <= H, W"):
        net(x[..., :15, :], y[..., :15, :])
    with pytest.raises(RuntimeError, match="same shape"):
        net(x, torch.zeros(1, 3, 16, 20, device=DEV))
    from mpmavatar_amd.lpips import LPIPS
    with pytest.raises(RuntimeError, match="no weights loaded"):
        LPIPS().to(DEV)(x, y)


def test_batch_is_summed_not_averaged(net, runs):
    """`odd` (N = 2) is the sum of its two images run alone, and its dx the two gradients"""
    name = "odd"
    both, alone = runs[name][0], [_run(net, name, slice(i, i + 1))[0] for i in range(2)]
    want = {"out": alone[0]["out"].astype(np.float64) + alone[1]["out"], "dx": np.concatenate([alone[0]["dx"], alone[1]["dx"]])}
    lc.report(name, both, want, "batch against its images alone")
    lc.report(name, {"out": want["out"], "dx": want["dx"]}, lc.fixture(name), "images alone against the fixture")


def test_load_state_dict_from_the_twin_and_its_float32_run_on_the_device(runs):
    """a state dict with the reference's keys goes in; the twin's own float32 run on the same device agrees within BOUND"""
    from mpmavatar_amd.lpips import LPIPS
    name = "tiles"
    fresh = LPIPS()
    result = fresh.load_state_dict(lc.params(torch.float32))
    assert not result.missing_keys and not result.unexpected_keys
    got, _ = _run(fresh.to(DEV), name)
    assert all(np.array_equal(got[q], runs[name][0][q]) for q in ("out", "dx"))
    t32 = lc.twin(name, torch.float32, DEV)
    lc.report(name, got, t32, "module against the twin's float32 run on the device")
    back = {k: v.cpu() for k, v in fresh.state_dict().items()}            # and out again, into the twin
    assert float(tw.forward(back, torch.tensor(lc.case(name)["x"]), torch.tensor(lc.case(name)["y"]))) > 0


def test_backward_layouts_follow_the_weights(net):
    """a weight changed in place is seen by the next backward pass (the layouts are rebuilt on a new _version)"""
    from mpmavatar_amd.lpips import LPIPS
    name = "tiny"
    mine = LPIPS()
    mine.load_state_dict({k: torch.tensor(v) for k, v in lc.weights().items()})
    mine = mine.to(DEV)
    first, _ = _run(mine, name)
    with torch.no_grad():
        mine.net.layers.get_submodule("5").weight.mul_(0.5)
    second, _ = _run(mine, name)
    c, p = lc.case(name), {k: v.detach().clone() for k, v in mine.state_dict().items()}
    x = torch.tensor(c["x"], device=DEV, requires_grad=True)
    tw.forward(p, x, torch.tensor(c["y"], device=DEV)).sum().backward()
    assert not np.array_equal(first["dx"], second["dx"])
    err = lc.rel(second["dx"], x.grad.cpu().numpy())
    print("dx after an in-place change against the twin on the device %.3g" % err)
    assert err <= lc.BOUND[name]["dx"]


def test_app_eval_writes_the_three_keys(net, tmp_path):
    from mpmavatar_amd.image_loss import AppEval
    c = lc.case("tiles")
    x, y = torch.tensor(c["x"][0], device=DEV), torch.tensor(c["y"][0], device=DEV)
    mask = torch.ones(1, *x.shape[1:], device=DEV)
    mask[:, :10] = 0.5
    ev = AppEval(lpips=net)
    triple = ev.add_frame(x, y, mask)
    ev.add_frame(x, y)
    assert len(triple) == 3 and all(t.dim() == 0 and t.is_cuda for t in triple)
    saved = np.load(ev.save(str(tmp_path)))
    assert list(saved) == ["LPIPS", "PSNR", "SSIM"] and all(saved[k].shape == (2,) and saved[k].dtype == np.float64 for k in saved)
    assert saved["LPIPS"][1] == float(net(x[None], y[None])) and saved["LPIPS"][0] == float(net((x * mask)[None], (y * mask)[None]))
    plain = AppEval()
    assert len(plain.add_frame(x, y)) == 2 and list(plain.results()) == ["PSNR", "SSIM"]


def test_chain_with_image_loss(net):
    """image_loss(image, gt)[0] + 0.1 * net(image[None], gt[None]) over a leaf image: the gradient is the sum of the two gradients
    taken separately, within the sum of their bounds (fp32 addition of the two maps: one rounding, 6e-8 of the larger)"""
    from mpmavatar_amd.image_loss import image_loss
    c = lc.case("tiles")
    gt = torch.tensor(c["y"][0], device=DEV)

    def grad(f):
        image = torch.tensor(c["x"][0], device=DEV, requires_grad=True)
        f(image).sum().backward()
        return image.grad.double().cpu().numpy()

    a = grad(lambda im: image_loss(im, gt)[0])
    b = grad(lambda im: 0.1 * net(im[None], gt[None]))
    both = grad(lambda im: image_loss(im, gt)[0] + 0.1 * net(im[None], gt[None]))
    err = np.abs(both - (a + b)).max()
    bound = 1e-7 * np.abs(a).max() + lc.BOUND["tiles"]["dx"] * np.abs(b).max()
    print("chain: largest difference %.3g of bound %.3g; max |d image_loss| %.3g, max |d 0.1 lpips| %.3g" % (err, bound, np.abs(a).max(), np.abs(b).max()))
    assert np.abs(b).max() > 0 and err <= bound
