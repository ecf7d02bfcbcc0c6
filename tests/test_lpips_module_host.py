"""The Python side of LPIPS without a GPU: the reference's two import lines through mpmavatar_amd/compat, the module's state dict
(the reference's 33 keys, shapes and order, all frozen), from_checkpoints over two files written here with the upstream key names,
the refusals, and AppEval without a module."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import lpips_twin_torch as tw
from mpmavatar_amd import build as hipbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "lpips.npz")

# train_appearance.py:30 and eval.py:14, verbatim
CHECK = '''
from lpipsPyTorch.modules.lpips import LPIPS
from lpipsPyTorch import lpips
import mpmavatar_amd.lpips as mine
assert issubclass(LPIPS, mine.LPIPS) and lpips is mine.lpips
import torch
for make in (lambda: LPIPS("vgg"), lambda: lpips(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16), net_type="vgg")):
    try:
        make()
    except RuntimeError as e:
        assert "MPMHIP_LPIPS_VGG16" in str(e) and "MPMHIP_LPIPS_LIN" in str(e), e
    else:
        raise SystemExit("no weights named and nothing raised")
try:
    LPIPS()                                     # the reference's default is 'alex'
except NotImplementedError as e:
    assert "net_type" in str(e)
else:
    raise SystemExit("net_type 'alex' accepted")
print("ok")
'''


@pytest.fixture(scope="module", autouse=True)
def lib():
    hipbuild.build()


def test_reference_import_lines_resolve_unchanged(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("MPMHIP_LPIPS_VGG16", "MPMHIP_LPIPS_LIN")}
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "mpmavatar_amd", "compat")])
    r = subprocess.run([sys.executable, "-c", CHECK], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


def test_state_dict_is_the_references():
    from mpmavatar_amd.lpips import LPIPS
    net, g = LPIPS(), np.load(GOLD)
    listed = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    assert listed == tw.state_shapes() and [k for k, _ in listed] == list(g["names"])
    assert [",".join(map(str, s)) for _, s in listed] == list(g["shapes"])
    assert len(list(net.parameters())) == 31 and not any(p.requires_grad for p in net.parameters())
    assert [k for k, _ in net.named_buffers()] == ["net.mean", "net.std"]
    assert torch.equal(net.net.mean.flatten(), torch.tensor(tw.MEAN)) and torch.equal(net.net.std.flatten(), torch.tensor(tw.STD))
    for bad in ("alex", "squeeze"):
        with pytest.raises(NotImplementedError, match="net_type"):
            LPIPS(bad)
    with pytest.raises(RuntimeError, match="no weights loaded"):
        net(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16))


def test_from_checkpoints_round_trips_two_files(tmp_path, monkeypatch):
    from mpmavatar_amd.lpips import LPIPS
    gen = torch.Generator().manual_seed(5)
    vgg = {"classifier.0.weight": torch.randn(4, 4, generator=gen), "classifier.0.bias": torch.randn(4, generator=gen)}
    want = {}
    for at, (cin, cout) in zip(tw.CONV_AT, tw.CHANNELS):
        vgg[f"features.{at}.weight"] = want[f"net.layers.{at}.weight"] = torch.randn(cout, cin, 3, 3, generator=gen)
        vgg[f"features.{at}.bias"] = want[f"net.layers.{at}.bias"] = torch.randn(cout, generator=gen)
    lin = {}
    for i, c in enumerate(tw.TAP_CHANNELS):
        lin[f"lin{i}.model.1.weight"] = want[f"lin.{i}.1.weight"] = torch.rand(1, c, 1, 1, generator=gen)
    torch.save(vgg, tmp_path / "vgg16.pth")
    torch.save(lin, tmp_path / "vgg.pth")
    net = LPIPS.from_checkpoints(str(tmp_path / "vgg16.pth"), str(tmp_path / "vgg.pth"))
    state = net.state_dict()
    assert net._loaded and len(state) == 33 and not any(k.startswith("classifier") for k in state)
    for k, v in want.items():
        assert torch.equal(state[k], v), k
    other = LPIPS()
    other.load_state_dict(state)                               # and on between two modules, as between this one and the reference's
    assert other._loaded and all(torch.equal(a, b) for a, b in zip(other.state_dict().values(), state.values()))
    monkeypatch.setenv("MPMHIP_LPIPS_VGG16", str(tmp_path / "vgg16.pth"))
    monkeypatch.setenv("MPMHIP_LPIPS_LIN", str(tmp_path / "vgg.pth"))
    assert torch.equal(LPIPS.from_environment().state_dict()["lin.3.1.weight"], want["lin.3.1.weight"])
    del vgg["features.17.bias"]
    torch.save(vgg, tmp_path / "short.pth")
    with pytest.raises(KeyError, match="features.17.bias"):
        LPIPS.from_checkpoints(str(tmp_path / "short.pth"), str(tmp_path / "vgg.pth"))


def test_unset_environment_names_both_variables(monkeypatch):
    from mpmavatar_amd.lpips import LPIPS, lpips
    monkeypatch.delenv("MPMHIP_LPIPS_VGG16", raising=False)
    monkeypatch.setenv("MPMHIP_LPIPS_LIN", "somewhere.pth")
    for make in (LPIPS.from_environment, lambda: lpips(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16), net_type="vgg")):
        with pytest.raises(RuntimeError) as e:
            make()
        assert "MPMHIP_LPIPS_VGG16" in str(e.value) and "MPMHIP_LPIPS_LIN" in str(e.value)


def test_app_eval_without_a_module_has_no_lpips_key(tmp_path):
    from mpmavatar_amd.image_loss import AppEval
    ev = AppEval()
    assert ev.lpips is None and sorted(ev.results()) == ["PSNR", "SSIM"]
    assert sorted(np.load(ev.save(str(tmp_path)))) == ["PSNR", "SSIM"]
    assert list(AppEval(lpips=object()).results()) == ["LPIPS", "PSNR", "SSIM"]       # the order of eval.py:59
