"""Golden vectors for LPIPS FROM THE REFERENCE'S OWN CLASS (tests/golden/lpips.npz).

The reference's ``LPIPS('vgg')`` (lpipsPyTorch/modules/{lpips,networks,utils}.py) is constructed and executed at generation time, in
float64 on the CPU; this script contains none of its text.  Its three modules are loaded by path behind two stand-ins:
``torchvision.models`` is a stub whose ``vgg16()`` is this project's own ``nn.Sequential`` of the standard VGG16 layout (plus a
``VGG16_Weights`` name), and ``torch.hub.load_state_dict_from_url`` returns the case's tap weights under the upstream keys
(``lin{i}.model.1.weight``), so that the reference's own renaming runs.  The convolution weights of tests/lpips_cases.py are then
loaded through the reference's ``state_dict()`` keys.  For each case the file stores the float32 inputs, ``out`` and d out / d x in
float64, and once the key list and shapes of the reference's ``state_dict()``.  Data only: inputs and expected outputs.
    python tests/golden/make_golden_lpips.py        (needs the reference checkout that make_golden_raster.py names)"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import lpips_cases as lc  # noqa: E402
from make_golden_raster import REF  # noqa: E402


def vgg16(weights=None):
    """torchvision's layout: features = conv/ReLU pairs with MaxPool2d(2, 2) after 2, 2, 3, 3, 3 of them"""
    layers, cin = [], 3
    for v in (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M"):
        if v == "M":
            layers.append(torch.nn.MaxPool2d(2, 2))
        else:
            layers += [torch.nn.Conv2d(cin, v, 3, padding=1), torch.nn.ReLU(inplace=True)]
            cin = v
    net = torch.nn.Module()
    net.features = torch.nn.Sequential(*layers)
    return net


def load_reference():
    models = types.ModuleType("torchvision.models")
    models.vgg16 = vgg16
    models.VGG16_Weights = types.SimpleNamespace(IMAGENET1K_V1="IMAGENET1K_V1")
    tv = types.ModuleType("torchvision")
    tv.models = models
    sys.modules["torchvision"], sys.modules["torchvision.models"] = tv, models
    taps = {f"lin{i}.model.1.weight": torch.tensor(lc.weights()[f"lin.{i}.1.weight"]) for i in range(5)}
    torch.hub.load_state_dict_from_url = lambda url, **kw: dict(taps)
    for pkg, path in (("lpipsPyTorch", "lpipsPyTorch"), ("lpipsPyTorch.modules", os.path.join("lpipsPyTorch", "modules"))):
        mod = types.ModuleType(pkg)
        mod.__path__ = [os.path.join(REF, path)]
        sys.modules[pkg] = mod
    for name in ("utils", "networks", "lpips"):
        spec = importlib.util.spec_from_file_location("lpipsPyTorch.modules." + name, os.path.join(REF, "lpipsPyTorch", "modules", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["lpipsPyTorch.modules." + name] = mod
        spec.loader.exec_module(mod)
    return sys.modules["lpipsPyTorch.modules.lpips"].LPIPS


def main():
    LPIPS = load_reference()
    net = LPIPS("vgg")
    listed = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    for i in range(5):                                                   # the reference's renaming has run on the tap weights
        assert torch.equal(net.state_dict()[f"lin.{i}.1.weight"], torch.tensor(lc.weights()[f"lin.{i}.1.weight"]))
    net.load_state_dict({k: torch.tensor(v) for k, v in lc.weights().items()})
    net = net.double()
    assert not any(p.requires_grad for p in net.parameters())
    out = {"names": np.array([k for k, _ in listed]), "shapes": np.array([",".join(map(str, s)) for _, s in listed])}
    for name in lc.CASES:
        c = lc.case(name)
        x = torch.tensor(c["x"], dtype=torch.float64, requires_grad=True)
        res = net(x, torch.tensor(c["y"], dtype=torch.float64))
        dx, = torch.autograd.grad(res.sum(), x)
        assert res.shape == (1, 1, 1, 1) and bool(torch.isfinite(dx).all()) and float(dx.abs().max()) > 0
        out[f"{name}/in/x"], out[f"{name}/in/y"] = np.asarray(c["x"]), np.asarray(c["y"])
        out[f"{name}/out"], out[f"{name}/dx"] = res.detach().numpy(), dx.numpy()
        print(name, "out %.6f  max |dx| %.3e" % (float(res.detach()), float(dx.abs().max())))
    path = os.path.join(HERE, "lpips.npz")
    np.savez_compressed(path, **out)
    print("lpips.npz: %d bytes, %d arrays" % (os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main()
