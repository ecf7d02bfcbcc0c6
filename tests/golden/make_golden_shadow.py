"""Golden vectors for the shadow network FROM THE REFERENCE'S OWN CLASS (tests/golden/shadow_net.npz).

The reference's ``ShadowUNet`` (scene/shadow.py:14-181 over scene/network.py) is constructed and executed at generation time, in
float64 on the CPU; this script contains none of its text.  scene/network.py and scene/shadow.py are loaded by path behind a stub
``scene`` package, because scene/__init__.py pulls in ``plyfile``.  For each of the four small cases of tests/shadow_cases.py the
module is built with the case's arguments, its parameters are overwritten with the case's seeded values (the constructor's own leave
the map flat), and the file stores: the float32 inputs, the names and shapes of ``named_parameters()`` in order, the three outputs and
the gradient of every parameter under sum(w * shadow_map).  Data only: inputs and expected outputs.  A gradient is stored flattened;
one of more than 2,048 elements (the untied biases of `tiles`) is stored at every eighth element (shadow_cases.fixture_stride):
float64 noise does not compress, and the file has to stay below the fixtures beside it.
    python tests/golden/make_golden_shadow.py        (needs the reference checkout that make_golden_raster.py names)"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import shadow_cases as sc  # noqa: E402
from make_golden_raster import REF  # noqa: E402


def load_reference():
    pkg = types.ModuleType("scene")
    pkg.__path__ = [os.path.join(REF, "scene")]
    sys.modules["scene"] = pkg
    for name in ("network", "shadow"):
        spec = importlib.util.spec_from_file_location("scene." + name, os.path.join(REF, "scene", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["scene." + name] = mod
        spec.loader.exec_module(mod)
    return sys.modules["scene.shadow"].ShadowUNet


def main():
    ShadowUNet = load_reference()
    torch.set_default_dtype(torch.float64)
    out = {}
    for name in sc.SMALL:
        c, sh = sc.case(name), sc.shape(name)
        f64 = lambda k: torch.tensor(c[k], dtype=torch.float64)
        net = ShadowUNet(uv_size=sh["uv_size"], ao_mean=f64("ao_mean"), shadow_size=sh["shadow_size"], lrelu_slope=sc.SLOPE, beta=sc.BETA,
                         n_dims=sh["n_dims"], interp_mode="bilinear", biases=sh["biases"]).double()
        listed = [(k, tuple(p.shape)) for k, p in net.named_parameters()]
        assert [k for k, _ in listed] == sc.names(name), listed
        with torch.no_grad():
            for k, p in net.named_parameters():
                assert tuple(p.shape) == c[k].shape, (k, p.shape, c[k].shape)
                p.copy_(f64(k))
        res = net(f64("ao_map"))
        grads = torch.autograd.grad((f64("w") * res["shadow_map"]).sum(), [p for _, p in net.named_parameters()])
        for k in ("ao_map", "ao_mean", "w"):
            out[f"{name}/in/{k}"] = np.asarray(c[k])
        out[f"{name}/names"] = np.array([k for k, _ in listed])
        out[f"{name}/shapes"] = np.array([",".join(map(str, s)) for _, s in listed])
        for k in sc.OUTPUTS:
            if k == "ao_map" and res[k].shape == c[k].shape:
                assert np.array_equal(res[k].numpy(), c[k].astype(np.float64))        # not resized: the input itself, not stored again
                continue
            out[f"{name}/out/{k}"] = res[k].detach().numpy()
        for (k, _), g in zip(listed, grads):
            assert g.dtype == torch.float64 and float(g.abs().max()) > 0, k
            out[f"{name}/grad/{k}"] = g.numpy().reshape(-1)[::sc.fixture_stride(g.numel())]
        print(name, "shadow_map %.3f .. %.3f" % (float(res["shadow_map"].detach().min()), float(res["shadow_map"].detach().max())))
    path = os.path.join(HERE, "shadow_net.npz")
    np.savez_compressed(path, **out)
    print("shadow_net.npz: %d bytes, %d arrays" % (os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main()
