"""LPIPS without a GPU: the fixture of the reference's own class (tests/golden/lpips.npz) and the twin (tests/lpips_twin_torch.py)
pinned against it, key list and shapes included; the measurement of S32, the constants the bounds are built on;
mpmavatar_amd/csrc/lpips_math.hpp compiled with g++ (tests/hostlpips/hostlpips.cpp: serial loops that mirror every kernel in its K
order) against the fixture on the three cases; the saved maps, the backward layout and the pooling route on their own; and the same
file as a stand-alone program under AddressSanitizer and UBSan.  Every comparison prints its figures before it asserts (-s)."""
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_cases as lc
import lpips_twin_torch as tw


@pytest.mark.parametrize("name", lc.CASES)
def test_twin_reproduces_the_reference(name):
    g, t, f = np.load(lc.GOLD), lc.t64(name), lc.fixture(name)
    listed = tw.state_shapes()
    assert list(g["names"]) == [k for k, _ in listed] and len(listed) == 33
    assert list(g["shapes"]) == [",".join(map(str, s)) for _, s in listed]
    assert [(k, v.shape) for k, v in lc.weights().items()] == listed
    for q in ("out", "dx"):
        err = lc.rel(t[q], f[q])
        print(name, q, "twin against the fixture %.3g" % err)
        assert err < 1e-12


def test_twin_against_central_differences():
    """an anchor independent of autograd: central differences of the float64 twin on three pixels of `tiny`"""
    name = "tiny"
    c, p, g = lc.case(name), lc.params(), lc.t64(name)["dx"]
    y = torch.tensor(c["y"], dtype=torch.float64)
    h = 1e-6
    for at in [(0, 0, 0, 0), (0, 1, 7, 9), (0, 2, 15, 15)]:
        x = torch.tensor(c["x"], dtype=torch.float64)
        x[at] += h
        up = float(tw.forward(p, x, y))
        x[at] -= 2 * h
        fd = (up - float(tw.forward(p, x, y))) / (2 * h)
        print(at, "autograd %.9g central difference %.9g" % (g[at], fd))
        assert abs(fd - g[at]) <= 1e-5 * np.abs(g).max()


@pytest.mark.parametrize("name", lc.CASES)
def test_s32_is_the_measurement(name):
    t64, threads = lc.t64(name), torch.get_num_threads()
    try:
        for n_threads in dict.fromkeys((threads, 1)):
            torch.set_num_threads(n_threads)
            t32 = lc.twin(name, torch.float32)
            for q in ("out", "dx"):
                err = lc.rel(t32[q], t64[q])
                print(name, q, "S32 measured %.4g on %d threads, committed %.4g" % (err, n_threads, lc.S32[name][q]))
                assert err <= lc.S32[name][q]
    finally:
        torch.set_num_threads(threads)
    assert all(lc.BOUND[name][q] == 10 * lc.S32[name][q] for q in ("out", "dx"))
    print(name, "decision margin over float32 error %.3g" % lc.decision_ratio(name))


@pytest.mark.parametrize("name", lc.CASES)
def test_host_against_the_fixture(name):
    got = lc.host_run(name)
    lc.report(name, got, lc.fixture(name), "host")
    assert np.array_equal(got["out"], got["out_quiet"])              # keeping nothing changes no bit


def test_host_saved_maps_and_live_fraction():
    """the thirteen saved maps of x against torch's float32 layers, and no dead tap: 30 - 80 % of the activations are live"""
    name = "odd"
    c, p, maps = lc.case(name), lc.params(torch.float32), lc.host_run(name)["maps"]
    v, i = (torch.tensor(c["x"]) - p["net.mean"]) / p["net.std"], 0
    for at in range(30):
        if at in tw.CONV_AT:
            v = F.relu(F.conv2d(v, p[f"net.layers.{at}.weight"], p[f"net.layers.{at}.bias"], padding=1))
            err = float(np.abs(maps[i] - v.numpy()).max() / v.abs().max())
            live = float((maps[i] > 0).mean())
            print("layer", i, "map error %.3g, live %.2f" % (err, live))
            assert err < 1e-5 and 0.3 < live < 0.8
            i += 1
        elif at in tw.POOL_AT:
            v = F.max_pool2d(v, 2, 2)


def test_backward_layout_is_the_transposed_convolution():
    """hlp_prepare's layout [cin][cout][3][3] is the weight of the convolution that computes the input gradient"""
    lib, keep = lc.host_lib(), []
    d = lc.host_desc(1, 16, 16, keep)
    lib.hlp_prepare(lc.C.byref(d))
    for i in (0, 4):
        w, back = keep[3 * i], keep[3 * i + 2]
        want = np.ascontiguousarray(np.flip(w, (2, 3)).transpose(1, 0, 2, 3))
        assert np.array_equal(back.reshape(want.shape), want)
        g = torch.randn(1, w.shape[0], 5, 4, generator=torch.Generator().manual_seed(i))
        dx = F.conv_transpose2d(g, torch.tensor(w), padding=1)
        assert torch.allclose(F.conv2d(g, torch.tensor(back.reshape(want.shape)), padding=1), dx, atol=1e-5)


def test_stand_alone_program_under_sanitizers():
    """prepare, two forward passes and a backward pass over exactly sized buffers at the sizes of `tiny` and `odd`, as a stand-alone
    program built with -fsanitize=address,undefined: an index past a map, a weight or a workspace section ends it with a report"""
    r = subprocess.run([lc.sanitizer_program()], capture_output=True, text=True, timeout=600)
    print(r.stdout.strip(), r.stderr.strip()[:2000])
    assert r.returncode == 0 and r.stdout.startswith("ok:"), (r.returncode, r.stderr[-2000:])
