"""The shadow network without a GPU: the twin (tests/shadow_twin_torch.py) pinned against the reference's own ShadowUNet
(tests/golden/shadow_net.npz), names, shapes and order included; a central-difference spot check of the twin; the measurement of S32,
the constants the bounds are built on; mpmavatar_amd/csrc/shadow_math.hpp compiled with g++ (tests/hostshadow/hostshadow.cpp: serial
loops that mirror every forward and backward stage, tables included) against the float64 twin on the four small cases; the index
rules and the inverse tables against torch and a brute-force walk; frozen parameters; and the same file as a stand-alone program
under AddressSanitizer and UBSan.  Every comparison prints its figures before it asserts (run with -s)."""
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import shadow_cases as sc
import shadow_twin_torch as tw

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shadow_net.npz")


# ---- the twin is the reference -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sc.SMALL)
def test_twin_reproduces_the_reference(name):
    """the reference's own class in float64 on the inputs of the case -- which are the fixture's own, bit for bit -- with its
    named_parameters() in order"""
    g, c, t = np.load(GOLD), sc.case(name), sc.t64(name)
    for k in ("ao_map", "ao_mean", "w"):
        assert np.array_equal(g[f"{name}/in/{k}"], c[k]) and g[f"{name}/in/{k}"].dtype == np.float32, k
    sh = sc.shape(name)
    listed = tw.param_shapes(sh["shadow_size"], sh["n_dims"], sh["biases"])
    assert list(g[f"{name}/names"]) == [k for k, _ in listed] == sc.names(name)
    assert list(g[f"{name}/shapes"]) == [",".join(map(str, s)) for _, s in listed]
    for k in sc.OUTPUTS:
        ref = g[f"{name}/out/{k}"] if f"{name}/out/{k}" in g else c[k].astype(np.float64)
        err = sc.rel(t[k], ref)
        print(name, k, "twin against the fixture %.3g" % err)
        assert ref.dtype == np.float64 and err < 1e-12, k
    for k in sc.names(name):
        ref = g[f"{name}/grad/{k}"]
        mine = t[k].reshape(-1)[::sc.fixture_stride(t[k].size)]
        err = sc.rel(mine, ref)
        print(name, k, "twin against the fixture %.3g" % err)
        assert ref.dtype == np.float64 and np.abs(ref).max() > 0 and err < 1e-12, k


def test_twin_against_central_differences():
    """an anchor independent of autograd: central differences of the float64 twin's loss on one weight_v, one weight_g and one untied
    bias texel"""
    name = "odd"
    c, sh, g = sc.case(name), sc.shape(name), sc.t64(name)
    f = lambda k: torch.tensor(c[k], dtype=torch.float64)

    def loss(p):
        return float((f("w") * tw.forward(p, f("ao_map"), f("ao_mean"), sh["shadow_size"], sh["uv_size"], sc.SLOPE, sc.BETA)[0]).sum())

    h = 1e-6
    for k, at in [("enc_layers.1.0.weight_v", (2, 1, 0, 2)), ("dec_layers.2.0.weight_g", (3, 0, 0, 0)), ("enc_layers.2.0.bias", (1, 3, 4)),
                  ("shadow_pred.bias", (0,))]:
        p = {n: f(n) for n in sc.names(name)}
        p[k][at] += h
        up = loss(p)
        p[k][at] -= 2 * h
        fd = (up - loss(p)) / (2 * h)
        print(k, at, "autograd %.9g central difference %.9g" % (g[k][at], fd))
        assert abs(fd - g[k][at]) <= 1e-6 * max(1.0, abs(g[k][at]))


# ---- the yardstick -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sc.CASES)
def test_s32_is_the_measurement(name):
    t64, threads = sc.t64(name), torch.get_num_threads()
    try:
        for n_threads in dict.fromkeys((threads, 1)):                       # a batch is summed in an order that depends on the threads
            torch.set_num_threads(n_threads)
            t32 = sc.twin(name, torch.float32)
            errs = {k: sc.rel(t32[k], t64[k]) for k in t64}
            worst = max(errs, key=errs.get)
            print(name, "S32 measured %.4g (%s) on %d threads, committed %.4g" % (errs[worst], worst, n_threads, sc.S32[name]))
            assert errs[worst] <= sc.S32[name]
    finally:
        torch.set_num_threads(threads)
    assert sc.BOUND[name] == 10 * sc.S32[name]
    assert all(np.abs(t64[k]).max() > 0 for k in sc.names(name))           # no parameter has a zero gradient
    assert t64["shadow_map"].max() - t64["shadow_map"].min() > 0.1          # the map is not flat


# ---- the index rules and the tables --------------------------------------------------------------------------------------------------------

def test_index_rules_are_torchs():
    """nearest_src and bilinear_tap against F.interpolate on ramps and impulses, at every size pair the cases use and a few more"""
    lib = sc.host_lib()
    pairs = [(33, 20), (20, 10), (10, 5), (5, 2), (2, 5), (5, 10), (10, 20), (20, 24), (16, 12), (9, 4), (4, 2), (2, 1), (1, 2), (2, 4), (4, 9),
             (256, 128), (32, 64), (7, 8), (13, 8), (40, 40), (8, 1), (70, 33)]
    for n_in, n_out in pairs:
        ramp = torch.arange(n_in, dtype=torch.float32).reshape(1, 1, 1, n_in)
        near = F.interpolate(ramp.expand(1, 1, 2, n_in), size=(2, n_out))[0, 0, 0].numpy()
        assert [lib.hsn_nearest(d, n_in, n_out) for d in range(n_out)] == list(near.astype(int)), (n_in, n_out)
        for align in (True, False):
            eye = torch.eye(n_in, dtype=torch.float32).reshape(1, n_in, 1, n_in).expand(1, n_in, 2, n_in)
            want = F.interpolate(eye, size=(2, n_out), mode="bilinear", align_corners=align)[0, :, 0].numpy()     # [source, destination]
            got = np.zeros((n_in, n_out), np.float32)
            for d in range(n_out):
                i0, i1, l1 = sc.C.c_int32(), sc.C.c_int32(), sc.C.c_float()
                lib.hsn_tap(d, n_in, n_out, int(align), sc.C.byref(i0), sc.C.byref(i1), sc.C.byref(l1))
                assert 0 <= i0.value <= i1.value <= n_in - 1 and 0.0 <= l1.value <= 1.0
                got[i0.value, d] += np.float32(1) - np.float32(l1.value)
                got[i1.value, d] += np.float32(l1.value)
            assert np.abs(got - want).max() <= 1e-6, (n_in, n_out, align)


@pytest.mark.parametrize("name", sc.SMALL)
def test_inverse_tables_of_a_brute_force_walk(name):
    """the blob the library fills (mpmhip_shadow_workspace_bytes, no device needed) equals the host build's, and every inverse list is
    what a walk over the forward table finds, in ascending (destination, side)"""
    from mpmavatar_amd.shadow_net import resample_tables
    sh = sc.shape(name)
    s, u, size_in = sh["shadow_size"], sh["uv_size"], sh["input"]
    words, ws_bytes = resample_tables(size_in, size_in, s, u, sh["n_dims"])
    assert np.array_equal(words, sc.host_tables(size_in, size_in, s, u)) and ws_bytes > 0
    t = sc.split_tables(words, s, u)
    assert list(t["ny"]) == [sc.host_lib().hsn_nearest(d, size_in, s) for d in range(s)] and np.array_equal(t["ny"], t["nx"])
    for key, r in t.items():
        if key in ("ny", "nx"):
            continue
        lists = [[] for _ in range(r["in"])]
        for d in range(r["out"]):
            lists[r["i0"][d]].append((d, np.float32(1) - r["l1"][d]))
            lists[r["i1"][d]].append((d, r["l1"][d]))
        assert r["inv_start"][0] == 0 and r["inv_start"][-1] == 2 * r["out"]
        for src in range(r["in"]):
            a, b = r["inv_start"][src], r["inv_start"][src + 1]
            assert list(r["inv_dst"][a:b]) == [d for d, _ in lists[src]], (key, src)
            assert np.array_equal(r["inv_w"][a:b], np.array([w for _, w in lists[src]], np.float32)), (key, src)
    if name == "tiny":
        assert t["down2"]["out"] == 1 and t["down2"]["l1"][0] == 0 and t["up0"]["in"] == 1 and (t["up0"]["i1"] == 0).all()
    if u == s:
        assert (t["fin"]["l1"] == 0).all() and list(t["fin"]["i0"]) == list(range(s))


def test_nearest_cell_is_the_same_in_float64():
    """the one discontinuous decision: the float32 rule picks the rows torch picks for the float64 twin"""
    c = sc.case("odd")
    idx = torch.arange(33 * 33, dtype=torch.float64).reshape(1, 1, 33, 33)
    got = F.interpolate(idx, size=(20, 20))[0, 0].numpy().astype(int)
    ny = sc.split_tables(sc.host_tables(33, 33, 20, 24), 20, 24)["ny"]
    assert np.array_equal(got, ny[:, None] * 33 + ny[None, :]) and c["ao_map"].shape[-1] == 33


# ---- shadow_math.hpp on the host against the float64 twin -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sc.SMALL)
def test_host_against_float64(name):
    got, want = sc.host_run(name), sc.t64(name)
    sc.report(name, got, want, sc.BOUND[name], "host")
    sh = sc.shape(name)
    if sh["uv_size"] == sh["shadow_size"]:
        assert np.array_equal(got["shadow_map"], got["shadow_map_lowres"])
    size_in = sh["input"]
    if size_in == sh["shadow_size"]:
        assert np.array_equal(got["ao_map"], sc.case(name)["ao_map"])


def test_host_frozen_parameters():
    """a parameter that wants no gradient gets none, and every other gradient keeps its bits"""
    name = "odd"
    frozen = ("enc_layers.0.0.weight_v", "enc_layers.0.0.weight_g", "enc_layers.2.0.bias", "dec_layers.1.0.weight_g", "shadow_pred.bias",
              "shadow_pred.weight_v")
    base, part = sc.host_run(name), sc.host_run(name, frozen=frozen)
    for k in sc.names(name):
        if k in frozen:
            assert part[k] is None
        else:
            assert np.array_equal(part[k], base[k]), k


def test_stand_alone_program_under_sanitizers():
    """forward and four backward passes over exactly sized buffers at six configurations, as a stand-alone program built with
    -fsanitize=address,undefined: an index past a row, a table or a workspace section ends it with a report"""
    r = subprocess.run([sc.sanitizer_program()], capture_output=True, text=True, timeout=300)
    print(r.stdout.strip(), r.stderr.strip()[:2000])
    assert r.returncode == 0 and r.stdout.startswith("ok:"), (r.returncode, r.stderr[-2000:])
