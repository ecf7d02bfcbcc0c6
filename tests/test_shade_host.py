"""The colour path of the appearance loop without a GPU: the twin (tests/shade_twin_torch.py) pinned against the reference's own
convert_SH / eval_sh and torch's F.grid_sample (tests/golden/shade.npz); a central-difference spot check of the twin; the measurement
of S32, the constant the bound is built on; the conditions the cases must meet; mpmavatar_amd/csrc/shade_math.hpp compiled with g++
(tests/hostshade/hostshade.cpp: serial loops that mirror the forward and the three backward stages) against the float64 twin; the
texel table of a brute-force walk; exact zeros; the NULL forms; and the same file as a stand-alone program under AddressSanitizer and
UBSan.  Every comparison prints its figures before it asserts (run with -s)."""
import os
import subprocess

import numpy as np
import pytest
import torch

import shade_cases as sc
import shade_twin_torch as tw

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shade.npz")
PAIRS = [(name, deg) for name in sc.CASES for deg in sc.DEGREES[name]]


# ---- the twin is the reference -----------------------------------------------------------------------------------------------

def test_twin_reproduces_the_reference():
    """tests/golden/shade.npz: the reference's convert_SH and eval_sh with torch's grid_sample under autograd, float64, on the inputs of
    `main` -- which are the fixture's own, bit for bit"""
    g, c = np.load(GOLD), sc.case("main")
    for k, v in c.items():
        assert np.array_equal(g[k], v) and g[k].dtype == v.dtype, k
    stride = int(g["rest_stride"])
    for deg in range(4):
        t, used = sc.t64("main", deg), (deg + 1) ** 2
        assert (t["features_rest"][:, used - 1:] == 0).all()
        pairs = {"colors": (t["colors"], g[f"deg{deg}_colors"]), "features_dc": (t["features_dc"], g[f"deg{deg}_d_features_dc"]),
                 "features_rest": (t["features_rest"][::stride, :used - 1], g[f"deg{deg}_d_features_rest_used"]),
                 "means3D": (t["means3D"], g[f"deg{deg}_d_means3D"]), "shadow_map": (t["shadow_map"], g[f"deg{deg}_d_shadow_map"])}
        for k, (mine, ref) in pairs.items():
            err = sc.rel(mine, ref)
            print("degree", deg, k, "twin against the fixture %.3g" % err)
            assert ref.dtype == np.float64 and err < 1e-13, (deg, k)


def test_twin_against_central_differences():
    """an anchor independent of autograd: central differences of the float64 twin's loss on a handful of coordinates, a map texel
    among them"""
    c, g = sc.case("main"), sc.t64("main", 3)
    uv, b = torch.tensor(c["face_uv"], dtype=torch.float64), torch.from_numpy(c["binding"].astype(np.int64))
    w, campos = torch.tensor(c["w"], dtype=torch.float64), torch.tensor(c["campos"], dtype=torch.float64)

    def loss(t):
        return float((w * tw.shaded(3, t["features_dc"], t["features_rest"], t["means3D"], campos, t["shadow_map"], uv, b)).sum())

    base = {k: torch.tensor(c[k], dtype=torch.float64) for k in sc.GRADS}
    tapped = int(np.abs(g["shadow_map"]).argmax())
    spots = [("features_dc", (3, 0, 1)), ("features_rest", (10, 0, 2)), ("features_rest", (11, 14, 0)), ("means3D", (20, 0)),
             ("means3D", (7, 2)), ("shadow_map", divmod(tapped, 7)), ("shadow_map", (0, 0)), ("shadow_map", (2, 6))]
    h = 1e-6
    for k, at in spots:
        t = {n: v.clone() for n, v in base.items()}
        t[k][at] += h
        up = loss(t)
        t[k][at] -= 2 * h
        fd = (up - loss(t)) / (2 * h)
        print(k, at, "autograd %.9g central difference %.9g" % (g[k][at], fd))
        assert abs(fd - g[k][at]) <= 1e-6 * max(1.0, abs(g[k][at]))
    assert g["shadow_map"][2, 6] == 0 and g["shadow_map"][0, 0] != 0


# ---- the yardstick and the conditions of the comparison ---------------------------------------------------------------------------

def test_s32_is_the_measurement():
    worst = 0.0
    for name, deg in PAIRS:
        t32 = sc.twin(sc.case(name), deg, torch.float32)
        errs = {k: sc.rel(t32[k], sc.t64(name, deg)[k]) for k in sc.TENSORS}
        print(name, "degree", deg, ", ".join("%s %.3g" % kv for kv in errs.items()))
        worst = max(worst, max(errs.values()))
    print("S32 measured %.4g, committed %.4g" % (worst, sc.S32))
    assert 0.5 * sc.S32 < worst <= sc.S32
    assert sc.BOUND == 10 * sc.S32


@pytest.mark.parametrize("name", sc.CASES)
def test_cases_meet_the_conditions(name):
    """over EVERY Gaussian, channel and degree 0..3 the case has coefficients for: no unclamped sh + 0.5 within CLAMP_MARGIN of zero
    (nothing left out); no position within 0.1 of the camera; the bilinear cell is the same in float32 and float64.  On `main` the
    clamp binds at every degree >= 2 and the index structure is the stated one."""
    c = sc.case(name)
    n, n_f = c["binding"].shape[0], c["face_uv"].shape[0]
    H, W = c["shadow_map"].shape
    assert float(np.linalg.norm(c["means3D"].astype(np.float64) - c["campos"], axis=1).min()) > sc.MIN_CAM_DISTANCE
    for deg in sc.DEGREES[name]:
        raw = sc.raw_sh(c, deg)
        print(name, "degree", deg, "closest unclamped value to zero %.3g, clamp binds on %.1f %%" % (np.abs(raw).min(), 100 * (raw < 0).mean()))
        assert raw.shape == (n, 3) and np.abs(raw).min() > sc.CLAMP_MARGIN
        if name == "main" and deg >= 2:
            assert (raw < 0).any()
    idx = {d: tw.taps(torch.tensor(c["face_uv"], dtype=d), H, W)[0].numpy() for d in (torch.float32, torch.float64)}
    assert np.array_equal(idx[torch.float32], idx[torch.float64])
    host_idx, host_w = sc.host_taps(c["face_uv"], H, W)
    assert np.array_equal(host_idx, idx[torch.float32])
    assert np.array_equal(host_w, tw.taps(torch.tensor(c["face_uv"]), H, W)[1].numpy())      # the same fp32 operations: the same bits
    if name == "main":
        i = idx[torch.float64]
        per_face = np.bincount(c["binding"], minlength=n_f)
        assert (n, n_f, H, W, c["features_rest"].shape[1]) == (300, 37, 5, 7, 15) and n % 64 != 0
        assert per_face[0] == 0 and per_face[1] >= 70 and (per_face[2:9] > 0).all() and (np.diff(c["binding"]) < 0).any()
        assert tuple(c["face_uv"][2]) == (-1.0, -1.0) and tuple(c["face_uv"][3]) == (1.0, 1.0)
        assert list(i[2]) == [-1, -1, -1, 0] and list(i[3]) == [H * W - 1, -1, -1, -1]       # the two corners of the map
        assert (i[4] == -1).all()                                                              # wholly outside
        assert list(i[5] >= 0) == [False, True, False, True] and list(i[6] >= 0) == [True, True, False, False]   # the half-texel border
        assert np.array_equal(c["face_uv"][7], c["face_uv"][8]) and np.array_equal(i[7], i[8]) and (i[7] >= 0).all()
        tapped = np.bincount(i[i >= 0], minlength=H * W)
        assert (tapped == 0).sum() >= 5 and tapped.max() >= 5


# ---- shade_math.hpp on the host against the float64 twin ----------------------------------------------------------------------------

@pytest.mark.parametrize("name,deg", PAIRS)
def test_host_against_float64(name, deg):
    got, want = sc.host_run(sc.case(name), deg), sc.t64(name, deg)
    for k in sc.TENSORS:
        err = sc.rel(got[k], want[k])
        print(name, "degree", deg, k, "%.3g of bound %.3g" % (err, sc.BOUND))
        assert np.isfinite(got[k]).all() and err <= sc.BOUND, k


@pytest.mark.parametrize("features,shadow", [(True, False), (False, True)], ids=["no_shadow_map", "no_features"])
def test_host_null_forms(features, shadow):
    """shadow_map == NULL: plain convert_SH; features_dc == NULL: the shadow on three channels"""
    c = sc.case("main")
    got, want = sc.host_run(c, 3, features=features, shadow=shadow), sc.twin(c, 3, features=features, shadow=shadow)
    for k in sc.TENSORS:
        if want[k] is None:
            assert got[k] is None
            continue
        err = sc.rel(got[k], want[k])
        print(k, "%.3g of bound %.3g" % (err, sc.BOUND))
        assert np.isfinite(got[k]).all() and err <= sc.BOUND, k
    if not features:
        assert (got["colors"][:, 0] == got["colors"][:, 1]).all() and (got["colors"][:, 0] == got["colors"][:, 2]).all()


def test_sampler_table_of_a_brute_force_walk():
    """the table ShadowSampler builds with torch ops (here: the same function on CPU tensors) against loops over the header's own
    taps"""
    from mpmavatar_amd.shading import texel_table
    for name in sc.CASES:
        c = sc.case(name)
        H, W = c["shadow_map"].shape
        t_start, t_items = texel_table(torch.tensor(c["face_uv"]), H, W)
        start, items = sc.brute_force_texel_table(c["face_uv"], H, W)
        assert t_start.dtype == torch.int32 and t_items.dtype == torch.int32
        assert np.array_equal(t_start.numpy(), start) and np.array_equal(t_items.numpy(), items), name
        for t in range(H * W):
            seg = items[start[t]:start[t + 1]]
            assert (np.diff(seg) > 0).all()


def test_host_exact_zeros():
    c = sc.case("main")
    H, W = c["shadow_map"].shape
    start, _ = sc.brute_force_texel_table(c["face_uv"], H, W)
    untapped = np.diff(start) == 0
    on_outside = c["binding"] == 4
    assert untapped.any() and on_outside.any()
    for deg in range(4):
        r, used = sc.host_run(c, deg), (deg + 1) ** 2
        assert (r["shadow_map"].reshape(-1)[untapped] == 0).all() and (r["shadow_map"].reshape(-1)[~untapped] != 0).any()
        assert (r["features_rest"][:, used - 1:] == 0).all() and (used == 1 or (r["features_rest"][:, :used - 1] != 0).any())
        assert (r["colors"][on_outside] == 0).all() and (r["features_dc"][on_outside] == 0).all()
        assert (r["means3D"] == 0).all() == (deg == 0)
    # the face without a Gaussian contributes nothing: wherever its uv lies, every output is the same
    base, moved = sc.host_run(c, 3), dict(c)
    moved["face_uv"] = c["face_uv"].copy()
    moved["face_uv"][0] = (-0.35, 0.45)
    assert not np.array_equal(sc.host_taps(moved["face_uv"], H, W)[0][0], sc.host_taps(c["face_uv"], H, W)[0][0])
    again = sc.host_run(moved, 3)
    for k in sc.TENSORS:
        assert np.array_equal(again[k], base[k]), k
    # no upstream gradient: every output is written, with zeros
    z = sc.host_run(c, 3, g=False)
    for k in sc.GRADS:
        assert (z[k] == 0).all(), k


def test_stand_alone_program_under_sanitizers(tmp_path):
    """the loops over the main case's index structure (the empty face, the 72-entry face, the uv outside the map, the texels without a
    tap) and n = 0, as a stand-alone program built with -fsanitize=address,undefined: an index past a row or a table ends it with a
    report"""
    c = sc.case("main")
    H, W = c["shadow_map"].shape
    path = tmp_path / "structure.bin"
    with open(path, "wb") as f:
        np.array([H, W, c["face_uv"].shape[0], c["binding"].shape[0], 16], np.int32).tofile(f)
        c["face_uv"].astype(np.float32).tofile(f)
        c["binding"].astype(np.int32).tofile(f)
    exe = sc.sanitizer_program()
    for args in ([str(path)], []):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
        print(r.stdout.strip(), r.stderr.strip()[:2000])
        assert r.returncode == 0 and r.stdout.startswith("ok:"), (r.returncode, r.stderr[-2000:])
        if args:
            start, _ = sc.brute_force_texel_table(c["face_uv"], H, W)
            untapped = int((np.diff(start) == 0).sum())
            assert f"5 x 7 map ({untapped} texels without a tap), 37 faces (1 without Gaussians, 1 outside the map), 300 Gaussians" in r.stdout
