"""The image head without a GPU: a central-difference anchor of the twin (tests/image_head_twin_torch.py: the two lines of
train_appearance.py:126-127 in torch); the measurement of S32, the constant the bound is built on; the conditions every pixel of
every case must meet; mpmavatar_amd/csrc/image_head_math.hpp compiled with g++ (tests/hostimagehead/hostimagehead.cpp: serial loops
that mirror the forward, the backward map and the fold) against the float64 twin; exact zeros; the NULL forms; the byte functions
against numpy, exactly; eval_mask against scipy.ndimage; and the same loops as a stand-alone program under AddressSanitizer and
UBSan.  Every comparison prints its figures before it asserts (run with -s)."""
import subprocess

import numpy as np
import pytest
import torch

import image_head_cases as ic
import image_head_twin_torch as tw


# ---- the twin ----------------------------------------------------------------------------------------------------------------

def test_twin_against_central_differences():
    """an anchor independent of autograd: central differences of the float64 twin's loss on a few coordinates of each of the four
    inputs, away from the clip's kinks (a pixel within 1e-3 of a bound would put the kink inside the stencil)"""
    c, g = ic.case("main"), ic.t64("main")
    v = ic.unclipped64(c)
    cam = c["cam"]
    w = torch.tensor(c["w"], dtype=torch.float64)

    def loss(t):
        return float((w * tw.camera_image(t["render"], t["mask"], t["cam_m"], t["cam_c"], cam)).sum())

    base = {k: torch.tensor(c[k], dtype=torch.float64) for k in ic.GRADS}
    inside = np.argwhere((v[1] > 0.05) & (v[1] < 0.95) & (c["mask"] > 0.1))
    clipped = np.argwhere(v[0] > 1.05)
    (y0, x0), (y1, x1), (y2, x2) = inside[0], inside[len(inside) // 2], clipped[0]
    spots = [("render", (1, y0, x0)), ("render", (1, y1, x1)), ("render", (0, y2, x2)), ("mask", (y0, x0)), ("mask", (y1, x1)),
             ("cam_m", (cam, 0)), ("cam_m", (cam, 2)), ("cam_m", (0, 1)), ("cam_c", (cam, 1)), ("cam_c", (4, 0))]
    h = 1e-6
    # a step of h in cam_m or cam_c moves EVERY pixel of a channel; none of them may cross a bound: |dv| <= 2 h
    assert ic.clip_distance("main", c) > 4 * h
    for k, at in spots:
        at = tuple(int(i) for i in at)
        t = {n: x.clone() for n, x in base.items()}
        t[k][at] += h
        up = loss(t)
        t[k][at] -= 2 * h
        fd = (up - loss(t)) / (2 * h)
        print(k, at, "autograd %.9g central difference %.9g" % (g[k][at], fd))
        assert abs(fd - g[k][at]) <= 1e-6 * max(1.0, abs(g[k][at]))
    assert g["render"][0, y2, x2] == 0 and g["cam_m"][0, 1] == 0 and g["cam_c"][4, 0] == 0 and g["cam_m"][cam, 0] != 0


def test_torch_clip_passes_the_gradient_at_both_ends():
    """the rule the kernels copy: x.clip(0., 1.) has gradient 1 at 0.0, -0.0 and 1.0, and 0 outside"""
    x = torch.tensor([0.0, -0.0, 1.0, -1e-30, 1.0000001], requires_grad=True)
    x.clip(0., 1.).sum().backward()
    assert x.grad.tolist() == [1.0, 1.0, 1.0, 0.0, 0.0]


# ---- the yardstick and the conditions of the comparison ---------------------------------------------------------------------------

def test_s32_is_the_measurement():
    worst = 0.0
    for name in ic.CASES:
        t32 = ic.twin(ic.case(name), torch.float32)
        errs = {k: ic.rel(t32[k], ic.t64(name)[k]) for k in ic.TENSORS}
        print(name, ", ".join("%s %.3g" % kv for kv in errs.items()))
        worst = max(worst, max(errs.values()))
    print("S32 measured %.4g, committed %.4g" % (worst, ic.S32))
    assert 0.5 * ic.S32 < worst <= ic.S32
    assert ic.BOUND == 10 * ic.S32


@pytest.mark.parametrize("name", ic.CASES)
def test_cases_meet_the_conditions(name):
    """over EVERY pixel and channel (nothing left out): v is an exact zero through mask == 0, or a planted exact 0 or 1, or further
    than CLIP_MARGIN from both clip bounds; the frames of the byte cases keep BYTE_MARGIN from every byte boundary; and each case
    holds what the table of tests/image_head_cases.py says"""
    c = ic.case(name)
    v, m = ic.unclipped64(c), c["mask"]
    H, W = m.shape
    from_mask = np.broadcast_to(m == 0, v.shape) & (v == 0)
    plant = ic.planted(name, v.shape) & ((v == 0) | (v == 1))
    clear = (np.abs(v) > ic.CLIP_MARGIN) & (np.abs(v - 1) > ic.CLIP_MARGIN)
    print(name, "closest v to a clip bound %.3g; below 0: %.1f %%, above 1: %.1f %%" % (ic.clip_distance(name, c), 100 * (v < 0).mean(),
                                                                                            100 * (v > 1).mean()))
    assert (from_mask | plant | clear).all()
    assert ic.planted(name, v.shape).sum() == plant.sum()
    if name in ic.BYTE_CASES:
        assert not ic.byte_offenders(c).any()
    wg = ic.host_lib().ih_workgroups(H * W)
    if name == "main":
        assert (H, W, c["cam_m"].shape[0], c["cam"]) == (37, 29, 5, 2) and (H * W) % 4 != 0 and wg == 2 and H * W - 1024 < 64
        assert (v < 0).any() and (v > 1).any() and (m == 0).sum() >= 50 and (m == 1).any() and ((m > 0) & (m < 1)).any()
    if name == "vec":
        assert (H * W) % 4 == 0 and wg == 3 and c["cam"] == 0
    if name == "last":
        assert c["cam"] == c["cam_m"].shape[0] - 1 and (H * W) % 4 == 0
    if name == "one":
        assert (H, W) == (1, 1)
    if name == "dark":
        t = ic.t64(name)
        assert (m == 0).all() and (t["image"] == 0).all() and (t["render"] == 0).all() and (t["mask"] != 0).any()
        assert (t["cam_m"] == 0).all() and (t["cam_c"] == 0).all()
    if name == "edges":
        t, cam = ic.t64(name), c["cam"]
        assert c["cam_m"][cam, 0] == 0 and c["cam_c"][cam, 0] == 0
        for y, x in ic.EDGE_ZERO:
            assert v[0, y, x] == 0 and m[y, x] != 0 and t["render"][0, y, x] != 0
        for y, x in ic.EDGE_ONE:
            assert v[0, y, x] == 1 and m[y, x] == 1 and t["render"][0, y, x] != 0


def test_workgroups_are_a_function_of_the_pixel_count():
    lib = ic.host_lib()
    for n, want in ((1, 1), (1024, 1), (1025, 2), (37 * 29, 2), (48 * 64, 3), (1024 * 1024, 1024), (1024 * 1024 + 1, 1024), (2 ** 31 - 1, 1024)):
        assert lib.ih_workgroups(n) == want == ic.scratch_doubles(1, n) // 6, n


# ---- image_head_math.hpp on the host against the float64 twin ------------------------------------------------------------------------

@pytest.mark.parametrize("name", ic.CASES)
def test_host_against_float64(name):
    c = ic.case(name)
    got, want = ic.host_run(c), ic.t64(name)
    for k in ic.TENSORS:
        err = ic.rel(got[k], want[k])
        print(name, k, "%.3g of bound %.3g" % (err, ic.BOUND))
        assert np.isfinite(got[k]).all() and err <= ic.BOUND, k
    if name == "edges":
        for y, x in ic.EDGE_ZERO + ic.EDGE_ONE:
            assert got["render"][0, y, x] != 0, (y, x)                  # the gradient passes at v == 0 and at v == 1


def test_host_exact_zeros():
    """the rows of the other cameras; d_render wherever mask == 0, although d_mask is not zero there; clipped pixels"""
    c = ic.case("main")
    r, cam, v = ic.host_run(c), c["cam"], ic.unclipped64(c)
    off = np.arange(c["cam_m"].shape[0]) != cam
    assert (r["cam_m"][off] == 0).all() and (r["cam_c"][off] == 0).all() and (r["cam_m"][cam] != 0).all() and (r["cam_c"][cam] != 0).all()
    dark = c["mask"] == 0
    assert (r["render"][:, dark] == 0).all() and (r["mask"][dark] != 0).all() and (r["image"][:, dark] == 0).all()
    out = (v < 0) | (v > 1)
    assert (r["render"][out] == 0).all() and (r["render"][~out & ~np.broadcast_to(dark, v.shape)] != 0).all()
    assert (r["image"][v > 1] == 1).all() and (r["image"][v < 0] == 0).all()
    d = ic.host_run(ic.case("dark"))
    assert (d["image"] == 0).all() and (d["render"] == 0).all() and (d["mask"] != 0).any() and (d["cam_m"] == 0).all() and (d["cam_c"] == 0).all()


def test_host_null_forms():
    """each gradient alone, the other three NULL: the same bits as in the run of all four; no upstream gradient: zeros"""
    c = ic.case("main")
    full = ic.host_run(c)
    for k in ic.GRADS:
        alone = ic.host_run(c, want=(k,))
        assert all(alone[o] is None for o in ic.GRADS if o != k)
        assert np.array_equal(alone[k], full[k]), k
    z = ic.host_run(c, g=False)
    for k in ic.GRADS:
        assert (z[k] == 0).all(), k
    assert np.array_equal(z["image"], full["image"])


def test_host_nan_propagates():
    c = dict(ic.case("one"))
    c["render"] = np.full((3, 1, 1), np.nan, np.float32)
    assert np.isnan(ic.host_run(c)["image"]).all()


# ---- the byte functions against numpy, exactly -------------------------------------------------------------------------------------

def test_division_by_255_at_all_256_values():
    """astype(float32) / 255. of eval.py:68, a true division: a product with the fp32 reciprocal differs at many values"""
    pred = np.arange(256 * 3, dtype=np.int64).reshape(16, 16, 3) % 256
    pred = pred.astype(np.uint8)
    gt = pred[::-1].copy()
    mask = np.ones((16, 16), np.float32)
    a, b = ic.host_eval_pair(pred, gt, mask, False)
    want = pred.astype(np.float32).transpose(2, 0, 1) / np.float32(255.)
    assert set(pred.reshape(-1).tolist()) == set(range(256))
    assert np.array_equal(a, want) and np.array_equal(b, gt.astype(np.float32).transpose(2, 0, 1) / np.float32(255.))
    by_reciprocal = np.arange(256, dtype=np.float32) * (np.float32(1.0) / np.float32(255.))
    differ = int((by_reciprocal != np.arange(256, dtype=np.float32) / np.float32(255.)).sum())
    print("a product with 1 / 255 differs from the division at %d of 256 values" % differ)
    assert differ > 0


@pytest.mark.parametrize("remove_white", [False, True])
def test_eval_pair_against_numpy(remove_white):
    """HWC -> CHW, the white rule at sums 688 (kept) and 689 (removed), each image on its own, the mask"""
    pred, gt, mask = ic.eval_frames(9, 7)
    a, b = ic.host_eval_pair(pred, gt, mask, remove_white)
    want_a, want_b = ic.numpy_eval_pair(pred, gt, mask, remove_white)
    assert np.array_equal(a, want_a) and np.array_equal(b, want_b)
    assert int(pred[0, 1].astype(int).sum()) == 688 and int(pred[0, 2].astype(int).sum()) == 689 and int(gt[0, 1].astype(int).sum()) == 689
    assert (a[:, 0, 1] != 0).all() and (b[:, 0, 2] != 0).all()                       # 688 stays
    assert ((a[:, 0, 2] == 0).all() and (b[:, 0, 1] == 0).all() and (a[:, 0, 0] == 0).all()) == remove_white      # 689 and 765 go
    assert (b[:, 0, 0] != 0).any()                                                   # white in pred only: gt keeps its pixel


def test_white_rule_is_the_mean_rule_for_bytes():
    """every triple of bytes with a sum in 680 .. 699: sum >= 689 exactly where torch's fp32 mean of the three quotients is > 0.90"""
    t = np.array([(a, b, c) for a in range(170, 256) for b in range(170, 256) for c in range(170, 256) if 680 <= a + b + c <= 699], np.uint8)
    f = torch.from_numpy(t.astype(np.float32).T.copy()) / 255.
    assert np.array_equal((f.mean(axis=0) > 0.90).numpy(), t.astype(int).sum(axis=1) >= 689)


@pytest.mark.parametrize("name", ic.BYTE_CASES)
@pytest.mark.parametrize("affine,white", ic.FRAME_FORMS)
def test_frame_bytes_on_the_host(name, affine, white):
    """every byte equals the floor of the float64 value: HWC layout, truncation, the white background, the NULL-affine form"""
    c = ic.case(name)
    got = ic.host_bytes(c["render"], c["mask"], c["cam_m"] if affine else None, c["cam_c"] if affine else None, c["cam"] if affine else None, white)
    want = ic.bytes64(c, affine, white)
    assert got.shape == want.shape == c["mask"].shape + (3,) and got.dtype == np.uint8
    assert np.array_equal(got, want)
    if name == "main":
        assert (want == 0).any() and (want == 255).any() and ((want > 0) & (want < 255)).any()


def test_frame_bytes_truncate():
    """(x * 255.).astype(uint8) truncates: 0.999 -> 254, 1 -> 255, above 1 -> 255, below 0 -> 0; numpy's own conversion agrees"""
    vals = np.array([0.0, 0.999, 1.0, 1.5, -0.2, 0.5, 0.004, 0.0039], np.float32)
    render = np.broadcast_to(vals[None, None, :], (3, 1, vals.size)).copy()
    got = ic.host_bytes(render, np.ones((1, vals.size), np.float32), None, None, None, False)
    want = (np.clip(vals, 0, 1) * 255.).astype(np.uint8)
    assert want.tolist() == [0, 254, 255, 255, 0, 127, 1, 0]
    assert all(np.array_equal(got[0, :, ch], want) for ch in range(3))


@pytest.mark.parametrize("white", [False, True])
def test_compose_against_numpy(white):
    c = ic.case("main")
    assert np.array_equal(ic.host_compose(c["render"], c["mask"], white), ic.numpy_compose(c["render"], c["mask"][None], white))


# ---- eval_mask against scipy.ndimage ------------------------------------------------------------------------------------------------

def test_eval_mask_against_scipy():
    """eval.py:81-84 (five 3 x 3 erosions, then the 5 x 5 blur of sigma 0) as scipy.ndimage states them.  The mask touches the top
    border -- where a border that eroded would show -- and holds the values 1, 254/255 and 250/255, so that the minimum is not
    trivially 0 or 1.  The erosion must be equal; the blur within 1e-6: two passes of five non-negative terms with sum <= 1, the
    products by 1/16 and 4/16 exact, one rounding of at most 2^-25 per 6/16 product and per addition -- at most 5 roundings a pass on
    partial sums <= 1, 10 * 2^-25 = 3e-7 over both, in either precision's order of the additions."""
    import scipy.ndimage as ndi
    from mpmavatar_amd.image_head import eval_mask
    rng = np.random.default_rng(5)
    H, W = 37, 29
    m = np.zeros((H, W), np.float32)
    m[0:24, 6:25] = 1.0                                  # touches the top border
    m[26:35, 2:20] = 1.0
    inside = m == 1
    pick = rng.uniform(size=m.shape)
    m[inside & (pick < 0.01)] = np.float32(254 / 255)
    m[3, 20] = m[30, 5] = np.float32(250 / 255)
    assert set(np.unique(m).tolist()) == {0.0, float(np.float32(250 / 255)), float(np.float32(254 / 255)), 1.0}
    eroded = m
    for _ in range(5):
        eroded = ndi.grey_erosion(eroded, size=(3, 3), mode="constant", cval=np.inf)
    k = np.array([1, 4, 6, 4, 1], np.float64) / 16
    blurred = ndi.correlate1d(ndi.correlate1d(eroded.astype(np.float64), k, axis=1, mode="mirror"), k, axis=0, mode="mirror")
    from torch.nn import functional as F
    ours_eroded = -F.max_pool2d(-torch.from_numpy(m)[None, None], 11, 1, 5)[0, 0].numpy()
    assert np.array_equal(ours_eroded, eroded)
    assert (eroded[0, 11:20] > 0).all() and len(np.unique(eroded)) == 4         # the border did not erode; the minimum is not trivial
    got = eval_mask(torch.from_numpy(m)).numpy()
    err = float(np.abs(got - blurred).max())
    print("erosion equal; blur differs from scipy's float64 by %.3g (bound 1e-6)" % err)
    assert got.dtype == np.float32 and got.shape == m.shape and err <= 1e-6


# ---- the same loops as a stand-alone program under the sanitizers ---------------------------------------------------------------------

def test_stand_alone_program_under_sanitizers(tmp_path):
    """the loops over `main` (a partial last quad, a second workgroup that is nearly empty), over `one` and over a call without a
    pixel, on exactly sized buffers, as a stand-alone program built with -fsanitize=address,undefined: an index past a plane, a row
    or the scratch ends it with a report"""
    paths = []
    for name in ("main", "one"):
        c = ic.case(name)
        _, H, W = c["render"].shape
        path = tmp_path / (name + ".bin")
        with open(path, "wb") as f:
            np.array([H, W, c["cam_m"].shape[0], c["cam"]], np.int32).tofile(f)
            for k in ("render", "mask", "cam_m", "cam_c", "w"):
                np.ascontiguousarray(c[k], np.float32).tofile(f)
        paths.append(str(path))
    r = subprocess.run([ic.sanitizer_program()] + paths, capture_output=True, text=True, timeout=120)
    print(r.stdout.strip(), r.stderr.strip()[:2000])
    assert r.returncode == 0 and r.stdout.startswith("ok: 2 cases, %d pixels, and a call without a pixel" % (37 * 29 + 1)), (r.returncode, r.stderr[-2000:])
