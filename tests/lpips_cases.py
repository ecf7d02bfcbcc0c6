"""Cases, yardstick and helpers shared by tests/test_lpips_host.py, tests/test_lpips_abi.py and tests/test_gpu_lpips.py.  Test
infrastructure only.

  case   (N, H, W)     levels                              what it exercises
  tiny   (1, 16, 16)   16, 8, 4, 2, 1                      level 5 is 1 x 1: every tap of its convolutions but the centre is padding
  odd    (2, 35, 22)   35x22, 17x11, 8x5, 4x2, 2x1         a batch (the sum over it), poolings that drop a row or a column at three levels
  tiles  (1, 72, 40)   72x40, 36x20, 18x10, 9x5, 4x2       18 x 2 pixel tiles of 4 x 32 at level 1, a ragged right edge; ragged below at 18 and 9

Weights are full-width VGG16 weights from numpy.random.default_rng(SEED), nothing of their 59 MB is stored: convolution weights
~ N(0, 2 / (9 cin)), biases ~ 0.05 + 0.05 N(0, 1), tap weights ~ U(0, 2 / C).  Images: x ~ U(0, 1), y = clip(x + 0.15 N(0, 1), 0, 1).
The yardstick is the reference's own class in float64 (tests/golden/lpips.npz, made by tests/golden/make_golden_lpips.py from these
inputs), which the twin (tests/lpips_twin_torch.py) reproduces to 1e-12.  No tap pixel of any case has a zero feature vector (t64
asserts it), so the one stated deviation -- the reference's NaN gradient there -- never enters a comparison.

The image seeds are chosen for one more condition, which t64 asserts too.  d out / d x is discontinuous where a pre-activation of x
crosses zero or two elements of a pooling window meet: a float32 evaluation that lands on the other side of one such decision is off
by that unit's whole gradient (about 3e-3 of max |dx| for one unit of conv3_2 at 72 x 40), whatever its arithmetic.  With some 10^6
decisions per case the smallest float64 margin is around 1e-6 .. 1e-5, the size of float32's error at depth, so about every other
random image has such a unit.  A comparison of gradients at 10 * S32 is meaningful only where float32 decides as float64 does: the
seeds are the first from 100 on for which every |pre-activation| and every gap between the two largest elements of a pooling window
with a positive maximum was at least SEED_MARGIN = 2 times the largest |float32 - float64| activation error of the TWIN at that
layer where the seeds were chosen (2.4 for `tiles`, 4.6 for `odd`, 11 for `tiny`); t64 asserts that the ratio it measures is above 1,
which leaves room for another CPU's float32 convolutions.  The code under test plays no part in the choice."""
import ctypes as C
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

import hostbuild
import lpips_twin_torch as tw
from mpmavatar_amd import _lib as L

_SHAPES = {"tiny": (1, 16, 16, 100), "odd": (2, 35, 22, 101), "tiles": (1, 72, 40, 113)}     # N, H, W, seed of the images
CASES = tuple(_SHAPES)
SEED = 7                                                                              # of the weights, shared by the cases
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lpips.npz")

# Measured on the CPU (tests/test_lpips_host.py::test_s32_is_the_measurement asserts that no figure it sees is above these): the TWIN's
# float32 run against its float64 run, `out` relative to itself, `dx` relative to max |dx|, the larger of the run on torch's own
# thread count and on one thread, rounded up by about a quarter since another CPU may pick another convolution algorithm.  The code
# under test plays no part in it.  Host restatement and GPU must lie within BOUND = 10 * S32 of the float64 fixture (the margin of
# shadow_cases.py): our own summation order over K of up to 4,608 and FMA where torch's kernels use none.
# measured here (8 threads / 1 thread): tiny out 1.660e-7, dx 1.284e-6 / 1.171e-6; odd out 3.209e-8, dx 1.130e-6; tiles out 5.894e-8,
# dx 1.318e-6 / 1.478e-6.  `out` is a float32 near 1e-3: half an ulp of it is 3.8e-8 of itself.
S32 = {"tiny": {"out": 2.1e-7, "dx": 1.6e-6}, "odd": {"out": 4.0e-8, "dx": 1.45e-6}, "tiles": {"out": 7.4e-8, "dx": 1.85e-6}}
BOUND = {k: {q: 10 * v for q, v in s.items()} for k, s in S32.items()}


def shape(name):
    return _SHAPES[name][:3]


@functools.lru_cache(maxsize=None)
def weights():
    """{state-dict key: read-only float32 array} in the reference's order, mean and std included"""
    rng = np.random.default_rng(SEED)
    out = {}
    for k, shp in tw.state_shapes():
        if k == "net.mean":
            v = np.array(tw.MEAN).reshape(shp)
        elif k == "net.std":
            v = np.array(tw.STD).reshape(shp)
        elif k.startswith("lin."):
            v = rng.uniform(0, 2.0 / shp[1], shp)
        elif k.endswith(".weight"):
            v = rng.normal(size=shp) * np.sqrt(2.0 / (9 * shp[1]))
        else:
            v = 0.05 + 0.05 * rng.normal(size=shp)
        out[k] = v.astype(np.float32)
        out[k].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """{"x", "y"}: read-only float32 [N, 3, H, W]"""
    n, h, w, seed = _SHAPES[name]
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, (n, 3, h, w))
    y = np.clip(x + 0.15 * rng.normal(size=x.shape), 0, 1)
    out = {"x": x.astype(np.float32), "y": y.astype(np.float32)}
    for v in out.values():
        v.setflags(write=False)
    return out


def params(dtype=torch.float64, device="cpu"):
    return {k: torch.tensor(v, dtype=dtype, device=device) for k, v in weights().items()}


SEED_MARGIN = 2.0


def _decisions(p, x):
    """-> (the thirteen pre-activation maps of x, per pooling the smallest gap between the two largest elements of a window whose
    maximum is positive)"""
    v, pre, gaps = (x - p["net.mean"]) / p["net.std"], [], []
    for at in range(30):
        if at in tw.CONV_AT:
            v = F.conv2d(v, p[f"net.layers.{at}.weight"], p[f"net.layers.{at}.bias"], padding=1)
            pre.append(v)
        elif at in tw.POOL_AT:
            n, ch, h, w = v.shape
            win = v[:, :, :h // 2 * 2, :w // 2 * 2].reshape(n, ch, h // 2, 2, w // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, ch, h // 2, w // 2, 4)
            top = win.sort(-1).values
            gaps.append(float((top[..., 3] - top[..., 2])[top[..., 3] > 0].min()))
            v = F.max_pool2d(v, 2, 2)
        else:
            v = F.relu(v)
    return pre, gaps


def decision_ratio(name):
    """the smallest float64 decision margin of x over the twin's float32 activation error at that layer (see the module docstring)"""
    x = case(name)["x"]
    with torch.no_grad():
        a64, gaps = _decisions(params(), torch.tensor(x, dtype=torch.float64))
        a32, _ = _decisions(params(torch.float32), torch.tensor(x))
    err = [float((a.double() - b).abs().max()) for a, b in zip(a32, a64)]
    relu = min(float(b.abs().min()) / e for b, e in zip(a64, err))
    pool = min(g / err[layer] for g, layer in zip(gaps, (1, 3, 6, 9)))
    return min(relu, pool)


def twin(name, dtype=torch.float64, device="cpu", images=None):
    """the twin's out [1, 1, 1, 1] and d out / d x in `dtype` -> {"out", "dx"} as numpy; images: a slice of the batch"""
    c, p = case(name), params(dtype, device)
    sel = slice(None) if images is None else images
    x = torch.tensor(c["x"][sel], dtype=dtype, device=device, requires_grad=True)
    y = torch.tensor(c["y"][sel], dtype=dtype, device=device)
    out = tw.forward(p, x, y)
    dx, = torch.autograd.grad(out.sum(), x)
    return {"out": out.detach().cpu().numpy(), "dx": dx.cpu().numpy()}


@functools.lru_cache(maxsize=None)
def t64(name):
    """the float64 twin of a case, computed once and shared; asserts that no tap pixel of x or y has a zero feature vector and that
    every ReLU and pooling decision of x is further from flipping than the twin's float32 error (module docstring)"""
    c, p = case(name), params()
    with torch.no_grad():
        for k in ("x", "y"):
            for f in tw.features(p, torch.tensor(c[k], dtype=torch.float64)):
                norm = float(torch.sqrt((f ** 2).sum(1)).min())
                assert norm > 0.1, (name, k, tuple(f.shape), norm)
    ratio = decision_ratio(name)
    assert ratio > 1.0, (name, ratio)
    out = twin(name)
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def fixture(name):
    """the reference's own results in float64 -> {"out", "dx"}; the stored inputs must be the case's, bit for bit"""
    g, c = np.load(GOLD), case(name)
    for k in ("x", "y"):
        assert g[f"{name}/in/{k}"].dtype == np.float32 and np.array_equal(g[f"{name}/in/{k}"], c[k]), (name, k)
    out = {"out": g[f"{name}/out"], "dx": g[f"{name}/dx"]}
    assert out["out"].dtype == out["dx"].dtype == np.float64 and out["out"].shape == (1, 1, 1, 1)
    return out


def rel(t, ref):
    """max |t - ref| / max |ref| over every element"""
    t, ref = np.asarray(t, np.float64), np.asarray(ref, np.float64)
    assert t.shape == ref.shape, (t.shape, ref.shape)
    top = np.abs(ref).max()
    assert top > 0
    return float(np.abs(t - ref).max() / top)


def report(name, got, want, label, bound=None):
    """every figure printed, then asserted: `out` relative to itself, `dx` relative to max |dx|"""
    bound = BOUND[name] if bound is None else bound
    for q in ("out", "dx"):
        err = rel(got[q], want[q])
        print(name, label, q, "%.3g of bound %.3g" % (err, bound[q]))
        assert np.isfinite(np.asarray(got[q])).all() and err <= bound[q], (name, q, err, bound[q])


# ---- the host build of lpips_math.hpp ------------------------------------------------------------------------------------------------

def host_lib():
    lib = hostbuild.host_lib("hostlpips", flags=["-march=native"])     # fmaf as one instruction where the CPU has one
    lib.hlp_workspace_words.restype = lib.hlp_map_offset.restype = C.c_int64
    return lib


def sanitizer_program():
    """the same file as a stand-alone program under AddressSanitizer and UBSan (run as a subprocess; nothing is loaded into Python)"""
    return hostbuild.host_program("hostlpips", name="hostlpips_asan",
                                  flags=["-O1", "-g", "-march=native", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                         "-DHOSTLPIPS_MAIN"])


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_desc(n, h, w, keep_alive):
    """a descriptor over host copies of weights(); the arrays it points into are appended to keep_alive"""
    d, wt = L.LpipsDesc(), weights()
    d.n, d.h, d.w = n, h, w
    for i, at in enumerate(tw.CONV_AT):
        wgt, bias = np.ascontiguousarray(wt[f"net.layers.{at}.weight"]), np.ascontiguousarray(wt[f"net.layers.{at}.bias"])
        back = np.full(wgt.size, np.nan, np.float32)
        keep_alive += [wgt, bias, back]
        d.weight[i], d.bias[i], d.weight_bwd[i] = wgt.ctypes.data, bias.ctypes.data, back.ctypes.data
    for i in range(5):
        tap = np.ascontiguousarray(wt[f"lin.{i}.1.weight"])
        keep_alive.append(tap)
        d.tap_weight[i] = tap.ctypes.data
    for c in range(3):
        d.mean[c], d.std[c] = tw.MEAN[c], tw.STD[c]
    return d


@functools.lru_cache(maxsize=None)
def host_run(name):
    """forward (kept), backward, and a forward that keeps nothing, on the host -> {"out", "dx", "out_quiet", "maps": the thirteen
    saved maps of x}"""
    c, lib = case(name), host_lib()
    n, h, w = shape(name)
    keep = []
    d = host_desc(n, h, w, keep)
    lib.hlp_prepare(C.byref(d))
    x, y = np.ascontiguousarray(c["x"]), np.ascontiguousarray(c["y"])
    out, quiet, g = np.full((1, 1, 1, 1), np.nan, np.float32), np.full((1, 1, 1, 1), np.nan, np.float32), np.ones(1, np.float32)
    dx = np.full(x.shape, np.nan, np.float32)
    ws = np.zeros(lib.hlp_workspace_words(n, h, w, 1), np.float32)
    lib.hlp_forward(C.byref(d), _p(x), _p(y), 1, _p(ws), _p(out))
    lib.hlp_backward(C.byref(d), _p(g), _p(ws), _p(dx))
    ws0 = np.zeros(lib.hlp_workspace_words(n, h, w, 0), np.float32)
    lib.hlp_forward(C.byref(d), _p(x), _p(y), 0, _p(ws0), _p(quiet))
    maps = []
    for i, (_, cout) in enumerate(tw.CHANNELS):
        level = (0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4)[i]
        at = lib.hlp_map_offset(n, h, w, 1, i)
        maps.append(ws[at:at + n * cout * (h >> level) * (w >> level)].reshape(n, cout, h >> level, w >> level))
    return {"out": out, "dx": dx, "out_quiet": quiet, "maps": maps}
