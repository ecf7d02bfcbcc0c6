"""Cases, yardstick and helpers shared by tests/test_shade_host.py, tests/test_shade_abi.py and tests/test_gpu_shade.py.  Test
infrastructure only.

  case   n     faces  map    K    degrees  what it holds
  main   300   37     5 x 7  16   0..3     face 0 without a Gaussian, face 1 with 72 (longer than a wave), unsorted binding; uv exactly
                                           at (-1, -1) and (1, 1) (faces 2, 3), one uv wholly outside the map (face 4), two in the
                                           half-texel border (faces 5, 6), two faces on one uv (7, 8); the two right-hand columns of
                                           the map are tapped by face 3 alone, so most of their texels have no tap
  k4     53    11     3 x 4  4    0..1     K = 4: features_rest has three rows
  one    1     1      1 x 1  16   0..3     a single Gaussian, face and texel

The loss of a case at a degree is sum(w * colors); its gradients go to features_dc, features_rest, means3D and shadow_map (GRADS).
The yardstick is the float64 run of tests/shade_twin_torch.py on the float32 inputs.  The inputs of `main` are also in
tests/golden/shade.npz beside the reference's own results (tests/golden/make_golden_shade.py reads them from here)."""
import ctypes as C
import functools

import numpy as np
import torch

import hostbuild
import shade_twin_torch as tw

CASES = ("main", "k4", "one")
DEGREES = {"main": (0, 1, 2, 3), "k4": (0, 1), "one": (0, 1, 2, 3)}
GRADS = ("features_dc", "features_rest", "means3D", "shadow_map")
TENSORS = ("colors",) + GRADS
CLAMP_MARGIN = 1e-4      # tests/raster_grad_scenes.py: no unclamped sh + 0.5 within this distance of zero
MIN_CAM_DISTANCE = 0.1

# Measured on the CPU (tests/test_shade_host.py::test_s32_is_the_measurement asserts it, from above and from below at half):
# S32 = the worst, over the cases, their degrees and the five tensors, of max |t32 - t64| / max |t64| of the TWIN, its float32 run
# against its float64 run.  The code under test plays no part in it.  Host restatement and GPU must lie within BOUND = 10 * S32 of
# the float64 twin -- the factor of the rasteriser's gradient tests (tests/raster_grad_scenes.py): FMA contraction, the device's
# division and sqrt, a different summation order (here only inside the two CSR walks).
S32 = 5.3e-7   # measured 5.110e-7 (shadow_map of `main` at degree 0); the other 49 figures 0 .. 5.0e-7
BOUND = 10 * S32

_SHAPES = {"main": (300, 37, 5, 7, 16, 0), "k4": (53, 11, 3, 4, 4, 1), "one": (1, 1, 1, 1, 16, 2)}   # n, faces, H, W, K, seed


@functools.lru_cache(maxsize=None)
def case(name):
    """dict of read-only arrays: binding int32 [n], face_uv [F, 2], shadow_map [H, W], features_dc [n, 1, 3], features_rest
    [n, K - 1, 3], means3D [n, 3], campos [3], w [n, 3] (float32)"""
    n, n_f, H, W, K, seed = _SHAPES[name]
    rng = np.random.default_rng(seed)
    uv = rng.uniform(-1.15, 1.15, (n_f, 2))
    if name == "main":
        uv[9:, 0] = rng.uniform(-1.15, 0.2, n_f - 9)            # nothing else reaches the two right-hand columns
        uv[2], uv[3], uv[4] = (-1.0, -1.0), (1.0, 1.0), (3.0, -2.5)
        uv[5], uv[6] = (-1.0 - 0.5 / W, 0.2), (0.1, 1.0 + 0.6 / H)
        uv[7] = uv[8] = (-0.35, 0.45)
        binding = rng.integers(2, n_f, n)
        binding[rng.choice(n, 75, replace=False)] = 1
        binding[:7] = np.arange(8, 1, -1)                       # every special face holds a Gaussian; the start is descending
        binding[7] = 1
    elif name == "k4":
        binding = rng.integers(0, n_f, n)
    else:
        uv[0] = (0.1, -0.2)
        binding = np.zeros(n, np.int64)
    c = {"binding": binding.astype(np.int32), "face_uv": uv.astype(np.float32),
         "shadow_map": rng.uniform(0.2, 1.0, (H, W)).astype(np.float32),
         "features_dc": rng.normal(0, 0.5, (n, 1, 3)).astype(np.float32),
         "features_rest": rng.normal(0, 0.3, (n, K - 1, 3)).astype(np.float32),
         "means3D": rng.normal(0, 1.0, (n, 3)).astype(np.float32), "campos": np.array([0.2, -0.1, 2.5], np.float32),
         "w": rng.normal(size=(n, 3)).astype(np.float32)}
    for v in c.values():
        v.setflags(write=False)
    return c


def rel(t, t64):
    """max |t - t64| / max |t64| over EVERY element; a tensor that is all zero in float64 must be all zero"""
    t, t64 = np.asarray(t, np.float64), np.asarray(t64, np.float64)
    assert t.shape == t64.shape, (t.shape, t64.shape)
    if t64.size == 0:
        return 0.0
    top = np.abs(t64).max()
    if top == 0.0:
        assert (t == 0).all()
        return 0.0
    return float(np.abs(t - t64).max() / top)


def twin(c, deg, dtype=torch.float64, features=True, shadow=True):
    """the twin's colours and gradients of sum(w * colors) in `dtype` -> dict over TENSORS (numpy); a tensor that plays no part
    (features=False / shadow=False: the NULL forms) is None"""
    t = {k: torch.tensor(np.asarray(c[k]), dtype=dtype, requires_grad=True) for k in GRADS}
    campos, uv = torch.tensor(c["campos"], dtype=dtype), torch.tensor(c["face_uv"], dtype=dtype)
    b = torch.from_numpy(np.asarray(c["binding"]).astype(np.int64))
    colors = tw.shaded(deg, t["features_dc"] if features else None, t["features_rest"], t["means3D"], campos,
                       t["shadow_map"] if shadow else None, uv, b)
    loss = (torch.tensor(c["w"], dtype=dtype) * colors).sum()
    grads = torch.autograd.grad(loss, [t[k] for k in GRADS], allow_unused=True)
    out = {"colors": colors.detach().numpy()}
    for k, g in zip(GRADS, grads):
        used = shadow if k == "shadow_map" else features
        out[k] = None if not used else (np.zeros(t[k].shape) if g is None else g.numpy())
    return out


@functools.lru_cache(maxsize=None)
def t64(name, deg):
    """the float64 twin of a case at a degree, computed once and shared"""
    out = twin(case(name), deg)
    for v in out.values():
        v.setflags(write=False)
    return out


def raw_sh(c, deg):
    """the unclamped sh + 0.5 [n, 3] in float64"""
    f = lambda k: torch.tensor(c[k], dtype=torch.float64)
    return tw.sh_colour(deg, f("features_dc"), f("features_rest"), f("means3D"), f("campos"))[1].numpy()


# ---- the two tables, with numpy's equivalents of the torch ops the package uses ---------------------------------------------------------

def csr(keys, n_keys):
    """key -> items: (start [n_keys + 1] int32, items int32 in ascending item index within a key)"""
    keys = np.asarray(keys, np.int64).reshape(-1)
    items = np.argsort(keys, kind="stable").astype(np.int32)
    start = np.zeros(n_keys + 1, np.int32)
    start[1:] = np.cumsum(np.bincount(keys, minlength=n_keys))
    return start, items


def brute_force_texel_table(uv, H, W):
    """texel -> taps (4 * face + corner, ascending), by loops over shade_math.hpp's own taps on the host"""
    idx, _ = host_taps(uv, H, W)
    lists = [[] for _ in range(H * W)]
    for f in range(idx.shape[0]):
        for k in range(4):
            if idx[f, k] >= 0:
                lists[idx[f, k]].append(4 * f + k)
    start = np.zeros(H * W + 1, np.int32)
    start[1:] = np.cumsum([len(l) for l in lists])
    return start, np.array([t for l in lists for t in l], np.int32)


# ---- the host build of shade_math.hpp ----------------------------------------------------------------------------------------------

def host_lib():
    return hostbuild.host_lib("hostshade")


def sanitizer_program():
    """the same file as a stand-alone program under AddressSanitizer and UBSan (run as a subprocess; nothing is loaded into Python)"""
    return hostbuild.host_program("hostshade", name="hostshade_asan",
                                  flags=["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DHOSTSHADE_MAIN"])


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, np.float32)


def host_taps(uv, H, W):
    uv = _f32(uv)
    n_f = uv.shape[0]
    idx, w = np.full((n_f, 4), -7, np.int32), np.full((n_f, 4), np.nan, np.float32)
    host_lib().hs_taps(n_f, _p(uv), H, W, _p(idx), _p(w))
    return idx, w


def host_run(c, deg, features=True, shadow=True, g=True):
    """forward and the three backward stages on the host -> dict over TENSORS (None where a tensor plays no part)"""
    n = c["binding"].shape[0]
    H, W = c["shadow_map"].shape
    n_f = c["face_uv"].shape[0]
    K = 1 + c["features_rest"].shape[1]
    binding, uv, smap = np.ascontiguousarray(c["binding"], np.int32), _f32(c["face_uv"]), _f32(c["shadow_map"])
    dc, rest, means, campos = [_f32(c[k]) for k in ("features_dc", "features_rest", "means3D", "campos")]
    if not features:
        dc = rest = means = campos = None
    if not shadow:
        smap = uv = None
    new = lambda a: None if a is None else np.full(a.shape, np.nan, np.float32)
    colors, d_dc, d_rest, d_means, d_map = np.full((n, 3), np.nan, np.float32), new(dc), new(rest), new(means), new(smap)
    fstart = fitems = tstart = titems = scratch = None
    if shadow:
        fstart, fitems = csr(binding, n_f)
        tstart, titems = brute_force_texel_table(uv, H, W)
        scratch = np.full(n + n_f, np.nan, np.float32)
    shared = [n, n_f if shadow else 0, _p(binding) if shadow else None, _p(means), _p(campos), deg, K if features else 0, _p(dc), _p(rest),
              _p(smap), H if shadow else 0, W if shadow else 0, _p(uv)]
    lib = host_lib()
    lib.hs_forward(*shared, _p(colors))
    lib.hs_backward(*shared, _p(_f32(c["w"])) if g else None, _p(d_dc), _p(d_rest), _p(d_means), _p(fstart), _p(fitems), _p(tstart), _p(titems),
                    _p(d_map), _p(scratch))
    return dict(zip(TENSORS, (colors, d_dc, d_rest, d_means, d_map)))
