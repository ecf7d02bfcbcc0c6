"""Cases, yardstick and helpers shared by tests/test_track4d_host.py, tests/test_track4d_abi.py and tests/test_gpu_track4d.py: the
uniform Laplacian and scale_ratio_loss of the 4D-DRESS tracking script (mpmavatar_amd/csrc/track4d_math.hpp).  Test infrastructure only.

  case     verts  faces  what it holds (sheet, closed, one, ties, wide: the meshes of tests/track_cases.py)
  sheet    183    313    not multiples of 256, a boundary, one edge shared by three faces, which must count once
  closed   42     80     the icosphere
  one      3      1      a single face: the variance is NaN
  ties     36     12     disjoint faces, the first four with equal longest edges
  flat     83     128    a 9 x 9 grid of vertices on multiples of 2^-6 (z affine in the grid indices), quads split along alternating
                         diagonals, so every interior vertex has 4 or 8 neighbours placed symmetrically about it: Lv == 0 exactly there,
                         in the float64 matrix product too (1/4 and 1/8 are exact).  Two more rows of `verts` that no face names: Lv = -v
  dyadic   12     4      hand-made rows on multiples of 2^28, so large that b + 1e-8 == b and m + 1e-8 == m in float64 as in float32
                         and the equalities below hold in both: face 0 has s0 == s1, face 1 has r == 5 exactly, face 2 has q == 1
                         exactly (edges 3, 4, 5 times 2^28), face 3 has two equal longest edges and s1 > s0
  wide     33306  65884  generated: the face reductions have a second level (258 partials)
  grid257  66049  131072 generated, the Laplacian only: 259 partials of the vertex reduction, its second level

  The scale cases carry their own log_scales: with those of tests/track_cases.py (N(., 0.4)) no face of sheet, closed or ties has
  r > 5 and the first hinge would be identically zero.  Here columns 0 and 1 are the log of the radius of a disc of the mean face
  area + N(0, 1.0), column 2 is -100, and `scale` = exp(log_scales) in float32 is the input of the direct calls.

A result is a dict over LAP_TENSORS or SCALE_TENSORS; the yardstick is the float64 run of tests/track4d_twin_torch.py on the float32
inputs."""
import ctypes as C
import functools

import numpy as np
import torch

import hostbuild
import reg_cases as rc
import track4d_twin_torch as tw
import track_cases as tc

SCALE_CASES = ("sheet", "closed", "one", "ties", "flat", "dyadic", "wide")
LAP_CASES = SCALE_CASES + ("grid257",)
FIXTURE_CASES = ("sheet", "closed", "one", "ties", "flat", "dyadic")
LAP_TENSORS = ("lv", "laplacian", "d_laplacian")
SCALE_VALUES = ("scale_ratio", "scale_edge_ratio", "scale_edge_ratio_var")
SCALE_GRADS = ("d_ratio_scale", "d_edge_verts", "d_edge_scale", "d_var_verts", "d_var_scale")
SCALE_TENSORS = SCALE_VALUES + SCALE_GRADS
WEIGHTS = (10.0, 1000.0, 10.0)               # train_mesh_lbs_4ddress.py:369; "d_log_scales" is the gradient of the weighted sum
TH = (5.0, 1.0)
TPB = 256
BIG = 2.0 ** 28

# Measured on the CPU (tests/test_track4d_host.py::test_s32_is_the_measurement asserts it, from above and from below at half): S32 =
# the worst, over every case above and all its tensors (LAP_TENSORS, SCALE_TENSORS and d_log_scales), of max |t32 - t64| / max |t64|
# of the TWIN, its float32 run against its float64 run.  The code under test plays no part in it.  Host restatement and GPU must lie
# within BOUND = 10 * S32 of the float64 twin, the factor of tests/track_cases.py.
# measured 3.69e-6 (d_laplacian of `grid257`); d_laplacian of `wide` 3.1e-6 and of `sheet` 2.5e-6, lv of `wide` 1.8e-6: the direction
# Lv / |Lv| of a difference of nearby vertices; every scale tensor 0 .. 3.5e-7
S32 = 4.0e-6
BOUND = 10 * S32


def _frozen(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def rel(t, t64):
    """max |t - t64| / max |t64| over every element that float64 leaves finite; the NaNs (the variance of a single face and what it
    hands on) must sit in the same places.  A float64 tensor that is zero throughout is compared absolutely."""
    t, t64 = np.asarray(t, np.float64), np.asarray(t64, np.float64)
    assert t.shape == t64.shape, (t.shape, t64.shape)
    nan = np.isnan(t64)
    assert np.array_equal(np.isnan(t), nan), "NaN in other places than the float64 twin's"
    if nan.all() or t64.size == 0:
        return 0.0
    a, b = np.where(nan, 0.0, t), np.where(nan, 0.0, t64)
    top = np.abs(b).max()
    return float(np.abs(a - b).max() / (top if top > 0 else 1.0))


def flat_mesh():
    n, q = 9, 2.0 ** -6
    i, j = [a.reshape(-1) for a in np.meshgrid(np.arange(n), np.arange(n))]
    verts = np.stack([i * q, j * q, (i + 2 * j) * q], 1)
    qi, qj = [a.reshape(-1) for a in np.meshgrid(np.arange(n - 1), np.arange(n - 1))]
    v00 = qj * n + qi
    v10, v01, v11 = v00 + 1, v00 + n, v00 + n + 1
    even = ((qi + qj) % 2 == 0)[:, None]
    first = np.where(even, np.stack([v00, v10, v11], 1), np.stack([v00, v10, v01], 1))
    second = np.where(even, np.stack([v00, v11, v01], 1), np.stack([v10, v11, v01], 1))
    faces = np.stack([first, second], 1).reshape(-1, 3)
    verts = np.concatenate([verts, [[0.5, 0.25, 0.125], [-0.25, 0.5, 1.0]]])
    return verts, faces.astype(np.int32)


def dyadic_mesh():
    tri = np.array([[(0, 0, 0), (2, 0, 0), (0, 1, 0)], [(0, 0, 0), (2, 0, 0), (0, 1, 0)], [(0, 0, 0), (3, 0, 0), (0, 4, 0)],
                    [(0, 0, 0), (1, 2, 0), (2, 0, 0)]], float)
    verts = (tri + np.arange(4)[:, None, None] * (8.0, 0.0, 0.0)).reshape(-1, 3) * BIG
    scale = np.array([[4 * BIG, 4 * BIG], [5 * BIG, BIG], [5 * BIG, 2 * BIG], [BIG, 2 * BIG]])
    return verts, np.arange(12, dtype=np.int32).reshape(4, 3), scale


def grid257_mesh():
    h = 0.02
    grid, faces = rc.sheet_mesh(256, 256, h, fin=False)
    rng = np.random.default_rng(57)
    i, j = np.round(grid[:, 0] / h), np.round(grid[:, 1] / h)
    # the recipe of `wide` (tests/reg_cases.py): folded into a stack 16 spacings wide, so that fp32 offsets stay small, and columns
    # alternately 1.25 h and 0.75 h wide, so that no vertex sits at the mean of its neighbours and Lv / |Lv| is well conditioned
    fold = lambda t: np.where(t % 32 <= 16, t % 32, 32 - t % 32)
    verts = h * np.stack([fold(i + 0.25 * (i % 2)), fold(j), 0.05 * (i // 16) + 0.6 * (j // 16)], 1)
    verts = 1.3 * (verts + rng.normal(0, 1, grid.shape) * h * (0.01, 0.01, 0.08)) + rng.normal(0, 0.01 * h, grid.shape)
    return verts, faces


@functools.lru_cache(maxsize=None)
def case(name):
    """dict of read-only arrays: faces int32 [F, 3], verts [V, 3], log_scales [F, 3], scale [F, 3] = exp(log_scales), float32"""
    scale = None
    if name == "flat":
        verts, faces = flat_mesh()
    elif name == "dyadic":
        verts, faces, scale = dyadic_mesh()
    elif name == "grid257":
        verts, faces = grid257_mesh()
    else:
        m = tc.mesh_case(name)
        verts, faces = m["verts"], m["faces"]
    verts = np.asarray(verts, np.float32)
    n_f = faces.shape[0]
    rng = np.random.default_rng(400 + LAP_CASES.index(name))
    ls = np.full((n_f, 3), -100.0)
    if scale is None:
        v64, f64 = torch.tensor(verts, dtype=torch.float64), torch.from_numpy(faces.astype(np.int64))
        t = v64[f64]
        area = (torch.linalg.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 1]).norm(dim=1) / 2).numpy()
        ls[:, :2] = 0.5 * np.log(area.mean() / np.pi) + rng.normal(0, 1.0, (n_f, 2))
    else:
        ls[:, :2] = np.log(scale)
    ls = ls.astype(np.float32)
    sc = np.exp(ls.astype(np.float64)).astype(np.float32)
    if scale is not None:
        sc[:, :2] = scale                                                        # the dyadic values themselves
    return _frozen({"faces": faces, "verts": verts, "log_scales": ls, "scale": sc})


# ---- the twin --------------------------------------------------------------------------------------------------------------------------

def _t(a, dtype, grad=False):
    return torch.tensor(np.asarray(a), dtype=dtype).requires_grad_(grad)


def _faces(c):
    return torch.from_numpy(np.asarray(c["faces"]).astype(np.int64))


def lap_twin(c, dtype=torch.float64):
    """-> dict over LAP_TENSORS (numpy) of the twin in `dtype`"""
    v = _t(c["verts"], dtype, True)
    m = tw.laplacian_matrix(_faces(c), v.shape[0], dtype)
    y = tw.laplacian(m, v)
    return {"lv": tw.apply(m, v).detach().numpy(), "laplacian": y.detach().numpy(), "d_laplacian": torch.autograd.grad(y, v)[0].numpy()}


def scale_twin(c, dtype=torch.float64):
    """-> dict over SCALE_TENSORS plus d_log_scales (through scale = exp(log_scales), the weighted sum)"""
    faces = _faces(c)
    v, s = _t(c["verts"], dtype, True), _t(c["scale"], dtype, True)
    terms = tw.scale_ratio_loss(v, faces, s, *TH)
    r = {k: t.detach().numpy() for k, t in zip(SCALE_VALUES, terms)}
    grad = lambda y, x: torch.autograd.grad(y, x, retain_graph=True)[0].numpy()
    r.update(d_ratio_scale=grad(terms[0], s), d_edge_verts=grad(terms[1], v), d_edge_scale=grad(terms[1], s), d_var_verts=grad(terms[2], v),
             d_var_scale=grad(terms[2], s))
    ls = _t(c["log_scales"], dtype, True)
    chained = tw.scale_ratio_loss(v, faces, torch.exp(ls), *TH)
    r["d_log_scales"] = grad(sum(w * t for w, t in zip(WEIGHTS, chained)), ls)
    return r


@functools.lru_cache(maxsize=None)
def lap64(name):
    return _frozen(lap_twin(case(name)))


@functools.lru_cache(maxsize=None)
def scale64(name):
    return _frozen(scale_twin(case(name)))


def adjacency(faces, n_v):
    """the CSR vertex adjacency as numpy int32 (start [V + 1], nbr [2 |E|]), ascending within a row"""
    row, col = tw.adjacency(torch.from_numpy(np.asarray(faces).astype(np.int64)), n_v)
    start = np.zeros(n_v + 1, np.int32)
    start[1:] = np.cumsum(np.bincount(row.numpy(), minlength=n_v))
    return start, col.numpy().astype(np.int32)


# ---- the host build of track4d_math.hpp ---------------------------------------------------------------------------------------------

def host_lib():
    lib = hostbuild.host_lib("hosttrack4d")
    vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
    lib.h4_laplacian_forward.argtypes = [i32] + [vp] * 5
    lib.h4_laplacian_backward.argtypes = [i32] + [vp] * 5
    lib.h4_scale_forward.argtypes = [i32, i32, vp, vp, vp, f32, f32, vp]
    lib.h4_scale_backward.argtypes = [i32, i32, vp, vp, vp, f32, f32] + [vp] * 7
    return lib


def sanitizer_program():
    """the same file as a stand-alone program under AddressSanitizer and UBSan (run as a subprocess; nothing is loaded into Python)"""
    return hostbuild.host_program("hosttrack4d", name="hosttrack4d_asan",
                                  flags=["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DHOSTTRACK4D_MAIN"])


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _nan(*shape):
    return np.full(shape, np.nan, np.float32)


def host_lap(c):
    """-> dict over LAP_TENSORS of the host build"""
    verts = np.ascontiguousarray(c["verts"], np.float32)
    n_v = verts.shape[0]
    start, nbr = adjacency(c["faces"], n_v)
    lib = host_lib()
    lv, value, d = _nan(n_v, 3), _nan(1), _nan(n_v, 3)
    lib.h4_laplacian_forward(n_v, _p(verts), _p(start), _p(nbr), _p(lv), _p(value))
    lib.h4_laplacian_backward(n_v, _p(lv), _p(start), _p(nbr), _p(np.ones(1, np.float32)), _p(d))
    return {"lv": lv, "laplacian": value[0], "d_laplacian": d}


def host_scale_backward(c, g, th=TH, want=(True, True)):
    """g [3] -> (d_verts, d_scale), None where not wanted"""
    faces, verts, scale = [np.ascontiguousarray(c[k]) for k in ("faces", "verts", "scale")]
    n_f, n_v = faces.shape[0], verts.shape[0]
    lib = host_lib()
    terms = _nan(4)
    lib.h4_scale_forward(n_f, n_v, _p(verts), _p(faces), _p(scale), th[0], th[1], _p(terms))
    start, items = tc.corner_table(faces, n_v)
    d = [_nan(*a.shape) if w else None for w, a in zip(want, (verts, scale))]
    stencil = _nan(n_f, 3, 3)
    lib.h4_scale_backward(n_f, n_v, _p(verts), _p(faces), _p(scale), th[0], th[1], _p(terms), _p(np.asarray(g, np.float32)), _p(start), _p(items),
                          _p(stencil), _p(d[0]), _p(d[1]))
    return d


def host_scale(c, th=TH):
    """-> dict over SCALE_TENSORS of the host build: the forward, then one backward per term"""
    faces, verts, scale = [np.ascontiguousarray(c[k]) for k in ("faces", "verts", "scale")]
    terms = _nan(4)
    host_lib().h4_scale_forward(faces.shape[0], verts.shape[0], _p(verts), _p(faces), _p(scale), th[0], th[1], _p(terms))
    r = dict(zip(SCALE_VALUES, terms[:3]))
    r["d_ratio_verts"], r["d_ratio_scale"] = host_scale_backward(c, (1, 0, 0), th)
    r["d_edge_verts"], r["d_edge_scale"] = host_scale_backward(c, (0, 1, 0), th)
    r["d_var_verts"], r["d_var_scale"] = host_scale_backward(c, (0, 0, 1), th)
    return r
