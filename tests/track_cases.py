"""Cases, yardstick and helpers shared by tests/test_track_host.py, tests/test_track_abi.py and tests/test_gpu_track.py.  Test
infrastructure only.

  mesh case  faces  verts  what it holds (sheet, closed, one, wide: the meshes of tests/reg_cases.py, their `verts`)
  sheet      313    183    not a multiple of 256 faces, a boundary, one edge with three faces
  closed     80     42     an icosphere
  one        1      3      a single face
  wide       65884  33306  more than 256 * 256 faces: the reduction has a second level.  Generated, not in the fixture
  ties       12     36     disjoint faces on multiples of 2^-6.  Faces 0-3: two or all three edges exactly equal and longest (e1 = e2,
                           e2 = e3, e1 = e3, all three), so the first of the longest must win.  Faces 4-11: a triangle whose frame is
                           the identity, turned by +-170 degrees about axes near x, y, z and by +-20 degrees about (1, 2, 3): the
                           branches 1, 2, 3 and 0 of the quaternion, each once with w > 0 and once with w < 0 before the sign rule

  with every mesh: log_scales [F, 3] with columns 0 and 1 about the log of the radius of a disc of the mean face area (N(., 0.4)) and
  column 2 at -100, as the reference initialises it; logit_opacities [F, 1] ~ N(0, 2), both signs; and the upstream weights w_* of the
  backward passes.

  collision case  n_cloth x n_body  what it holds
  main            700 x 1100        neither a multiple of the 1024-query tile nor of the 32-target chunk; the search cuts the body
                                    into 5 slices of 220 (6 whole chunks and a partial one each)
  tiny            5 x 1
  short           3 x 31            less than one 32-target chunk
  even            300 x 2048
  dyadic          8 x 1100          multiples of 2^-6, axis-aligned normals, eps = 2^-10.  Rows 0-2 have two body vertices at exactly
                                    the same distance: 40 and 700 (different slices, so different workgroups), 230 and 250 (the same
                                    chunk), 1092 and 1097 (the partial chunk at the end); the lower index must win.  Row 3 sits at
                                    exactly d == eps: the slope is 1/2.  (At these sizes a slice never fills a second 1024-target LDS
                                    tile; two tiles of one workgroup need more than 65,536 body vertices.)
  the body is a sphere of radius 0.5 with outward normals, the cloth its points moved along the normal by U(-0.02, 0.02) and along
  the surface by N(0, 0.003): on both sides, so the hinge is active for about half.

A mesh result is the dict over MESH_TENSORS, a collision result the dict over COLLISION_TENSORS; the yardstick is the float64 run of
tests/track_twin_torch.py on the float32 inputs."""
import ctypes as C
import functools

import numpy as np
import torch

import hostbuild
import reg_cases as rc
import track_twin_torch as tw
from reg_cases import TINY, rel  # noqa: F401  (the yardstick is the regularisers')

MESH_CASES = ("sheet", "closed", "one", "ties", "wide")
FIXTURE_MESHES = ("sheet", "closed", "one", "ties")
COLLISION_CASES = ("main", "tiny", "short", "even", "dyadic")
SIZES = {"main": (700, 1100), "tiny": (5, 1), "short": (3, 31), "even": (300, 2048), "dyadic": (8, 1100)}
MODES = ("distance", "average", "cubed")
MESH_VALUES = ("means3D", "rotations", "scales", "opacities", "face_normals", "face_areas", "vertex_normals", "area", "scale", "opacity")
MESH_GRADS = ("d_means3D", "d_rotations", "d_scales", "d_opacities", "d_area_verts", "d_area_scales", "d_scale", "d_opacity")
MESH_TENSORS = MESH_VALUES + MESH_GRADS
COLLISION_TENSORS = ("distance", "average", "cubed", "d_distance", "d_average", "d_cubed")
TPB = 256
TIE_ROWS = {0: (40, 700), 1: (230, 250), 2: (1092, 1097)}
KINK_ROW = 3

# Measured on the CPU (tests/test_track_host.py::test_s32_is_the_measurement asserts it, from above and from below at half): S32 = the
# worst, over every case above and all its tensors, of max |t32 - t64| / max |t64| of the TWIN, its float32 run against its float64
# run.  The code under test plays no part in it.  Host restatement and GPU must lie within BOUND = 10 * S32 of the float64 twin, the
# factor of tests/reg_cases.py: FMA contraction, the device's division, sqrt and exp, a different summation order.
# measured 3.41e-7 (d_opacity of `wide`); d_opacity of `sheet` and `closed` 3.0e-7, vertex_normals of `wide` 3.0e-7, the rest 0 .. 1.9e-7
S32 = 3.5e-7
BOUND = 10 * S32


def _frozen(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _rotation(axis, degrees):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.radians(degrees)
    return np.eye(3) + np.sin(t) * k + (1 - np.cos(t)) * k @ k


def ties_mesh():
    tri = [[(0, 0, 0), (1, 2, 0), (2, 0, 0)],          # e1 = e2 = sqrt 5 > e3: e1
           [(0, 0, 0), (2, 0, 0), (1, 2, 0)],          # e2 = e3 > e1: e2
           [(1, 2, 0), (2, 0, 0), (0, 0, 0)],          # e1 = e3 > e2: e1
           [(1, 0, 0), (0, 1, 0), (0, 0, 1)]]          # all three sqrt 2: e1
    base = np.array([(0, 0, 0), (2, 0, 0), (0.5, 1, 0)])                         # frame = identity
    for axis in ((1, 0.1, 0.05), (0.1, 1, 0.05), (0.05, 0.1, 1)):
        for s in (1, -1):
            tri.append(base @ _rotation(axis, s * 170).T)
    for s in (1, -1):
        tri.append(base @ _rotation((1, 2, 3), s * 20).T)
    verts = np.round(np.array(tri, float).reshape(-1, 3) * 64) / 64 + np.repeat(np.arange(12), 3)[:, None] * (4, 0, 0)
    return verts, np.arange(36, dtype=np.int32).reshape(12, 3)


@functools.lru_cache(maxsize=None)
def mesh_case(name):
    """dict of read-only arrays: faces int32 [F, 3], verts [V, 3], log_scales [F, 3], logit_opacities [F, 1] and the upstream weights
    w_means3D [F, 3], w_rotations [F, 4], w_scales [F, 3], w_opacities [F, 1], w_matrices [F, 3, 3], all float32"""
    if name == "ties":
        verts, faces = ties_mesh()
    else:
        m = rc.mesh_case(name)
        verts, faces = m["verts"], m["faces"]
    verts = np.asarray(verts, np.float32)
    n_f = faces.shape[0]
    rng = np.random.default_rng(100 + MESH_CASES.index(name))
    area = tw.face_areas(torch.tensor(verts, dtype=torch.float64), torch.from_numpy(faces.astype(np.int64))).numpy()
    ls = np.full((n_f, 3), -100.0)
    ls[:, :2] = 0.5 * np.log(area.mean() / np.pi) + rng.normal(0, 0.4, (n_f, 2))
    c = {"faces": faces, "verts": verts, "log_scales": ls.astype(np.float32), "logit_opacities": rng.normal(0, 2, (n_f, 1)).astype(np.float32)}
    for k, w in (("means3D", 3), ("rotations", 4), ("scales", 3), ("opacities", 1)):
        c["w_" + k] = rng.normal(0, 1, (n_f, w)).astype(np.float32)
    c["w_matrices"] = rng.normal(0, 1, (n_f, 3, 3)).astype(np.float32)          # the fixture's upstream on the frame matrices
    return _frozen(c)


def _sphere(rng, m):
    p = rng.normal(0, 1, (m, 3))
    return p / np.linalg.norm(p, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def collision_case(name):
    """dict: va [n, 3], vb and nb [m, 3] float32, w [n] float32 (the upstream of the distance mode), eps"""
    n, m = SIZES[name]
    rng = np.random.default_rng(200 + COLLISION_CASES.index(name))
    if name == "dyadic":
        q = 2.0 ** -6
        # the body: distinct grid points with |x| >= 1, far from the planted ones near the origin
        grid = np.stack(np.meshgrid(np.arange(64, 64 + 11), np.arange(-5, 5), np.arange(-5, 5), indexing="ij"), -1).reshape(-1, 3)[:m] * q
        axes = np.eye(3)[rng.integers(0, 3, m)] * rng.choice([-1.0, 1.0], (m, 1))
        vb, nb = grid.copy(), axes.copy()
        va = np.zeros((n, 3))
        for row, (lo, hi) in TIE_ROWS.items():
            centre = np.array([0.0, 0.25 * row, 0.0])
            va[row] = centre
            vb[lo], vb[hi] = centre + (3 * q, 0, 0), centre - (3 * q, 0, 0)
            nb[lo], nb[hi] = (1, 0, 0), (0, 1, 0)
        eps = 2.0 ** -10
        vb[500], nb[500] = (0, -0.5, 0.25), (0, 0, 1)
        va[KINK_ROW] = vb[500] - np.array([0, q, eps])                           # d = -nb . (va - vb) = eps exactly
        for row in range(4, n):                                                  # plain rows on both sides of a planted vertex
            j = 600 + row
            vb[j], nb[j] = (0.5, 0.25 * row, 0.5), (0, 1, 0)
            va[row] = vb[j] + np.array([q, (-1) ** row * q, 0])
    else:
        eps = 1e-3
        nb = _sphere(rng, m)
        vb = 0.5 * nb
        j = rng.integers(0, m, n)
        va = vb[j] + nb[j] * rng.uniform(-0.02, 0.02, (n, 1)) + rng.normal(0, 0.003, (n, 3))
    c = {"va": va.astype(np.float32), "vb": vb.astype(np.float32), "nb": nb.astype(np.float32), "w": rng.normal(0, 1, n).astype(np.float32),
         "eps": eps}
    return _frozen(c)


# ---- the twin --------------------------------------------------------------------------------------------------------------------------

def _t(a, dtype, grad=False):
    return torch.tensor(np.asarray(a), dtype=dtype).requires_grad_(grad)


def mesh_twin(c, dtype=torch.float64):
    """-> dict over MESH_TENSORS (numpy) of the twin in `dtype`"""
    faces = torch.from_numpy(np.asarray(c["faces"]).astype(np.int64))
    v, ls, lo = _t(c["verts"], dtype, True), _t(c["log_scales"], dtype, True), _t(c["logit_opacities"], dtype, True)
    outs = dict(zip(("means3D", "rotations", "scales", "opacities"), tw.render_vars(v, faces, ls, lo)))
    terms = tw.terms(v, faces, ls, lo)
    r = {k: t.detach().numpy() for k, t in outs.items()}
    r.update(face_normals=tw.face_normals(v, faces).detach().numpy(), face_areas=tw.face_areas(v, faces).detach().numpy(),
             vertex_normals=tw.vertex_normals(v, faces).detach().numpy())
    r.update(zip(("area", "scale", "opacity"), terms.detach().numpy()))
    grad = lambda y, x: torch.autograd.grad(y, x, retain_graph=True)[0].numpy()
    for k, leaf in (("means3D", v), ("rotations", v), ("scales", ls), ("opacities", lo)):
        r["d_" + k] = grad((_t(c["w_" + k], dtype) * outs[k]).sum(), leaf)
    r.update(d_area_verts=grad(terms[0], v), d_area_scales=grad(terms[0], ls), d_scale=grad(terms[1], ls), d_opacity=grad(terms[2], lo))
    return r


def collision_twin(c, dtype=torch.float64, index=None):
    """-> dict over COLLISION_TENSORS plus index (int64 [n])"""
    va, vb, nb = _t(c["va"], dtype, True), _t(c["vb"], dtype), _t(c["nb"], dtype)
    j = tw.nearest(va.detach(), vb) if index is None else torch.from_numpy(np.asarray(index).astype(np.int64))
    r = {"index": j.numpy()}
    for mode in MODES:
        y = tw.collision(va, vb, nb, c["eps"], mode, j)
        r[mode] = y.detach().numpy()
        r["d_" + mode] = torch.autograd.grad((_t(c["w"], dtype) * y).sum() if mode == "distance" else y, va)[0].numpy()
    return r


@functools.lru_cache(maxsize=None)
def mesh64(name):
    """the float64 twin of a mesh case, computed once and shared"""
    return _frozen(mesh_twin(mesh_case(name)))


@functools.lru_cache(maxsize=None)
def collision64(name):
    return _frozen(collision_twin(collision_case(name)))


def corner_table(faces, n_v):
    """vertex -> corner items (item = 3 f + c), ascending within a vertex"""
    keys = np.asarray(faces).reshape(-1).astype(np.int64)
    start = np.zeros(n_v + 1, np.int32)
    start[1:] = np.cumsum(np.bincount(keys, minlength=n_v))
    return start, np.argsort(keys, kind="stable").astype(np.int32)


# ---- the host build of track_math.hpp -------------------------------------------------------------------------------------------------

def host_lib():
    lib = hostbuild.host_lib("hosttrack")
    vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
    lib.ht_render_vars.argtypes = [i32, i32] + [vp] * 8
    lib.ht_render_vars_backward.argtypes = [i32, i32] + [vp] * 14
    lib.ht_face_geometry.argtypes = [i32, i32] + [vp] * 4
    lib.ht_terms_forward.argtypes = [i32, i32] + [vp] * 5
    lib.ht_terms_backward.argtypes = [i32, i32] + [vp] * 11
    lib.ht_vertex_normals.argtypes = [i32, i32] + [vp] * 5
    lib.ht_collision_forward.argtypes = [i32, vp, vp, vp, i32, f32, i32, vp, vp, vp]
    lib.ht_collision_backward.argtypes = [i32, vp, i32, vp, vp, f32, i32, vp, vp]
    return lib


def sanitizer_program():
    """the same file as a stand-alone program under AddressSanitizer and UBSan (run as a subprocess; nothing is loaded into Python)"""
    return hostbuild.host_program("hosttrack", name="hosttrack_asan",
                                  flags=["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DHOSTTRACK_MAIN"])


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _nan(*shape):
    return np.full(shape, np.nan, np.float32)


def host_render_backward(c, g, want=(True, True, True)):
    """g: the four upstream arrays (None = zeros) -> (d_verts, d_log_scales, d_logit_opacities), None where not wanted"""
    faces, verts, ls, lo = [np.ascontiguousarray(c[k]) for k in ("faces", "verts", "log_scales", "logit_opacities")]
    n_f, n_v = faces.shape[0], verts.shape[0]
    start, items = corner_table(faces, n_v)
    g = [None if a is None else np.ascontiguousarray(a, np.float32) for a in g]
    d = [_nan(*a.shape) if w else None for w, a in zip(want, (verts, ls, lo))]
    stencil = _nan(n_f, 3, 3)
    host_lib().ht_render_vars_backward(n_f, n_v, _p(verts), _p(faces), _p(ls), _p(lo), *[_p(a) for a in g], _p(start), _p(items), _p(stencil),
                                       _p(d[0]), _p(d[1]), _p(d[2]))
    return d


def host_terms_backward(c, g, want=(True, True, True)):
    faces, verts, ls, lo = [np.ascontiguousarray(c[k]) for k in ("faces", "verts", "log_scales", "logit_opacities")]
    n_f, n_v = faces.shape[0], verts.shape[0]
    start, items = corner_table(faces, n_v)
    d = [_nan(*a.shape) if w else None for w, a in zip(want, (verts, ls, lo))]
    stencil = _nan(n_f, 3, 3)
    host_lib().ht_terms_backward(n_f, n_v, _p(verts), _p(faces), _p(ls), _p(lo), _p(np.asarray(g, np.float32)), _p(start), _p(items), _p(stencil),
                                 _p(d[0]), _p(d[1]), _p(d[2]))
    return d


def host_mesh(c):
    """-> dict over MESH_TENSORS of the host build: the forward passes, then one backward per output or term"""
    faces, verts, ls, lo = [np.ascontiguousarray(c[k]) for k in ("faces", "verts", "log_scales", "logit_opacities")]
    n_f, n_v = faces.shape[0], verts.shape[0]
    lib = host_lib()
    r = {"means3D": _nan(n_f, 3), "rotations": _nan(n_f, 4), "scales": _nan(n_f, 3), "opacities": _nan(n_f, 1), "face_normals": _nan(n_f, 3),
         "face_areas": _nan(n_f), "vertex_normals": _nan(n_v, 3)}
    lib.ht_render_vars(n_f, n_v, _p(verts), _p(faces), _p(ls), _p(lo), _p(r["means3D"]), _p(r["rotations"]), _p(r["scales"]), _p(r["opacities"]))
    lib.ht_face_geometry(n_f, n_v, _p(verts), _p(faces), _p(r["face_normals"]), _p(r["face_areas"]))
    start, items = corner_table(faces, n_v)
    lib.ht_vertex_normals(n_f, n_v, _p(verts), _p(faces), _p(start), _p(items), _p(r["vertex_normals"]))
    terms = _nan(3)
    lib.ht_terms_forward(n_f, n_v, _p(verts), _p(faces), _p(ls), _p(lo), _p(terms))
    r.update(zip(("area", "scale", "opacity"), terms))
    for i, (k, leaf) in enumerate((("means3D", 0), ("rotations", 0), ("scales", 1), ("opacities", 2))):
        g = [None] * 4
        g[i] = c["w_" + k]
        r["d_" + k] = host_render_backward(c, g)[leaf]
    d = host_terms_backward(c, (1, 0, 0))
    r["d_area_verts"], r["d_area_scales"] = d[0], d[1]
    r["d_scale"] = host_terms_backward(c, (0, 1, 0))[1]
    r["d_opacity"] = host_terms_backward(c, (0, 0, 1))[2]
    return r


def host_collision(c):
    """-> dict over COLLISION_TENSORS plus index"""
    va, vb, nb = [np.ascontiguousarray(c[k], np.float32) for k in ("va", "vb", "nb")]
    n, m = va.shape[0], vb.shape[0]
    lib = host_lib()
    r = {}
    for mode, name in enumerate(MODES):
        index, dist, value = np.full(n, -1, np.int32), _nan(n), _nan(1)
        lib.ht_collision_forward(n, _p(va), _p(vb), _p(nb), m, c["eps"], mode, _p(index), _p(dist), _p(value))
        g = np.ascontiguousarray(c["w"], np.float32) if name == "distance" else np.ones(1, np.float32)
        d_va = _nan(n, 3)
        lib.ht_collision_backward(n, _p(nb), m, _p(index), _p(dist), c["eps"], mode, _p(g), _p(d_va))
        r[name] = dist if name == "distance" else value[0]
        r["d_" + name] = d_va
        r["index"] = index
    return r
