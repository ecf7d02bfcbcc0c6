"""Cases, yardstick and helpers shared by tests/test_reg_host.py, tests/test_reg_abi.py and tests/test_gpu_reg.py.  Test
infrastructure only.

  mesh case  faces  verts  what it holds
  sheet      313    183    an open 12 x 13 grid of quads (spacing 0.02) split into triangles, diagonals towards the nearer corner, plus
                           one "fin" triangle on an interior diagonal: that edge has three faces, so two rows of the neighbour array
                           are cut and the array is not symmetric; 47 faces carry their own index (the boundary and the fin); more
                           than one 256-thread workgroup, the second partly filled.  verts0 = grid + N(0, 0.12 h), verts = verts0 +
                           N(0, 0.15 h)
  closed     80     42     an icosphere of radius 0.03, perturbed the same way: no boundary, no self rows
  one        1      3      a single triangle: every neighbour is itself
  two        2      4      two triangles sharing an edge, folded by about 50 degrees
  flat       312    182    the sheet without fin or noise on multiples of 2^-6, verts == verts0: every dot product is exactly 1
  wide       65884  33306  a 181 x 182 sheet folded into a stack, generated here, no fixture: ceil(F / 256) = 258 partials, more than
                           the 256 lanes of the final workgroup take in one pass (F > 256 * 256 = 65536; 181 x 181 quads would give
                           65522)

  Gaussian case  n    what it holds
  main           300  _xyz ~ N(0, 0.8), _scaling ~ N(-0.9, 0.5), _opacity ~ N(0, 2), radii in 0..3, thresholds 1.0 and 0.6
  one            1    a single visible row
  none_visible   300  main with all radii 0

A mesh result is the [3] terms and the gradient of each term on verts (d_normal, d_iso, d_area); a Gaussian result is the [3] terms
and the gradients of their sum on the three parameters (each term reads exactly one).  The yardstick is the float64 run of
tests/reg_twin_torch.py on the float32 inputs; set-up included, as the reference takes neighbor_dist and neighbor_weight from
verts_orig[0] in the working precision.  The inputs of sheet, closed, one and Gaussians main are also in tests/golden/reg.npz beside
the reference's own results (tests/golden/make_golden_reg.py reads them from here)."""
import ctypes as C
import functools

import numpy as np
import torch

import hostbuild
import reg_twin_torch as tw

MESH_CASES = ("sheet", "closed", "one", "two", "flat")
GAUSS_CASES = ("main", "one", "none_visible")
MESH_VALUES, MESH_GRADS = ("normal", "iso", "area"), ("d_normal", "d_iso", "d_area")
GAUSS_VALUES, GAUSS_GRADS = ("opacity", "xyz", "scale"), ("_opacity", "_xyz", "_scaling")
MESH_TENSORS, GAUSS_TENSORS = MESH_VALUES + MESH_GRADS, GAUSS_VALUES + GAUSS_GRADS
K, TPB = 3, 256
THRESHOLDS = (1.0, 0.6)
WIDE = (181, 182)

# Measured on the CPU (tests/test_reg_host.py::test_s32_is_the_measurement asserts it, from above and from below at half):
# S32 = the worst, over the cases above (wide excepted: 65,884 faces fold fp32 coordinates 16 spacings wide) and all their tensors, of
# max |t32 - t64| / max |t64| of the TWIN, its float32 run against its float64 run.  The code under test plays no part in it.  Host
# restatement and GPU must lie within BOUND = 10 * S32 of the float64 twin -- the factor of tests/raster_grad_scenes.py and
# tests/shade_cases.py: FMA contraction, the device's division, sqrt and exp, a different summation order.
S32 = 9.0e-7   # measured 8.87e-7 (d_iso of `sheet`); the other figures 0 .. 8.0e-7 (iso of `two`); `wide`, not counted, 2.9e-6
BOUND = 10 * S32


def sheet_mesh(nx, ny, h, fin):
    """-> (grid vertices [(nx + 1)(ny + 1) (+ 1), 3] float64, faces int32): quad (i, j) is cut along the diagonal that points to the
    nearer corner of the sheet, so each of the four corner quads has a triangle with two boundary edges; every triangle is
    counter-clockwise seen from +z.  fin: one more vertex above the middle quad's diagonal and one more triangle on that diagonal."""
    i, j = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1))
    verts = np.stack([i.reshape(-1) * h, j.reshape(-1) * h, np.zeros(i.size)], 1)
    qi, qj = [a.reshape(-1) for a in np.meshgrid(np.arange(nx), np.arange(ny))]
    v00 = qj * (nx + 1) + qi
    v10, v01, v11 = v00 + 1, v00 + nx + 1, v00 + nx + 2
    other = (qi < nx / 2) == (qj < ny / 2)
    first = np.where(other[:, None], np.stack([v00, v10, v01], 1), np.stack([v00, v10, v11], 1))
    second = np.where(other[:, None], np.stack([v10, v11, v01], 1), np.stack([v00, v11, v01], 1))
    faces = np.stack([first, second], 1).reshape(-1, 3)
    if fin:
        q = (ny // 2) * nx + nx // 2
        assert not other[q]
        a, b = v00[q], v11[q]
        verts = np.concatenate([verts, [(verts[a] + verts[b]) / 2 + (0.0, 0.0, 0.8 * h)]])
        faces = np.concatenate([faces, [[a, b, verts.shape[0] - 1]]])
    return verts, faces.astype(np.int32)


def icosphere(radius):
    """the icosahedron with every face split in four: 42 vertices, 80 faces, outward orientation"""
    p = (1 + 5 ** 0.5) / 2
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, float) / np.linalg.norm(x) for x in v]
    mid, out = {}, []

    def m(a, b):
        key = (min(a, b), max(a, b))
        if key not in mid:
            v.append((v[a] + v[b]) / np.linalg.norm(v[a] + v[b]))
            mid[key] = len(v) - 1
        return mid[key]

    for a, b, c in f:
        ab, bc, ca = m(a, b), m(b, c), m(c, a)
        out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
    return radius * np.array(v), np.array(out, np.int32)


@functools.lru_cache(maxsize=None)
def mesh_case(name):
    """dict of read-only arrays: faces int32 [F, 3], verts0 and verts float32 [V, 3]"""
    h = 0.02
    if name in ("sheet", "wide"):
        nx, ny = (12, 13) if name == "sheet" else WIDE
        grid, faces = sheet_mesh(nx, ny, h, fin=name == "sheet")
        seed = 0
    elif name == "flat":
        h = 2.0 ** -6
        grid, faces = sheet_mesh(12, 13, h, fin=False)
    elif name == "closed":
        grid, faces = icosphere(0.03)
        seed = 1
    elif name == "one":
        grid, faces, seed = np.array([[0, 0, 0], [h, 0, 0], [0, h, 0]], float), np.array([[0, 1, 2]], np.int32), 2
    else:
        grid, faces, seed = np.array([[0, 0, 0], [h, 0, 0], [h, h, 0], [0, h, 0.9 * h]], float), np.array([[0, 1, 2], [0, 2, 3]], np.int32), 3
    if name == "flat":
        verts0 = verts = grid
    elif name == "wide":
        # Two things a sheet of 65,884 faces cannot leave to chance.  Its extent: 182 spacings across, fp32 centre offsets would
        # carry 4e-5 of relative error in any implementation, so the sheet is folded zig-zag every 16 quads in both directions into a
        # stack 16 spacings wide (layers 0.05 h apart).  Its kinks: the columns are alternately 1.25 h and 0.75 h wide (areas 25 % off
        # their mean either way) and verts is verts0 stretched by 1.3 (every distance 30 % above neighbor_dist) with noise of 0.01 h;
        # verts0 carries 0.08 h of noise in z, so that no face is flat against its neighbours
        rng = np.random.default_rng(seed)
        i, j = np.round(grid[:, 0] / h), np.round(grid[:, 1] / h)
        fold = lambda t: np.where(t % 32 <= 16, t % 32, 32 - t % 32)
        grid = h * np.stack([fold(i + 0.25 * (i % 2)), fold(j), 0.05 * (i // 16) + 0.6 * (j // 16)], 1)
        verts0 = grid + rng.normal(0, 1, grid.shape) * h * (0.01, 0.01, 0.08)
        verts = 1.3 * verts0.astype(np.float32) + rng.normal(0, 0.01 * h, grid.shape)
    else:
        rng = np.random.default_rng(seed)
        verts0 = grid + rng.normal(0, 0.12 * h, grid.shape)
        verts = verts0.astype(np.float32) + rng.normal(0, 0.15 * h, grid.shape)
    c = {"faces": faces, "verts0": verts0.astype(np.float32), "verts": verts.astype(np.float32)}
    for v in c.values():
        v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def neighbors(name):
    """the package's adjacent_faces on the case's faces (test_reg_host.py checks it against the reference's array of the fixture)"""
    from mpmavatar_amd.regularizers import adjacent_faces
    nb = adjacent_faces(mesh_case(name)["faces"]).astype(np.int32)
    nb.setflags(write=False)
    return nb


@functools.lru_cache(maxsize=None)
def gauss_case(name):
    """dict of read-only arrays: _opacity [n, 1], _xyz [n, 3], _scaling [n, 3] float32, radii int32 [n]"""
    n = 1 if name == "one" else 300
    rng = np.random.default_rng(7 if name == "one" else 0)
    c = {"_xyz": rng.normal(0, 0.8, (n, 3)), "_scaling": rng.normal(-0.9, 0.5, (n, 3)), "_opacity": rng.normal(0, 2, (n, 1))}
    c = {k: v.astype(np.float32) for k, v in c.items()}
    c["radii"] = rng.integers(0, 4, n).astype(np.int32)
    if name == "one":
        c["radii"][:] = 2
        c["_xyz"][0] = (0.9, -0.8, 0.5)
        c["_scaling"][0] = (-0.2, -1.5, 0.1)
    if name == "none_visible":
        c["radii"][:] = 0
    for v in c.values():
        v.setflags(write=False)
    return c


TINY = 1e-9


def rel(t, t64):
    """max |t - t64| / max |t64| over EVERY element.  Where the float64 tensor stays below TINY it holds the twin's own rounding of
    an exact zero (| n . n - 1 | and its slope where every neighbour is the face itself) or the sqrt(1e-20) constants of iso, and the
    error is the absolute one: such a tensor must be zero to within BOUND of the unit vectors and unit weights it is made of."""
    t, t64 = np.asarray(t, np.float64), np.asarray(t64, np.float64)
    assert t.shape == t64.shape, (t.shape, t64.shape)
    if t64.size == 0:
        return 0.0
    top = np.abs(t64).max()
    return float(np.abs(t - t64).max() / (top if top >= TINY else 1.0))


# ---- the twin --------------------------------------------------------------------------------------------------------------------------

def mesh_twin(c, nb, dtype=torch.float64):
    """-> dict over MESH_TENSORS (numpy) of the twin in `dtype`, set-up included"""
    faces, nbl = torch.from_numpy(np.asarray(c["faces"]).astype(np.int64)), torch.from_numpy(np.asarray(nb).astype(np.int64))
    nd, nw = tw.setup(torch.tensor(c["verts0"], dtype=dtype), faces, nbl)
    verts = torch.tensor(c["verts"], dtype=dtype, requires_grad=True)
    terms = tw.mesh_terms(verts, faces, nbl, nd, nw)
    out = dict(zip(MESH_VALUES, terms.detach().numpy()))
    for i, k in enumerate(MESH_GRADS):
        out[k] = torch.autograd.grad(terms[i], verts, retain_graph=True)[0].numpy()
    return out


def gauss_twin(c, dtype=torch.float64):
    t = {k: torch.tensor(c[k], dtype=dtype, requires_grad=True) for k in GAUSS_GRADS}
    terms = tw.gauss_terms(t["_opacity"], t["_xyz"], t["_scaling"], torch.from_numpy(np.asarray(c["radii"]) > 0), *THRESHOLDS)
    grads = torch.autograd.grad(terms.sum(), [t[k] for k in GAUSS_GRADS])
    out = dict(zip(GAUSS_VALUES, terms.detach().numpy()))
    out.update({k: g.numpy() for k, g in zip(GAUSS_GRADS, grads)})
    return out


@functools.lru_cache(maxsize=None)
def mesh64(name):
    """the float64 twin of a mesh case, computed once and shared"""
    out = mesh_twin(mesh_case(name), neighbors(name))
    for k in MESH_GRADS:
        out[k].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def gauss64(name):
    out = gauss_twin(gauss_case(name))
    for k in GAUSS_GRADS:
        out[k].setflags(write=False)
    return out


def stencil_table(faces, nb, n_v):
    """vertex -> stencil items (item = 12 f + 3 s + c of S[f, s, c] = faces[nbx[f, s], c], nbx[f, 0] = f), ascending within a vertex"""
    nbx = np.concatenate([np.arange(faces.shape[0])[:, None], nb], 1)
    keys = np.asarray(faces)[nbx].reshape(-1).astype(np.int64)
    start = np.zeros(n_v + 1, np.int32)
    start[1:] = np.cumsum(np.bincount(keys, minlength=n_v))
    return start, np.argsort(keys, kind="stable").astype(np.int32)


# ---- the host build of reg_math.hpp ---------------------------------------------------------------------------------------------------

def host_lib():
    lib = hostbuild.host_lib("hostreg")
    vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
    lib.hr_mesh_forward.argtypes = [i32, i32] + [vp] * 8
    lib.hr_mesh_backward.argtypes = [i32, i32] + [vp] * 11
    lib.hr_gauss_forward.argtypes = [i32] + [vp] * 5 + [f32, f32, vp, vp]
    lib.hr_gauss_backward.argtypes = [i32] + [vp] * 5 + [f32, f32] + [vp] * 5
    return lib


def sanitizer_program():
    """the same file as a stand-alone program under AddressSanitizer and UBSan (run as a subprocess; nothing is loaded into Python)"""
    return hostbuild.host_program("hostreg", name="hostreg_asan",
                                  flags=["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DHOSTREG_MAIN"])


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host_setup(c, nb):
    """neighbor_dist, neighbor_weight as MeshRegularizer takes them: one forward on verts0 that stores the squared distances"""
    faces, v0 = np.ascontiguousarray(c["faces"], np.int32), np.ascontiguousarray(c["verts0"], np.float32)
    n_f, n_v = faces.shape[0], v0.shape[0]
    sq, zero = np.full((n_f, K), np.nan, np.float32), np.zeros((n_f, K), np.float32)
    terms, stats = np.zeros(3, np.float32), np.zeros(2, np.float32)
    host_lib().hr_mesh_forward(n_f, n_v, _p(v0), _p(faces), _p(np.ascontiguousarray(nb, np.int32)), _p(zero), _p(zero), _p(terms), _p(stats), _p(sq))
    return np.sqrt(sq), np.exp(np.float32(-2000) * sq)


def host_mesh(c, nb, g=None):
    """forward, and a backward per term (g = None) or one backward with upstream g [3] -> dict over MESH_TENSORS, or
    {"terms", "d_verts", "d_stencil"}"""
    faces, verts, nb = np.ascontiguousarray(c["faces"], np.int32), np.ascontiguousarray(c["verts"], np.float32), np.ascontiguousarray(nb, np.int32)
    n_f, n_v = faces.shape[0], verts.shape[0]
    nd, nw = host_setup(c, nb)
    lib = host_lib()
    terms, stats = np.full(3, np.nan, np.float32), np.full(2, np.nan, np.float32)
    lib.hr_mesh_forward(n_f, n_v, _p(verts), _p(faces), _p(nb), _p(nd), _p(nw), _p(terms), _p(stats), None)
    start, items = stencil_table(faces, nb, n_v)

    def back(up):
        up = np.asarray(up, np.float32)
        d_stencil, d_verts = np.full((n_f, 1 + K, 3, 3), np.nan, np.float32), np.full((n_v, 3), np.nan, np.float32)
        lib.hr_mesh_backward(n_f, n_v, _p(verts), _p(faces), _p(nb), _p(nd), _p(nw), _p(stats), _p(up), _p(start), _p(items), _p(d_stencil), _p(d_verts))
        return d_verts, d_stencil

    if g is not None:
        d_verts, d_stencil = back(g)
        return {"terms": terms, "d_verts": d_verts, "d_stencil": d_stencil}
    out = dict(zip(MESH_VALUES, terms))
    for i, k in enumerate(MESH_GRADS):
        out[k] = back(np.eye(3)[i])[0]
    return out


def host_gauss(c, mask=False, g=(1.0, 1.0, 1.0)):
    """-> dict over GAUSS_TENSORS plus n_visible"""
    opa, xyz, scl = [np.ascontiguousarray(c[k], np.float32) for k in GAUSS_GRADS]
    n = xyz.shape[0]
    radii = np.ascontiguousarray(c["radii"], np.int32)
    vis = (None, np.ascontiguousarray(radii > 0).view(np.uint8)) if mask else (radii, None)
    lib = host_lib()
    terms, n_visible = np.full(3, np.nan, np.float32), np.full(1, -1, np.int32)
    lib.hr_gauss_forward(n, _p(opa), _p(xyz), _p(scl), _p(vis[0]), _p(vis[1]), *THRESHOLDS, _p(terms), _p(n_visible))
    d = [np.full(a.shape, np.nan, np.float32) for a in (opa, xyz, scl)]
    lib.hr_gauss_backward(n, _p(opa), _p(xyz), _p(scl), _p(vis[0]), _p(vis[1]), *THRESHOLDS, _p(n_visible), _p(np.asarray(g, np.float32)),
                          _p(d[0]), _p(d[1]), _p(d[2]))
    out = dict(zip(GAUSS_VALUES, terms))
    out.update(_opacity=d[0], _xyz=d[1], _scaling=d[2], n_visible=int(n_visible[0]))
    return out
