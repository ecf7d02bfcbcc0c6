"""Cases, yardstick and helpers shared by tests/test_repose_host.py, tests/test_gpu_repose.py and tests/golden/make_golden_repose.py.
Test infrastructure only.

  search case   N x M        D  K        what it holds
  main          700 x 1100   3  10       N no multiple of the 256-query tile; the search cuts the targets into 5 slices of 220
  six           300 x 2100   6  10       more than two LDS tiles of 1,024 targets when searched as one slice; 9 slices of 234 otherwise
  full          5 x 16       3  16       K equals M
  short1/3/4    3 x 31       3  1, 3, 4  less than one tile, the list shorter than, and as long as, its padded length
  self3, self4  500 points   3  3, 4     knn_self: the k + 1 nearest of the set to itself, the first dropped
  dyadic        6 x 2101     3  4        integer coordinates, so every distance is exact.  Row 0: six targets at distance^2 9, at
                                         indices 5, 300, 1030, 1500, 2060, 2100 -- with the automatic 9 slices of 234 in slices
                                         0, 1, 4, 6, 8, 8; searched as one slice in LDS tiles 0, 0, 1, 1, 2, 2; 2100 is the single
                                         target of the last group of four.  More than K are tied at the K-th place: the four lowest
                                         indices must win, in ascending order.  Row 1: one nearer target at the high index 2099, then
                                         five tied at distance^2 4 at 2098, 7, 1100, 600, 1025.  Row 2: two targets ON the query
                                         (distance 0) at 900 and 50, then ties.  Rows 3-5: plain.
  The points of the random cases are uniform in the unit cube (the normal halves of `six`: unit vectors times 0.1).

  skinning case  dir    J   B  P     W          scale   transl
  pose_a         pose   55  5  1000  [1, P, J]  [B]     yes
  pose_b         pose   3   1  257   [B, P, J]  0-dim   None
  pose_c         pose   55  5  257   [B, P, J]  None    yes      W differs from frame to frame
  pose_d         pose   3   5  1     [1, P, J]  0-dim   None
  tpose_a        tpose  55  5  1000  [1, P, J]  0-dim   yes
  tpose_b        tpose  3   1  257   [B, P, J]  [B]     yes
  tpose_sum      tpose  55  5  257   [B, P, J]  0-dim   yes      rows of W sum to 0.8 .. 1.2: the last row of T is not (0, 0, 0, 1)
  tpose_one      tpose  55  1  1     [1, P, J]  0-dim   yes
  tpose_knn      tpose  55  2  257   searched   0-dim   yes      lbs_w=None: the 6-D search with normals, k = 10, V = 300
  tpose_knn3     tpose  55  1  100   searched   [B]     yes      lbs_w=None without normals: the 3-D search
  The searched cases blend ten body vertices per point, so their body is made coherent, as a real one is: the main joint of a body
  vertex follows its azimuth in twelve sectors, and the rotations stay within 30 degrees; with unrelated joints on neighbouring
  vertices and 90 degrees the blended T reached a condition number of 130 and the inverse alone set S32 at 1e-5.
  A [B, J, 4, 4]: per frame a random parent chain (parent[j] < j), every joint a rotation of up to 90 degrees about a random axis with
  a translation of order 1, composed along the chain.  W rows: a main joint with weight 0.55 .. 0.9, the rest on its parent and
  grandparent and a little on one random joint (J = 3: a Dirichlet draw).  The reference accepts a [B] scale on the way to the T-pose
  only for B == 1 (it divides [B, P, 3] by [B, 1]), so the [B] scale of a tpose case has B == 1.

The yardstick is the float64 run of tests/repose_twin_torch.py on the float32 inputs."""
import ctypes as C
import functools

import numpy as np
import torch

import hostbuild
import repose_twin_torch as tw
from reg_cases import TINY, rel  # noqa: F401  (the yardstick is the regularisers')

# name: (N, M, D, K, seed).  The seeds were chosen on the CPU so that the gap condition of test_repose_host.py holds.
KNN_CASES = {"main": (700, 1100, 3, 10, 2), "six": (300, 2100, 6, 10, 2), "full": (5, 16, 3, 16, 1), "short1": (3, 31, 3, 1, 1),
             "short3": (3, 31, 3, 3, 1), "short4": (3, 31, 3, 4, 1)}
SELF_CASES = {"self3": (500, 3, 1), "self4": (500, 4, 1)}
DYADIC = (6, 2101, 3, 4)
DYADIC_WANT = {0: [5, 300, 1030, 1500], 1: [2099, 7, 600, 1025], 2: [50, 900, 3, 1029]}
# name: (direction, J, B, P, W batched, scale kind, transl, seed)
SKIN_CASES = {"pose_a": ("pose", 55, 5, 1000, False, "B", True, 1), "pose_b": ("pose", 3, 1, 257, True, "0", False, 2),
              "pose_c": ("pose", 55, 5, 257, True, None, True, 3), "pose_d": ("pose", 3, 5, 1, False, "0", False, 4),
              "tpose_a": ("tpose", 55, 5, 1000, False, "0", True, 5), "tpose_b": ("tpose", 3, 1, 257, True, "B", True, 6),
              "tpose_sum": ("tpose", 55, 5, 257, True, "0", True, 7), "tpose_one": ("tpose", 55, 1, 1, False, "0", True, 8)}
# name: (J, B, P, V, k, normals, scale kind, seed)
SEARCHED_CASES = {"tpose_knn": (55, 2, 257, 300, 10, True, "0", 1), "tpose_knn3": (55, 1, 100, 300, 10, False, "B", 1)}
NORMAL_WEIGHT = 0.1
GAP = 1e-5           # 100 x the float32 rounding of the direct-form distance (about 1e-7 relative)

# Measured on the CPU (tests/test_repose_host.py::test_s32_is_the_measurement asserts it, from above and from below at half): S32 = the
# worst, over every case above and all its tensors, of max |t32 - t64| / max |t64| of the TWIN, its float32 run against its float64
# run.  The code under test plays no part in it.  Host restatement and GPU must lie within BOUND = 10 * S32 of the float64 twin, the
# factor of tests/track_cases.py: FMA contraction, the device's division, a different summation order, cofactors instead of LU.
# measured 3.54e-7 (T of `tpose_knn`: Shepard's weights go with distance^-4, which doubles the rounding of the distances before the
# inverse sees it); pnts and T of the two searched cases 3.2e-7 .. 3.5e-7, their W 2.2e-7 .. 2.5e-7, the rest 0 .. 1.7e-7
S32 = 3.6e-7
S32_SET_BY = "T of `tpose_knn`"
BOUND = 10 * S32
# the largest 2-norm condition number of a blended T over all cases (test_repose_host.py asserts it from above and at half from below):
# measured 66.2 (`tpose_a`, median 7.4); the case that sets S32 has 7.8
KAPPA = 67.0


def _frozen(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _unit(rng, n):
    p = rng.normal(0, 1, (n, 3))
    return p / np.linalg.norm(p, axis=1, keepdims=True)


# ---- the searches ----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def knn_case(name):
    """dict: p1 [N, D], p2 [M, D] float32, K"""
    if name == "dyadic":
        return _dyadic()
    if name in SELF_CASES:
        n, k, seed = SELF_CASES[name]
        p = _f32(np.random.default_rng(300 + seed).uniform(0, 1, (n, 3)))
        return _frozen({"p1": p, "p2": p, "K": k + 1, "self": True})
    n, m, d, k, seed = KNN_CASES[name]
    rng = np.random.default_rng(310 + 7 * list(KNN_CASES).index(name) + seed)
    p1, p2 = rng.uniform(0, 1, (n, 3)), rng.uniform(0, 1, (m, 3))
    if d == 6:
        p1, p2 = np.concatenate([p1, NORMAL_WEIGHT * _unit(rng, n)], 1), np.concatenate([p2, NORMAL_WEIGHT * _unit(rng, m)], 1)
    return _frozen({"p1": _f32(p1), "p2": _f32(p2), "K": k, "self": False})


def _dyadic():
    n, m, _, k = DYADIC
    # the background: distinct integer points with x >= 100, far from the queries on the y axis
    grid = np.stack(np.meshgrid(np.arange(100, 100 + 22), np.arange(10), np.arange(10), indexing="ij"), -1).reshape(-1, 3)[:m].astype(float)
    p2 = grid.copy()
    p1 = np.zeros((n, 3))
    for r in range(n):
        p1[r] = (0, 20 * r, 0)
    six = np.array([(3, 0, 0), (-3, 0, 0), (0, 3, 0), (0, -3, 0), (0, 0, 3), (0, 0, -3)], float)
    for j, off in zip((5, 300, 1030, 1500, 2060, 2100), six):
        p2[j] = p1[0] + off
    p2[2099] = p1[1] + (1, 0, 0)
    for j, off in zip((2098, 7, 1100, 600, 1025), six * 2 / 3):
        p2[j] = p1[1] + off
    p2[900] = p2[50] = p1[2]
    for j, off in zip((1029, 3, 2000), six[[0, 2, 4]]):
        p2[j] = p1[2] + off
    for r in range(3, n):                                                        # plain rows: distances^2 1, 4, 9, 16 at scattered indices
        for j, x in zip((400 + r, 10 + r, 1700 + r, 1200 + r), (1, 2, 3, 4)):
            p2[j] = p1[r] + (0, 0, x)
    return _frozen({"p1": _f32(p1), "p2": _f32(p2), "K": k, "self": False})


ALL_KNN = tuple(KNN_CASES) + tuple(SELF_CASES) + ("dyadic",)


def _t(a, dtype=torch.float64):
    return None if a is None else torch.tensor(np.asarray(a), dtype=dtype)


def knn_twin(c, dtype=torch.float64):
    """-> (dists [N, K], idx int64 [N, K]) of a search case, the self column NOT dropped"""
    d, i = tw.knn(_t(c["p1"], dtype), _t(c["p2"], dtype), c["K"])
    return d.numpy(), i.numpy()


@functools.lru_cache(maxsize=None)
def knn64(name):
    d, i = knn_twin(knn_case(name))
    d.setflags(write=False)
    i.setflags(write=False)
    return d, i


def relative_gaps(p1, p2, k):
    """float64: over every query, the smallest (d[r + 1] - d[r]) / d[r + 1] for the sorted distances of ranks 1 .. min(k + 1, M)"""
    d = tw.squared_distances(_t(p1), _t(p2)).sort(1).values[:, :min(k + 1, p2.shape[0])].numpy()
    if d.shape[1] < 2:
        return np.ones(d.shape[0])
    return ((d[:, 1:] - d[:, :-1]) / d[:, 1:]).min(1)


# ---- skinning --------------------------------------------------------------------------------------------------------------------------

def _rotation(axis, angle):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * k @ k


def _transforms(rng, B, J, max_angle=np.pi / 2):
    """-> (A [B, J, 4, 4], parent [J])"""
    parent = np.array([-1] + [int(rng.integers(max(0, j - 4), j)) for j in range(1, J)])
    A = np.zeros((B, J, 4, 4))
    for b in range(B):
        for j in range(J):
            local = np.eye(4)
            local[:3, :3] = _rotation(rng.normal(0, 1, 3), rng.uniform(-max_angle, max_angle))
            local[:3, 3] = rng.normal(0, 1, 3) * (1.0 if j == 0 else 0.3)
            A[b, j] = local if parent[j] < 0 else A[b, parent[j]] @ local
    return A, parent


def _weights(rng, n, J, parent, main=None):
    """rows that sum to 1: the main joint (random unless given), its parent and grandparent, a little on a random joint"""
    if J <= 3:
        return rng.dirichlet(np.full(J, 0.7), n)
    W = np.zeros((n, J))
    main = rng.integers(0, J, n) if main is None else main
    share = rng.uniform(0.55, 0.9, n)
    for i in range(n):
        p1 = max(parent[main[i]], 0)
        p2 = max(parent[p1], 0)
        rest = (1 - share[i]) * rng.dirichlet((2.0, 1.0, 0.3))
        W[i, main[i]] += share[i]
        W[i, p1] += rest[0]
        W[i, p2] += rest[1]
        W[i, rng.integers(0, J)] += rest[2]
    return W


def _by_azimuth(unit, J):
    """a main joint per body vertex that varies slowly over the sphere: twelve sectors of azimuth on every fourth joint"""
    sector = np.floor((np.arctan2(unit[:, 1], unit[:, 0]) + np.pi) / (2 * np.pi) * 12).astype(int) % 12
    return (4 * sector + 3) % J


def _scale(rng, kind, B):
    if kind is None:
        return None
    return _f32(rng.uniform(0.8, 1.25, B)) if kind == "B" else np.float32(rng.uniform(0.8, 1.25))


@functools.lru_cache(maxsize=None)
def skin_case(name):
    """dict of float32 arrays: verts [B, P, 3], W [B or 1, P, J], A [B, J, 4, 4], transl [B, 3] or None, scale ([B], 0-dim or None),
    direction; for a searched case also lbs [V, J], body [B, V, 3], normals [B, P, 3] and body_normals [B, V, 3] (or None), k"""
    if name in SEARCHED_CASES:
        J, B, P, V, k, normals, skind, seed = SEARCHED_CASES[name]
        rng = np.random.default_rng(500 + 11 * list(SEARCHED_CASES).index(name) + seed)
        A, parent = _transforms(rng, B, J, np.pi / 6)
        body_n = np.stack([_unit(rng, V) for _ in range(B)])
        body = 0.5 * body_n + rng.normal(0, 0.01, (B, V, 3))
        pick = rng.integers(0, V, (B, P))
        verts = np.stack([body[b, pick[b]] for b in range(B)]) + rng.normal(0, 0.03, (B, P, 3))
        vn = np.stack([body_n[b, pick[b]] for b in range(B)]) + rng.normal(0, 0.2, (B, P, 3))
        vn /= np.linalg.norm(vn, axis=-1, keepdims=True)
        c = {"direction": "tpose", "verts": _f32(verts), "W": None, "A": _f32(A), "transl": _f32(rng.normal(0, 0.5, (B, 3))),
             "scale": _scale(rng, skind, B), "lbs": _f32(_weights(rng, V, J, parent, _by_azimuth(body_n[0], J))), "body": _f32(body), "k": k,
             "normals": _f32(vn) if normals else None, "body_normals": _f32(body_n) if normals else None}
        return _frozen(c)
    direction, J, B, P, batched, skind, transl, seed = SKIN_CASES[name]
    rng = np.random.default_rng(400 + seed)
    A, parent = _transforms(rng, B, J)
    W = np.stack([_weights(rng, P, J, parent) for _ in range(B if batched else 1)])
    if name == "tpose_sum":
        W = W * rng.uniform(0.8, 1.2, (W.shape[0], P, 1))
    c = {"direction": direction, "verts": _f32(rng.normal(0, 0.6, (B, P, 3))), "W": _f32(W), "A": _f32(A),
         "transl": _f32(rng.normal(0, 0.5, (B, 3))) if transl else None, "scale": _scale(rng, skind, B)}
    return _frozen(c)


ALL_SKIN = tuple(SKIN_CASES) + tuple(SEARCHED_CASES)


def t_rows(P):
    """the points whose T (and searched W) the fixture keeps: every (P // 16)-th"""
    return np.arange(0, P, max(1, P // 16))


def searched_points(c, dtype=torch.float64):
    """the two point sets transform_to_t_pose hands to the search, per frame -> list of (points [P, D], body [V, D])"""
    out = []
    for b in range(c["verts"].shape[0]):
        p, v = _t(c["verts"][b], dtype), _t(c["body"][b], dtype)
        if c["normals"] is not None:
            p, v = tw.six(p, _t(c["normals"][b], dtype), NORMAL_WEIGHT), tw.six(v, _t(c["body_normals"][b], dtype), NORMAL_WEIGHT)
        out.append((p, v))
    return out


def skin_twin(c, dtype=torch.float64, idx=None):
    """-> dict pnts [1, B, P, 3], T [1, B, P, 4, 4], W [B or 1, P, J] (and idx int64 [B, P, k], dists [B, P, k] of a searched case); idx: the
    neighbours to use instead of the twin's own search (the float32 run of the S32 measurement keeps the float64 decisions)"""
    A, v = _t(c["A"], dtype), _t(c["verts"], dtype)
    r = {}
    if c["W"] is None:
        found = [tw.knn(p, b, c["k"]) for p, b in searched_points(c, dtype)]
        r["idx"] = np.stack([i.numpy() for _, i in found]) if idx is None else np.asarray(idx)
        if idx is not None:                      # the distances of the given neighbours, in this dtype
            found = [(tw.squared_distances(p, b).gather(1, torch.tensor(r["idx"][n])), None) for n, (p, b) in enumerate(searched_points(c, dtype))]
        r["dists"] = np.stack([d.numpy() for d, _ in found])
        W = torch.stack([tw.shepard_lbs(d, torch.tensor(r["idx"][n]), _t(c["lbs"], dtype)) for n, (d, _) in enumerate(found)])
    else:
        W = _t(c["W"], dtype)
    fn = tw.to_pose if c["direction"] == "pose" else tw.to_tpose
    pnts, T = fn(v, W, A, _t(c["transl"], dtype), _t(c["scale"], dtype))
    r.update(pnts=pnts[None].numpy(), T=T[None].numpy(), W=W.numpy())
    return r


@functools.lru_cache(maxsize=None)
def skin64(name):
    return _frozen(skin_twin(skin_case(name)))


def round_trip_expected(name):
    """what to the T-pose and back to the same pose gives in exact arithmetic, float64 [B, P, 3].  With T = [[M, tau], [0, sigma]] the
    reference drops the fourth coordinate 1 / sigma of T^-1 (v', 1), so the way back adds tau (1 - 1 / sigma) before the scale: the
    input returns exactly only where the row of W sums to 1 (float32 rows: to 1e-7)."""
    c = skin_case(name)
    T = tw.blend(_t(c["W"]), _t(c["A"]))
    s = 1.0 if c["scale"] is None else _t(c["scale"]).reshape(-1, 1, 1) if np.ndim(c["scale"]) else float(c["scale"])
    return (_t(c["verts"]) + s * T[:, :, :3, 3] * (1 - 1 / T[:, :, 3, 3])[..., None]).numpy()


def condition_numbers(name):
    """the 2-norm condition numbers of the blended T of a case, float64 -> [B, P]"""
    c = skin_case(name)
    W = _t(skin64(name)["W"])
    return torch.linalg.cond(tw.blend(W, _t(c["A"]))).numpy()


# ---- the host build of repose_math.hpp ---------------------------------------------------------------------------------------------------

def host_lib():
    lib = hostbuild.host_lib("hostrepose")
    vp, i32 = C.c_void_p, C.c_int32
    lib.hr_knn.argtypes = [i32] * 5 + [vp] * 5
    lib.hr_knn.restype = i32
    lib.hr_shepard.argtypes = [i32, i32, i32, vp, vp, vp, i32, i32, vp]
    lib.hr_shepard.restype = None
    lib.hr_skin.argtypes = [i32, i32, i32, i32, vp, i32, vp, i32, vp, vp, vp, i32, vp, vp]
    lib.hr_skin.restype = None
    return lib


def sanitizer_program():
    """the same file as a stand-alone program under AddressSanitizer and UBSan (run as a subprocess; nothing is loaded into Python)"""
    return hostbuild.host_program("hostrepose", name="hostrepose_asan",
                                  flags=["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DHOSTREPOSE_MAIN"])


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host_knn(p1, p2, k, slices=0):
    """-> (dists [N, k] float32, idx int32 [N, k], the number of slices used)"""
    p1, p2 = _f32(p1), _f32(p2)
    n, d = p1.shape
    dists, idx, used = np.full((n, k), np.nan, np.float32), np.full((n, k), -1, np.int32), C.c_int32(0)
    rc = host_lib().hr_knn(n, p2.shape[0], d, k, slices, _p(p1), _p(p2), _p(dists), _p(idx), C.addressof(used))
    assert rc == 0, rc
    return dists, idx, used.value


def host_shepard(d2, idx, power, lbs):
    d2 = _f32(d2)
    n, k = d2.shape
    if lbs is None:
        out = np.full((n, k), np.nan, np.float32)
        host_lib().hr_shepard(n, k, power, _p(d2), None, None, 0, 0, _p(out))
        return out
    lbs, idx = _f32(lbs), np.ascontiguousarray(idx, np.int32)
    out = np.full((n, lbs.shape[1]), np.nan, np.float32)
    host_lib().hr_shepard(n, k, power, _p(d2), _p(idx), _p(lbs), lbs.shape[0], lbs.shape[1], _p(out))
    return out


def host_skin(c, W=None, with_T=True):
    """-> dict pnts [1, B, P, 3], T [1, B, P, 4, 4] or None of the host build; W: the weights of a searched case"""
    W = _f32(c["W"] if W is None else W)
    verts, A = _f32(c["verts"]), _f32(c["A"])
    B, P, J = A.shape[0], verts.shape[1], A.shape[1]
    scale = None if c["scale"] is None else _f32(np.atleast_1d(c["scale"]))
    transl = None if c["transl"] is None else _f32(c["transl"])
    pnts = np.full((1, B, P, 3), np.nan, np.float32)
    T = np.full((1, B, P, 4, 4), np.nan, np.float32) if with_T else None
    host_lib().hr_skin(int(c["direction"] == "tpose"), B, P, J, _p(verts), int(B > 1), _p(W), int(W.shape[0] == B and B > 1), _p(A), _p(transl),
                       _p(scale), int(scale is not None and scale.shape[0] == B and B > 1), _p(pnts), _p(T))
    return {"pnts": pnts, "T": T}


def host_searched(c):
    """a searched case through the host build: search, Shepard's weights, skinning -> dict pnts, T, W, idx, dists"""
    found = [host_knn(p.numpy(), b.numpy(), c["k"]) for p, b in searched_points(c, torch.float32)]
    W = np.stack([host_shepard(d, i, 2, c["lbs"]) for d, i, _ in found])
    r = host_skin(c, W)
    r.update(W=W, idx=np.stack([i for _, i, _ in found]).astype(np.int64), dists=np.stack([d for d, _, _ in found]))
    return r
