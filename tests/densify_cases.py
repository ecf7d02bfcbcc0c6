"""Cases, yardstick and helpers shared by tests/test_densify_host.py, tests/test_gpu_densify.py and
tests/golden/make_golden_densify.py.  Test infrastructure only.

  case       n    faces  R   what it holds
  main       777  40     15  more than two 256-row scan tiles plus a remainder; clones, splits and prunes (a screen size is given, so
                             the world-size test is on); face 0 has a single Gaussian, which is flagged; every Gaussian of face 1 is
                             flagged, one of them cloned and one split, so the face rule binds twice; rows with denom = 0; rows with
                             g == max_grad exactly (denom = 1), one on each side of the clone / split line
  tiny       5    3      0   zero-width _features_rest: a clone, a split, a pruned row, two that stay
  none       50   8      2   nothing selected and nothing pruned: the output is the input
  all_split  70   6      1   every row is split (no screen size)
  empty      0    4      3   no Gaussians at all

Every case carries Adam moments for all six parameters, noise [n, 2, 3], and the inputs of one statistics update (grad, radii and
the statistics before it).  The builder asserts in float64 that, apart from the exact-equality rows, every compared quantity -- g,
max(gs), sigmoid(_opacity), the child's world scale -- is at least MARGIN = 1e-3 relative away from its threshold, so that no fp32
exp, division or sigmoid can flip a decision, and that each case holds the situations it is named for.  Copied data (features,
moments) are multiples of 1/64 so that the fixture compresses; what enters arithmetic is full-entropy fp32."""
import ctypes as C
import functools

import numpy as np
import torch

import densify_twin_torch as tw
import hostbuild

CASES = ("main", "tiny", "none", "all_split", "empty")
PARAMS = tw.PARAMS
WIDTH = lambda c, k: int(np.prod(c[k].shape[1:]))
MAX_GRAD = 2.0 ** -12          # exactly an fp32, so that g == max_grad exists in every precision
HYPER = dict(max_grad=MAX_GRAD, min_opacity=0.005, extent=2.0, percent_dense=0.01)
MARGIN = 1e-3
COMPUTED = ("_xyz", "_scaling")               # what a split child computes; everything else is copied

# Measured on the CPU (tests/test_densify_host.py::test_s32_is_the_measurement asserts it, from above and from below at half):
# S32 = the worst, over the cases above, of max |t32 - t64| / max |t64| of the TWIN, its float32 run against its float64 run, over
# the new _xyz and _scaling, the three statistics after an update and the reset opacities.  The code under test plays no part in it.
# Host restatement and GPU must lie within BOUND = 10 * S32 of the float64 twin -- the factor of tests/reg_cases.py: FMA
# contraction, the device's division, sqrt, exp and log, a different order in the 3 x 3 product.
S32 = 8.0e-8   # measured 7.97e-8 (the new _xyz of `all_split`); the other figures 0 .. 5.4e-8 (add_accum of `none`)
BOUND = 10 * S32


def _coarse(rng, shape, scale=64):
    return (rng.integers(-scale, scale + 1, shape) / 64.0).astype(np.float32)


def _build(name):
    n, n_f, r, seed = {"main": (777, 40, 15, 0), "tiny": (5, 3, 0, 1), "none": (50, 8, 2, 2), "all_split": (70, 6, 1, 3), "empty": (0, 4, 3, 4)}[name]
    rng = np.random.default_rng(seed)
    h = dict(HYPER, max_screen_size=20 if name in ("main", "tiny") else None)
    dense, world = h["percent_dense"] * h["extent"], 0.1 * h["extent"]
    fs = rng.uniform(0.02, 0.08, (n_f, 1))
    binding = rng.integers(2, n_f, n) if name == "main" else rng.integers(0, n_f, n)
    # log of g / max_grad, of max(gs) / dense, and the opacity: two clusters each, nothing within 0.01 of a line
    away = lambda size, p: np.where(rng.random(size) < p, 1.0, -1.0) * (0.01 + rng.exponential(0.7, size))
    lg, lm = away(n, 0.45), away(n, 0.5)
    opa = np.where(rng.random(n) < 0.12, rng.uniform(-9.0, -6.0, n), rng.uniform(-4.0, 4.0, n))
    denom = rng.integers(0, 6, n).astype(np.float64)
    if name == "main":
        binding[0], binding[1:4] = 0, 1                                   # the single-Gaussian face; the all-flagged face
        opa[0:4] = (-7.0, -6.5, -8.0, -7.5)
        lg[0:4], lm[0:4] = (-1.0, -0.5, 0.4, 0.6), (0.3, -0.3, -0.5, 0.5)  # stays, stays, cloned, split
        denom[0:4] = (2, 0, 3, 1)
        denom[10:14], denom[14:16], lg[14:16], lm[14:16] = 0, 1, 0.0, (-0.4, 0.4)   # denom = 0; g == max_grad: a clone and a split
        opa[14:16] = (1.0, 2.0)
        for f in range(2, n_f):                                           # every other face keeps an unflagged, unselected row
            i = 20 + f
            binding[i], opa[i], lg[i], lm[i], denom[i] = f, 1.5, -1.0, -0.5, 2
    if name == "tiny":
        binding[:] = (0, 0, 1, 1, 2)
        lg[:], lm[:], opa[:], denom[:] = (0.5, 0.7, -1.0, -0.6, -0.3), (-0.5, 0.6, -0.2, -0.4, 0.3), (1.0, 0.5, -7.0, 2.0, 0.0), (1, 2, 3, 1, 4)
    if name == "none":
        lg, lm, opa = -np.abs(lg), -np.abs(lm), np.abs(opa) - 3.0
        opa[opa < -4.0] = 0.5
    if name == "all_split":
        lg, lm, opa, denom = np.abs(lg), np.abs(lm), rng.uniform(-3.0, 3.0, n), np.maximum(denom, 1.0)
    m = dense * np.exp(lm)
    for line in (world, 1.6 * world):                                     # max(gs) and max(gs) / 1.6 against the world limit
        m = np.where(np.abs(np.log(m / line)) < 0.01, m * 1.03, m)
    gs = m[:, None] * np.concatenate([np.ones((n, 1)), rng.uniform(0.2, 0.9, (n, 2))], 1)
    gs = np.take_along_axis(gs, np.argsort(rng.random((n, 3)), 1), 1)     # the largest component anywhere in the row
    c = {"_xyz": rng.normal(0, 0.5, (n, 3)), "_scaling": np.log(gs / fs[binding]), "_rotation": rng.normal(0, 1, (n, 4)), "_opacity": opa[:, None],
         "accum": (MAX_GRAD * np.exp(lg) * denom)[:, None], "denom": denom[:, None], "face_scaling": fs, "noise": rng.normal(0, 1, (n, 2, 3)),
         "grad": rng.normal(0, 1e-3, (n, 3)), "add_accum": rng.uniform(0, 1e-2, (n, 1)), "add_max_radii": rng.integers(0, 9, n)}
    c = {k: np.ascontiguousarray(v, np.float32) for k, v in c.items()}
    c["add_denom"] = rng.integers(0, 5, (n, 1)).astype(np.float32)
    c["_features_dc"], c["_features_rest"] = _coarse(rng, (n, 1, 3)), _coarse(rng, (n, r, 3), 8)
    for k in PARAMS:
        c["m_" + k], c["v_" + k] = _coarse(rng, c[k].shape, 8), np.abs(_coarse(rng, c[k].shape, 8))
    c["binding"], c["radii"] = binding.astype(np.int32), rng.integers(0, 12, n).astype(np.int32)
    c["radii"][rng.random(n) < 0.3] = 0
    c["n_faces"], c["hyper"] = n_f, h
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _check(name, c)
    return c


def decisions(c, dtype=np.float64):
    """-> dict of the compared quantities of a case in `dtype` and the decisions they lead to"""
    h = c["hyper"]
    lim = {k: np.float32(v) for k, v in dict(max_grad=h["max_grad"], dense=h["percent_dense"] * h["extent"], min_opacity=h["min_opacity"],
                                             world=0.1 * h["extent"]).items()}
    with np.errstate(invalid="ignore", divide="ignore"):
        g = np.nan_to_num((c["accum"].astype(dtype) / c["denom"].astype(dtype)).reshape(-1), nan=0.0)
    fs = c["face_scaling"].astype(dtype)[c["binding"]]
    gs = np.exp(c["_scaling"].astype(dtype)) * fs
    m = gs.max(1) if gs.size else np.zeros(0, dtype)
    mc = (np.exp(np.log(gs / fs / dtype(1.6))) * fs).max(1) if gs.size else m
    sig = 1 / (1 + np.exp(-c["_opacity"].astype(dtype).reshape(-1)))
    sel = g >= lim["max_grad"]
    d = dict(g=g, m=m, mc=mc, sig=sig, lim=lim, clone=sel & (m <= lim["dense"]), split=sel & (m > lim["dense"]), faint=sig < lim["min_opacity"])
    big = bool(h["max_screen_size"])
    d["flag_self"], d["flag_child"] = d["faint"] | (big & (m > lim["world"])), d["faint"] | (big & (mc > lim["world"]))
    return d


def _check(name, c):
    d, h, n = decisions(c), c["hyper"], c["binding"].shape[0]
    lim = d["lim"]
    exact = d["g"] == lim["max_grad"]
    rel = lambda v, t: np.abs(v / np.float64(t) - 1)
    assert (rel(d["g"][~exact & (d["g"] > 0)], lim["max_grad"]) >= MARGIN).all(), name
    assert (rel(d["m"], lim["dense"]) >= MARGIN).all() and (rel(d["sig"], lim["min_opacity"]) >= MARGIN).all(), name
    assert (rel(d["m"], lim["world"]) >= MARGIN).all() and (rel(d["mc"][d["split"]], lim["world"]) >= MARGIN).all(), name
    d32 = decisions(c, np.float32)
    for k in ("clone", "split", "flag_self", "flag_child"):
        assert np.array_equal(d[k], d32[k]), (name, k)
    assert (c["denom"][exact] == 1).all()
    per_face = np.bincount(c["binding"], minlength=c["n_faces"])
    if name == "main":
        assert n == 777 and n > 3 * 256 and n % 256 != 0 and c["_features_rest"].shape[1] == 15
        assert d["clone"].sum() >= 50 and d["split"].sum() >= 50 and (d["flag_self"] & ~d["faint"]).sum() >= 5 and d["faint"].sum() >= 50
        assert (d["flag_child"] & ~d["faint"] & d["split"]).sum() >= 1 and (d["flag_self"] & ~d["flag_child"] & d["split"]).sum() >= 1
        assert per_face[0] == 1 and d["flag_self"][0] and not d["clone"][0] and not d["split"][0]
        on1 = c["binding"] == 1
        assert per_face[1] == 3 and d["faint"][on1].all() and d["clone"][on1].sum() == 1 and d["split"][on1].sum() == 1
        assert (c["denom"] == 0).sum() >= 5 and exact.sum() == 2 and d["clone"][exact].sum() == 1 and d["split"][exact].sum() == 1
        assert (per_face[2:] >= 2).all()
    if name == "tiny":
        assert c["_features_rest"].shape == (5, 0, 3) and d["clone"].sum() == 1 and d["split"].sum() == 1 and d["faint"].sum() == 1
    if name == "none":
        assert not (d["clone"] | d["split"] | d["flag_self"]).any() and n == 50
    if name == "all_split":
        assert d["split"].all() and not d["faint"].any() and not h["max_screen_size"] and n > 64
    if name == "empty":
        assert n == 0 and c["n_faces"] == 4


@functools.lru_cache(maxsize=None)
def case(name):
    return _build(name)


def rel(t, t64):
    """max |t - t64| / max |t64| over every element"""
    t, t64 = np.asarray(t, np.float64), np.asarray(t64, np.float64)
    assert t.shape == t64.shape, (t.shape, t64.shape)
    if t64.size == 0:
        return 0.0
    top = np.abs(t64).max()
    return float(np.abs(t - t64).max() / (top if top > 0 else 1.0))


# ---- the twin --------------------------------------------------------------------------------------------------------------------------

def twin(c, dtype=torch.float64, device="cpu", mask=False):
    """-> dict of numpy arrays: the densification (the six parameters, m_* / v_*, binding, binding_counter, src, kind, counts), the
    statistics after an update (add_*; mask: from radii > 0 as a bool) and the reset opacities"""
    t = lambda k: torch.tensor(c[k], dtype=dtype, device=device)
    params = {k: t(k) for k in PARAMS}
    moments = {k: (t("m_" + k), t("v_" + k)) for k in PARAMS}
    binding = torch.tensor(c["binding"].astype(np.int64), device=device)
    r = tw.densify_and_prune(params, moments, binding, c["n_faces"], t("face_scaling"), t("accum"), t("denom"), t("noise"), **c["hyper"])
    out = {k: r[k].cpu().numpy() for k in PARAMS}
    for k in PARAMS:
        out["m_" + k], out["v_" + k] = (m.cpu().numpy() for m in r["moments"][k])
    out.update(binding=r["binding"].cpu().numpy().astype(np.int32), binding_counter=r["binding_counter"].cpu().numpy().astype(np.int32),
               src=r["src"].cpu().numpy(), kind=r["kind"].cpu().numpy(), counts=np.array(r["counts"], np.int32))
    radii = torch.tensor(c["radii"], device=device)
    a = tw.stats_add(t("add_accum"), t("add_denom"), t("add_max_radii"), t("grad"), radii > 0 if mask else radii)
    out.update(add_accum=a[0].cpu().numpy(), add_denom=a[1].cpu().numpy(), add_max_radii=a[2].cpu().numpy())
    out["reset"] = tw.reset_opacity(t("_opacity")).cpu().numpy()
    return out


@functools.lru_cache(maxsize=None)
def twin64(name, mask=False):
    """the float64 twin of a case, computed once and shared"""
    out = twin(case(name), mask=mask)
    for v in out.values():
        v.setflags(write=False)
    return out


EXACT = ("binding", "binding_counter", "src", "kind", "counts", "_features_dc", "_features_rest", "_opacity", "_rotation") + \
    tuple(p + k for p in ("m_", "v_") for k in PARAMS)
NUMERIC = COMPUTED + ("add_accum", "add_denom", "add_max_radii", "reset")


def compare(got, want, bound, label, copied_exact=True):
    """integer outputs, copied tensors and the copied rows of _xyz and _scaling bit for bit; the computed values within `bound`"""
    for k in EXACT:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k].astype(got[k].dtype)), (label, k)
    new = want["kind"] == 2
    for k in NUMERIC:
        if k not in got:
            continue
        err = rel(got[k], want[k])
        print(label, k, "%.3g of bound %.3g" % (err, bound))
        assert np.isfinite(np.asarray(got[k], np.float64)).all() and err <= bound, (label, k, err)
        if k in COMPUTED and copied_exact:
            assert np.array_equal(got[k][~new], want[k][~new].astype(got[k].dtype)), (label, k, "copied rows")


# ---- the host build of densify_math.hpp ------------------------------------------------------------------------------------------------

def host_lib():
    lib = hostbuild.host_lib("hostdensify")
    vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
    lib.hd_stats_add.argtypes = [i32] + [vp] * 6
    lib.hd_plan.argtypes = [i32, i32] + [vp] * 6 + [f32] * 4 + [i32] + [vp] * 3
    lib.hd_emit.argtypes = [i32, i32, i32] + [vp] * 8 + [i32] + [vp] * 8
    lib.hd_reset_opacity.argtypes = [i32, vp, vp]
    return lib


def sanitizer_program():
    """the same file as a stand-alone program under AddressSanitizer and UBSan (run as a subprocess; nothing is loaded into Python)"""
    return hostbuild.host_program("hostdensify", name="hostdensify_asan",
                                  flags=["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DHOSTDENSIFY_MAIN"])


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host(c, mask=False):
    """the serial loops of tests/hostdensify/hostdensify.cpp on a case -> the dict of `twin`, in fp32"""
    lib, h = host_lib(), c["hyper"]
    n, n_f = c["binding"].shape[0], c["n_faces"]
    f32 = lambda x: float(np.float32(x))
    keep, at, counts = np.zeros(3 * n + 1, np.uint32), np.zeros(3 * n + 1, np.uint32), np.full(8, -1, np.int32)
    lib.hd_plan(n, n_f, _p(c["_scaling"]), _p(c["_opacity"]), _p(c["binding"]), _p(c["face_scaling"]), _p(c["accum"]), _p(c["denom"]),
                f32(h["max_grad"]), f32(h["percent_dense"] * h["extent"]), f32(h["min_opacity"]), f32(0.1 * h["extent"]),
                1 if h["max_screen_size"] else 0, _p(keep), _p(at), _p(counts))
    assert counts[4] == 0
    n_out = int(counts[0])
    out, table = {}, []
    for k in PARAMS:
        for prefix, mode in (("", {"_xyz": 2, "_scaling": 3}.get(k, 0)), ("m_", 1), ("v_", 1)):
            out[prefix + k] = np.full((n_out,) + c[k].shape[1:], np.nan, np.float32)
            if WIDTH(c, k) > 0:
                table.append((c[prefix + k], out[prefix + k], WIDTH(c, k), mode))
    ptrs = lambda j: (C.c_void_p * len(table))(*[t[j].ctypes.data for t in table])
    ints = lambda j: (C.c_int32 * len(table))(*[t[j] for t in table])
    ins, outs, widths, modes = ptrs(0), ptrs(1), ints(2), ints(3)
    src, kind, binding = (np.full(n_out, -1, np.int32) for _ in range(3))
    counter = np.full(n_f, -1, np.int32)
    lib.hd_emit(n, n_f, n_out, _p(c["_xyz"]), _p(c["_scaling"]), _p(c["_rotation"]), _p(c["binding"]), _p(c["face_scaling"]), _p(c["noise"]),
                _p(keep), _p(at), len(table), C.addressof(ins), C.addressof(outs), C.addressof(widths), C.addressof(modes), _p(src), _p(kind),
                _p(binding), _p(counter))
    out.update(src=src, kind=kind, binding=binding, binding_counter=counter, counts=counts[:4].copy())
    a = [np.array(c[k]) for k in ("add_accum", "add_denom", "add_max_radii")]
    vis = (None, np.ascontiguousarray(c["radii"] > 0).view(np.uint8)) if mask else (c["radii"], None)
    lib.hd_stats_add(n, _p(c["grad"]), _p(vis[0]), _p(vis[1]), _p(a[0]), _p(a[1]), _p(a[2]))
    out.update(add_accum=a[0], add_denom=a[1], add_max_radii=a[2])
    out["reset"] = np.full(c["_opacity"].shape, np.nan, np.float32)
    lib.hd_reset_opacity(n, _p(c["_opacity"]), _p(out["reset"]))
    return out
