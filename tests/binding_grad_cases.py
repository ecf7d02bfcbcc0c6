"""Cases, yardstick and helpers shared by tests/test_binding_grad_host.py and tests/test_gpu_binding_grad.py.  Test infrastructure only.

  case     from                                  what it holds
  main     tests/golden/binding_grad.npz         icosphere(2): 162 vertices, 320 faces (two blocks of 256), N(0, 4e-3) vertex noise, 657
                                                 Gaussians bound at random and unsorted, 300 of them on one face, the last five faces
                                                 empty; all four quaternion branches; the reference's own float64 gradients
  render   tests/golden/render_inputs.npz        the 12 x 10 sheet of the render fixture, 198 faces, 413 Gaussians; weights seeded here

The loss of a case is  sum(w_m * means3D) + sum(w_r * rotations) + sum(w_s * scales) + sum(w_o * opacities); its gradients go to
``verts``, ``_xyz``, ``_rotation``, ``_scaling``, ``_opacity`` (NAMES).  The yardstick is the float64 run of tests/binding_twin_torch.py.
"""
import ctypes as C
import os

import numpy as np
import torch

import binding_twin_torch as tw
import hostbuild

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = ("verts", "_xyz", "_rotation", "_scaling", "_opacity")
OUTS = ("means3D", "rotations", "scales", "opacities")
CASES = ("main", "render")
MIN_MARGIN = 1e-3          # the quaternion branch of every face is decided by at least this much

# Measured on the CPU (tests/test_binding_grad_host.py::test_g32_is_the_measurement asserts it): G32 = the worst, over the five tensors
# and the two cases, of max |g32 - g64| / max |g64| of the TWIN, its float32 run against its float64 run.  The code under test plays
# no part in it.  Host restatement and GPU must lie within BOUND = 10 * G32 of the float64 twin -- the factor the rasteriser's
# gradient tests use (tests/raster_grad_scenes.py): a different summation order, FMA contraction, the device's expf and division.
G32 = 3.1e-7   # measured 3.048e-7 (_opacity of `render`); the other nine figures 0.4e-7 .. 2.1e-7
BOUND = 10 * G32

_cache = {}


def case(name):
    """dict of read-only arrays: verts, faces, binding, _xyz, _rotation, _scaling, _opacity (float32 / int32) and w_<output> weights"""
    if name in _cache:
        return _cache[name]
    if name == "main":
        g = np.load(os.path.join(HERE, "golden", "binding_grad.npz"))
        c = {k: g[k] for k in g.files}
    else:
        g = np.load(os.path.join(HERE, "golden", "render_inputs.npz"))
        c = {k: g[k] for k in ("verts", "faces", "binding", "_xyz", "_rotation", "_scaling", "_opacity")}
        rng = np.random.default_rng(29)
        n = c["binding"].shape[0]
        for k, w in zip(OUTS, (3, 4, 3, 1)):
            c["w_" + k] = rng.normal(size=(n, w)).astype(np.float32)
    for v in c.values():
        v.setflags(write=False)
    _cache[name] = c
    return c


def rel_grad(g, g64):
    """max |g - g64| / max |g64| over EVERY element"""
    g, g64 = np.asarray(g, np.float64), np.asarray(g64, np.float64)
    assert g.shape == g64.shape, (g.shape, g64.shape)
    return float(np.abs(g - g64).max() / np.abs(g64).max())


def twin_grads(c, dtype=torch.float64, binding=None, weights=None):
    """the twin's gradients of the case's loss in `dtype` -> dict over NAMES (numpy), computed once per (case, dtype) by the callers"""
    t = {k: torch.tensor(np.asarray(c[k]), dtype=dtype, requires_grad=True) for k in NAMES}
    b = torch.from_numpy(np.asarray(c["binding"] if binding is None else binding).astype(np.int64))
    out = tw.render_inputs(t["verts"], torch.from_numpy(np.asarray(c["faces"]).astype(np.int64)), b, t["_xyz"], t["_rotation"],
                           t["_scaling"], t["_opacity"])
    w = weights or {k: c["w_" + k] for k in OUTS}
    loss = sum((torch.tensor(np.asarray(w[k]), dtype=dtype) * out[k]).sum() for k in OUTS if w.get(k) is not None)
    grads = torch.autograd.grad(loss, [t[k] for k in NAMES], allow_unused=True)
    return {k: (np.zeros(t[k].shape) if g is None else g.numpy()) for k, g in zip(NAMES, grads)}


_g64 = {}


def g64(name):
    """the float64 twin's gradients of a case, computed once and shared"""
    if name not in _g64:
        _g64[name] = twin_grads(case(name))
        for v in _g64[name].values():
            v.setflags(write=False)
    return _g64[name]


# ---- the two tables, with numpy's equivalents of the torch ops the package uses (stable sort, bincount, cumsum) ---------------------

def csr(keys, n_keys):
    """key -> items: (start [n_keys + 1] int32, items int32 in ascending item index within a key)"""
    keys = np.asarray(keys, np.int64).reshape(-1)
    items = np.argsort(keys, kind="stable").astype(np.int32)
    start = np.zeros(n_keys + 1, np.int32)
    start[1:] = np.cumsum(np.bincount(keys, minlength=n_keys))
    return start, items


# ---- the host build of frames_grad_math.hpp -------------------------------------------------------------------------------------

def host_lib():
    return hostbuild.host_lib("hostframes_grad")


def sanitizer_program():
    """the same file as a stand-alone program under AddressSanitizer and UBSan (run as a subprocess; nothing is loaded into Python)"""
    return hostbuild.host_program("hostframes_grad", name="hostframes_grad_asan",
                                  flags=["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                         "-DHOSTFRAMES_GRAD_MAIN"])


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, np.float32)


def host_frames_backward(verts, faces, mat, quat, g_center, g_mat, g_quat, g_fscale):
    """kernels 3 and 4 on the host -> (d_verts [n_v, 3], d_corners [n_f, 3, 3])"""
    verts, faces = _f32(verts), np.ascontiguousarray(faces, np.int32)
    n_v, n_f = verts.shape[0], faces.shape[0]
    start, corners = csr(faces, n_v)
    args = [_f32(a) for a in (mat, quat, g_center, g_mat, g_quat, g_fscale)]
    d_corners, d_verts = np.full((n_f, 3, 3), np.nan, np.float32), np.full((n_v, 3), np.nan, np.float32)
    host_lib().hf_face_frames_backward(_p(verts), _p(faces), n_f, n_v, *[_p(a) for a in args], _p(start), _p(corners), _p(d_corners),
                                       _p(d_verts))
    return d_verts, d_corners


def host_binding_backward(n_f, binding, xyz, rot, scl, opa, mat, quat, fscale, g_mean, g_opac, g_scale, g_rot, want_faces=True):
    """kernels 1 and 2 on the host -> (d_xyz, d_rot, d_scaling, d_opacity, d_center, d_mat, d_quat, d_fscale)"""
    binding = np.ascontiguousarray(binding, np.int32)
    n = binding.shape[0]
    start, items = csr(binding, n_f)
    ins = [_f32(a) for a in (xyz, rot, scl, opa, mat, quat, fscale, g_mean, g_opac, g_scale, g_rot)]
    new = lambda *s: np.full(s, np.nan, np.float32)
    outs = [new(n, 3), new(n, 4), new(n, 3), new(n, 1)]
    fouts = [new(n_f, 3), new(n_f, 3, 3), new(n_f, 4), new(n_f, 1)] if want_faces else [None] * 4
    host_lib().hf_render_inputs_backward(n, n_f, _p(binding), *[_p(a) for a in ins], *[_p(a) for a in outs], _p(start), _p(items),
                                         *[_p(a) for a in fouts])
    return outs + fouts


# ---- the host build of frames_math.hpp: the forward itself (tests/hostframes/hostframes.cpp) -------------------------------------

# the bounds tests/test_frames.py asserts for the device against tests/golden/frames.npz and oracle/face_frames.py
FRAME_TOL = {"mat": 2e-6, "scale": 1e-6, "center": 5e-7, "quat": 5e-6}


def frames_lib():
    return hostbuild.host_lib("hostframes")


def host_frames_forward(verts, faces, n_f=None):
    """k_face_frames on the host -> (face_center [n_f, 3], face_orien_mat [n_f, 3, 3], face_orien_quat [n_f, 4] WXYZ, face_scaling
    [n_f, 1]); n_f: only the first n_f faces (the outputs have that many rows)"""
    verts, faces = _f32(verts), np.ascontiguousarray(faces, np.int32)
    n_f = faces.shape[0] if n_f is None else n_f
    new = lambda *s: np.full(s, np.nan, np.float32)
    center, mat, quat, scale = new(n_f, 3), new(n_f, 3, 3), new(n_f, 4), new(n_f, 1)
    frames_lib().hfr_face_frames(_p(verts), _p(faces), n_f, _p(center), _p(mat), _p(quat), _p(scale))
    return center, mat, quat, scale


def host_quat_from_pieces(mat):
    """the matrix -> quaternion map as the backward states it (quat_branch, quat_numerators, norm4 of frames_math.hpp) on a saved
    face_orien_mat -> (branch int32 [n_f], unit quaternion WXYZ [n_f, 4])"""
    mat = _f32(mat)
    branch, quat = np.full(mat.shape[0], -1, np.int32), np.full((mat.shape[0], 4), np.nan, np.float32)
    frames_lib().hfr_quat_from_pieces(_p(mat), mat.shape[0], _p(branch), _p(quat))
    return branch, quat


def host_quat_branch(mat):
    return host_quat_from_pieces(mat)[0]


def oracle_frames(verts, faces):
    """the same four arrays as oracle/face_frames.py (pinned against the reference) states them"""
    from oracle import face_frames as ff
    o = ff.MeshFramesOracle(np.asarray(faces))
    o.set_mesh_by_verts(np.asarray(verts))
    return o.face_center, o.face_orien_mat, o.face_orien_quat.astype(np.float32), o.face_scaling


def host_grads(c, binding=None):
    """the whole backward on the host for a case's loss -> dict over NAMES"""
    b = c["binding"] if binding is None else binding
    n_f = c["faces"].shape[0]
    _, mat, quat, fscale = host_frames_forward(c["verts"], c["faces"])
    r = host_binding_backward(n_f, b, c["_xyz"], c["_rotation"], c["_scaling"], c["_opacity"], mat, quat, fscale, c["w_means3D"],
                              c["w_opacities"], c["w_scales"], c["w_rotations"])
    d_verts, _ = host_frames_backward(c["verts"], c["faces"], mat, quat, *r[4:])
    return dict(zip(NAMES, [d_verts] + r[:4]))
