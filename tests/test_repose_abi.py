"""The entry points of csrc/repose.hip as return codes, without a GPU (like tests/test_track_abi.py): mpmhip_knn, mpmhip_knn_scratch,
mpmhip_shepard_weights, mpmhip_skin_to_pose and mpmhip_skin_to_tpose are declared, built and signed alike; a bad argument is
MPMHIP_ERR_INVALID whatever the device, a device that does not exist is MPMHIP_ERR_NO_DEVICE even for a request for nothing, and
nothing is written on either.  Every launching call names device -1, so nothing is launched on any machine; the pointers are addresses
of host buffers nothing reads before the return.  mpmhip_knn_scratch needs no device and is checked against the slicing rule."""
import ctypes as C
import os
import re

import pytest

from mpmavatar_amd import _lib as L
from mpmavatar_amd import build as hipbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mpmhip.h")).read()
ENTRIES = ["mpmhip_knn", "mpmhip_knn_scratch", "mpmhip_shepard_weights", "mpmhip_skin_to_pose", "mpmhip_skin_to_tpose"]


@pytest.fixture(scope="module")
def lib():
    hipbuild.build()
    return L.load()


@pytest.fixture()
def buf():
    return C.create_string_buffer(b"\x5a" * 256, 256)


def _params(name):
    return [a.strip().split()[-1].lstrip("*") for a in re.search(r"int %s\((.*?)\);" % name, HEADER, re.S).group(1).split(",")]


def _args(name, p, **ints):
    """a valid request behind (device, stream) with every pointer `p` -> (args, {argument name: position})"""
    params = _params(name)[2:]
    base = {"n": 1, "m": 4, "dim": 3, "k": 2, "slices": 0, "scratch_len": 64, "power": 2, "n_verts": 4, "n_joints": 3, "n_frames": 1,
            "n_points": 1, "verts_batched": 0, "w_batched": 0, "scale_batched": 0}
    base.update(ints)
    return [base.get(k, p) for k in params], {k: i for i, k in enumerate(params)}


def test_every_entry_point_is_declared_built_and_signed(lib):
    assert "repose.hip" in hipbuild.SOURCES and "repose_math.hpp" in hipbuild.HEADERS and "knn_device.hpp" in hipbuild.HEADERS
    for n in ENTRIES:
        declared = re.search(r"int %s\((.*?)\);" % n, HEADER, re.S).group(1).split(",")
        res, argtypes = L.SIGNATURES[n]
        assert hasattr(lib, n) and res is C.c_int and len(declared) == len(argtypes), n
        for text, ct in zip(declared, argtypes):
            if n == "mpmhip_knn_scratch" and "*" in text:
                assert ct is C.POINTER(C.c_int64)
                continue
            want = C.c_void_p if "*" in text else C.c_int64 if text.split()[-2] == "int64_t" else C.c_int32
            assert ct is want, (n, text)
    for cite in ("utils/smplx_deformer.py:164-337", ":164-185", ":187-205", ":235-241", ":290-337", ":262-286", "preprocess/helpers.py:84-94",
                 "train_material_params.py:335-349", "train_mesh_lbs_actorshq.py:495-516"):
        assert cite in HEADER, cite
    assert "MPMHIP_SKIN_MAX_JOINTS 127" in HEADER
    assert lib.mpmhip_version() == 100


def test_knn_scratch_follows_the_slicing_rule(lib):
    need = C.c_int64(-1)
    for (n, m, dim, k, slices), want in (((700, 1100, 3, 10, 0), 5 * 700 * 10), ((300, 2100, 6, 10, 0), 9 * 300 * 10), ((5, 16, 3, 16, 0), 5 * 16),
                                         ((3, 31, 3, 1, 0), 3), ((3, 31, 3, 5, 7), 7 * 3 * 5), ((3, 31, 3, 4, 100), 31 * 3 * 4),
                                         ((0, 31, 3, 4, 0), 0), ((20301, 10475, 6, 10, 0), 26 * 20301 * 10)):
        assert lib.mpmhip_knn_scratch(n, m, dim, k, slices, C.byref(need)) == L.OK and need.value == want, (n, m, dim, k, slices, need.value)
    for bad in ((-1, 4, 3, 1, 0), (1, 0, 3, 1, 0), (1, 4, 4, 1, 0), (1, 4, 3, 0, 0), (1, 4, 3, 5, 0), (1, 40, 3, 17, 0), (1, 4, 3, 1, -1)):
        assert lib.mpmhip_knn_scratch(*bad, C.byref(need)) == L.ERR_INVALID, bad
    assert lib.mpmhip_knn_scratch(1, 4, 3, 1, 0, None) == L.ERR_INVALID


def test_knn_invalid_then_no_device(lib, buf):
    p, before = C.addressof(buf), buf.raw
    f = lib.mpmhip_knn
    args, at = _args("mpmhip_knn", p)
    assert f(-1, None, *args) == L.ERR_NO_DEVICE

    def changed(**kw):
        a = list(args)
        for k, v in kw.items():
            a[at[k]] = v
        return f(-1, None, *a)

    for bad in (dict(n=-1), dict(m=0), dict(dim=4), dict(dim=2), dict(k=0), dict(k=5), dict(k=17, m=40), dict(slices=-1), dict(scratch_len=1),
                dict(queries=None), dict(targets=None), dict(scratch=None), dict(out_dists=None), dict(out_idx=None)):
        assert changed(**bad) == L.ERR_INVALID, bad
    assert changed(scratch_len=2) == L.ERR_NO_DEVICE                               # 1 slice x 1 query x 2 keys is enough
    assert changed(slices=4, scratch_len=7) == L.ERR_INVALID and changed(slices=4, scratch_len=8) == L.ERR_NO_DEVICE
    assert changed(dim=6, k=4) == L.ERR_NO_DEVICE
    assert changed(n=0, m=0) == L.ERR_INVALID                                      # an argument error wins over an empty request
    assert changed(n=0, queries=None, scratch=None, out_dists=None, out_idx=None, scratch_len=0) == L.ERR_NO_DEVICE
    assert buf.raw == before


def test_shepard_invalid_then_no_device(lib, buf):
    p, before = C.addressof(buf), buf.raw
    f = lib.mpmhip_shepard_weights
    args, at = _args("mpmhip_shepard_weights", p)
    assert f(-1, None, *args) == L.ERR_NO_DEVICE

    def changed(**kw):
        a = list(args)
        for k, v in kw.items():
            a[at[k]] = v
        return f(-1, None, *a)

    for bad in (dict(n=-1), dict(k=0), dict(k=17), dict(power=-1), dict(n_verts=0), dict(n_joints=0), dict(dists=None), dict(idx=None), dict(out_w=None)):
        assert changed(**bad) == L.ERR_INVALID, bad
    assert changed(lbs_weights=None, idx=None, n_verts=0, n_joints=0) == L.ERR_NO_DEVICE     # the weights alone
    assert changed(n=0, dists=None, idx=None, out_w=None) == L.ERR_NO_DEVICE
    assert changed(n=0, k=0) == L.ERR_INVALID
    assert buf.raw == before


@pytest.mark.parametrize("name", ["mpmhip_skin_to_pose", "mpmhip_skin_to_tpose"])
def test_skin_invalid_then_no_device(lib, buf, name):
    p, before = C.addressof(buf), buf.raw
    f = getattr(lib, name)
    args, at = _args(name, p)
    assert f(-1, None, *args) == L.ERR_NO_DEVICE

    def changed(**kw):
        a = list(args)
        for k, v in kw.items():
            a[at[k]] = v
        return f(-1, None, *a)

    for bad in (dict(n_frames=-1), dict(n_points=-1), dict(n_joints=0), dict(n_joints=128), dict(verts=None), dict(w=None), dict(A=None),
                dict(out_points=None), dict(n_frames=2 ** 20, n_points=2 ** 20)):
        assert changed(**bad) == L.ERR_INVALID, bad
    assert changed(n_joints=127) == L.ERR_NO_DEVICE
    assert changed(transl=None, scale=None, out_T=None) == L.ERR_NO_DEVICE         # the optional pointers
    for empty in (dict(n_frames=0), dict(n_points=0)):
        assert changed(verts=None, w=None, A=None, out_points=None, **empty) == L.ERR_NO_DEVICE
    assert changed(n_points=0, n_joints=0) == L.ERR_INVALID                        # an argument error wins over an empty request
    assert buf.raw == before
