"""The entry points of csrc/track.hip as return codes, without a GPU (like tests/test_reg_abi.py): every mpmhip_track_* function of
the header has a ctypes signature of the same length; a bad argument is MPMHIP_ERR_INVALID whatever the device, a device that does
not exist is MPMHIP_ERR_NO_DEVICE even for a request for nothing, and nothing is written on either.  Every call names device -1, so
nothing is launched on any machine; the pointers are addresses of host buffers nothing reads before the return."""
import ctypes as C
import os
import re

import pytest

from mpmavatar_amd import _lib as L
from mpmavatar_amd import build as hipbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mpmhip.h")).read()
ENTRIES = sorted(set(re.findall(r"int (mpmhip_track_\w+)\(", HEADER)))


@pytest.fixture(scope="module")
def lib():
    hipbuild.build()
    return L.load()


@pytest.fixture()
def buf():
    return C.create_string_buffer(b"\x5a" * 256, 256)


def _mesh_args(name, p):
    """a valid request behind (device, stream): 1 face on 3 vertices, every pointer `p` -> (args, {argument name: position})"""
    params = [a.strip().split()[-1].lstrip("*") for a in re.search(r"int %s\((.*?)\);" % name, HEADER, re.S).group(1).split(",")][2:]
    ints = {"n_verts": 3, "n_faces": 1, "n": 1, "n_body": 1, "mode": 1}
    args = [ints.get(k, 1e-3 if k == "eps" else p) for k in params]
    return args, {k: i for i, k in enumerate(params)}


def test_every_entry_point_is_declared_built_and_signed(lib):
    assert "track.hip" in hipbuild.SOURCES and "track_math.hpp" in hipbuild.HEADERS and "nn_device.hpp" in hipbuild.HEADERS
    assert len(ENTRIES) == 8 and sorted(n for n in L.SIGNATURES if n.startswith("mpmhip_track_")) == ENTRIES
    for n in ENTRIES:
        declared = re.search(r"int %s\((.*?)\);" % n, HEADER, re.S).group(1).split(",")
        res, argtypes = L.SIGNATURES[n]
        assert hasattr(lib, n) and res is C.c_int and len(declared) == len(argtypes), n
        for text, ct in zip(declared, argtypes):                                  # pointer <-> c_void_p, int32_t <-> c_int32, float <-> c_float
            want = C.c_void_p if "*" in text else C.c_float if text.split()[-2] == "float" else C.c_int32
            assert ct is want, (n, text)
    for cite in ("train_mesh_lbs_actorshq.py:209-279", "utils/geo_utils.py:8-19", "preprocess/losses/physics.py:6-20", "UNCONFIRMED"):
        assert cite in HEADER, cite
    assert "MPMHIP_TRACK_TERMS_SCRATCH" in HEADER and "MPMHIP_TRACK_COLLISION_SCRATCH" in HEADER


@pytest.mark.parametrize("name", [n for n in ENTRIES if "collision" not in n])
def test_mesh_entries_invalid_then_no_device(lib, buf, name):
    f, p = getattr(lib, name), C.addressof(buf)
    before = buf.raw
    args, at = _mesh_args(name, p)
    assert f(-1, None, *args) == L.ERR_NO_DEVICE

    def changed(**kw):
        a = list(args)
        for k, v in kw.items():
            a[at[k]] = v
        return f(-1, None, *a)

    required = {"mpmhip_track_render_vars": ("log_scales", "logit_opacities", "out_means3D", "out_rotations", "out_scales", "out_opacities"),
                "mpmhip_track_render_vars_backward": ("log_scales", "logit_opacities", "vert_start", "vert_items", "d_stencil"),
                "mpmhip_track_face_geometry": (),
                "mpmhip_track_terms_forward": ("log_scales", "logit_opacities", "scratch", "out_terms"),
                "mpmhip_track_terms_backward": ("log_scales", "logit_opacities", "g_terms", "vert_start", "vert_items", "d_stencil"),
                "mpmhip_track_vertex_normals": ("vert_start", "vert_items", "out_normals")}[name]
    for bad in [dict(n_verts=-1), dict(n_faces=-1), dict(n_faces=2 ** 31 // 3 + 1), dict(verts=None), dict(faces=None)] + [{k: None} for k in required]:
        assert changed(**bad) == L.ERR_INVALID, bad
    assert changed(n_faces=0, n_verts=-1) == L.ERR_INVALID                        # an argument error wins over an empty request
    # valid forms reach the device check: no faces, and the optional pointers NULL
    assert changed(n_faces=0, faces=None) == L.ERR_NO_DEVICE
    optional = {"mpmhip_track_render_vars_backward": ("g_means3D", "g_rotations", "g_scales", "g_opacities", "d_log_scales", "d_logit_opacities"),
                "mpmhip_track_face_geometry": ("out_normals", "out_areas"),
                "mpmhip_track_terms_backward": ("d_log_scales", "d_logit_opacities")}.get(name, ())
    assert changed(**{k: None for k in optional}) == L.ERR_NO_DEVICE
    if name.endswith("_backward"):                                                # without d_verts neither the table nor the stencil is needed
        assert changed(d_verts=None, vert_start=None, vert_items=None, d_stencil=None) == L.ERR_NO_DEVICE
    assert buf.raw == before                                                      # nothing was written through any pointer


def test_collision_entries_invalid_then_no_device(lib, buf):
    p = C.addressof(buf)
    before = buf.raw
    for name, required, bad_ints in (("mpmhip_track_collision_forward", ("va", "vb", "best_scratch", "scratch", "out_index", "out_distance", "out_value"),
                                      [dict(n=-1), dict(n_body=0), dict(n_body=-1), dict(mode=3), dict(mode=-1)]),
                                     ("mpmhip_track_collision_backward", ("nb", "index", "distance", "g"),
                                      [dict(n=-1), dict(n_body=0), dict(mode=3)])):
        f = getattr(lib, name)
        args, at = _mesh_args(name, p)
        assert f(-1, None, *args) == L.ERR_NO_DEVICE

        def changed(**kw):
            a = list(args)
            for k, v in kw.items():
                a[at[k]] = v
            return f(-1, None, *a)

        for bad in bad_ints + [{k: None} for k in required]:
            assert changed(**bad) == L.ERR_INVALID, (name, bad)
        for mode in (0, 1, 2):
            assert changed(mode=mode) == L.ERR_NO_DEVICE
        if name.endswith("forward"):
            assert changed(nb=None, out_distance=None, scratch=None, out_value=None) == L.ERR_NO_DEVICE          # the index alone
            assert changed(mode=0, scratch=None, out_value=None) == L.ERR_NO_DEVICE                              # the distances alone
            assert changed(n=0, va=None, best_scratch=None, out_index=None, out_distance=None) == L.ERR_NO_DEVICE
        else:
            assert changed(d_va=None) == L.ERR_NO_DEVICE
            assert changed(n=0, index=None, distance=None) == L.ERR_NO_DEVICE
    assert buf.raw == before
