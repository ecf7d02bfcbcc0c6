"""The entry points of csrc/track4d.hip as return codes, without a GPU (like tests/test_track_abi.py): every mpmhip_track4d_* function
of the header has a ctypes signature of the same length and types and is built from a source that stands after track.hip; a bad
argument is MPMHIP_ERR_INVALID whatever the device, a device that does not exist is MPMHIP_ERR_NO_DEVICE even for a request for
nothing, and nothing is written on either.  Every call names device -1, so nothing is launched on any machine; the pointers are
addresses of host buffers nothing reads before the return."""
import ctypes as C
import os
import re

import pytest

from mpmavatar_amd import _lib as L
from mpmavatar_amd import build as hipbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mpmhip.h")).read()
ENTRIES = sorted(set(re.findall(r"int (mpmhip_track4d_\w+)\(", HEADER)))
NAMES = ["mpmhip_track4d_laplacian_backward", "mpmhip_track4d_laplacian_forward", "mpmhip_track4d_scale_ratio_backward",
         "mpmhip_track4d_scale_ratio_forward"]


@pytest.fixture(scope="module")
def lib():
    hipbuild.build()
    return L.load()


@pytest.fixture()
def buf():
    return C.create_string_buffer(b"\x5a" * 256, 256)


def _args(name, p):
    """a valid request behind (device, stream): 1 face on 3 vertices, 6 adjacency entries, every pointer `p`, scratch of 4 doubles
    -> (args, {argument name: position})"""
    params = [a.strip().split()[-1].lstrip("*") for a in re.search(r"int %s\((.*?)\);" % name, HEADER, re.S).group(1).split(",")][2:]
    ints = {"n_verts": 3, "n_faces": 1, "n_nbr": 6, "n_scratch": 4}
    floats = {"th_ratio": 5.0, "th_edge": 1.0}
    return [ints.get(k, floats.get(k, p)) for k in params], {k: i for i, k in enumerate(params)}


def test_every_entry_point_is_declared_built_and_signed(lib):
    s = hipbuild.SOURCES
    assert s.index("track4d.hip") == s.index("track.hip") + 1 and "track4d_math.hpp" in hipbuild.HEADERS
    assert ENTRIES == NAMES and sorted(n for n in L.SIGNATURES if n.startswith("mpmhip_track4d_")) == ENTRIES
    for n in ENTRIES:
        declared = re.search(r"int %s\((.*?)\);" % n, HEADER, re.S).group(1).split(",")
        res, argtypes = L.SIGNATURES[n]
        assert hasattr(lib, n) and res is C.c_int and len(declared) == len(argtypes), n
        for text, ct in zip(declared, argtypes):                                  # pointer <-> c_void_p, int32_t <-> c_int32, float <-> c_float
            want = C.c_void_p if "*" in text else C.c_float if text.split()[-2] == "float" else C.c_int32
            assert ct is want, (n, text)
    for cite in ("train_mesh_lbs_4ddress.py:279-292", ":363", ":212-214", "laplacian_packed", "UNCONFIRMED against pytorch3d"):
        assert cite in HEADER, cite
    assert "MPMHIP_TRACK4D_LAPLACIAN_SCRATCH" in HEADER and "MPMHIP_TRACK4D_SCALE_RATIO_SCRATCH" in HEADER


@pytest.mark.parametrize("name", NAMES)
def test_entries_invalid_then_no_device(lib, buf, name):
    f, p = getattr(lib, name), C.addressof(buf)
    before = buf.raw
    args, at = _args(name, p)
    assert f(-1, None, *args) == L.ERR_NO_DEVICE

    def changed(**kw):
        a = list(args)
        for k, v in kw.items():
            a[at[k]] = v
        return f(-1, None, *a)

    bad = {"mpmhip_track4d_laplacian_forward": [dict(n_verts=0), dict(n_verts=-1), dict(n_nbr=-1), dict(verts=None), dict(nbr_start=None), dict(nbr=None),
                                                dict(scratch=None), dict(n_scratch=0), dict(n_verts=257, n_scratch=1)],
           "mpmhip_track4d_laplacian_backward": [dict(n_verts=0), dict(n_nbr=-1), dict(lv=None), dict(nbr_start=None), dict(nbr=None), dict(g=None)],
           "mpmhip_track4d_scale_ratio_forward": [dict(n_verts=0), dict(n_faces=0), dict(n_faces=-1), dict(n_faces=2 ** 31 // 3 + 1), dict(verts=None),
                                                  dict(faces=None), dict(scales=None), dict(scratch=None), dict(out_terms=None), dict(n_scratch=3),
                                                  dict(n_faces=257, n_scratch=4)],
           "mpmhip_track4d_scale_ratio_backward": [dict(n_verts=0), dict(n_faces=0), dict(verts=None), dict(faces=None), dict(scales=None), dict(terms=None),
                                                   dict(g_terms=None), dict(vert_start=None), dict(vert_items=None), dict(d_stencil=None)]}[name]
    for kw in bad:
        assert changed(**kw) == L.ERR_INVALID, kw
    # valid forms reach the device check
    ok = {"mpmhip_track4d_laplacian_forward": [dict(n_nbr=0, nbr=None), dict(out_value=None, scratch=None, n_scratch=0), dict(out_lv=None),
                                               dict(out_lv=None, out_value=None, scratch=None), dict(n_verts=256, n_scratch=1), dict(n_verts=257, n_scratch=2)],
          "mpmhip_track4d_laplacian_backward": [dict(n_nbr=0, nbr=None), dict(d_verts=None)],
          "mpmhip_track4d_scale_ratio_forward": [dict(n_faces=256), dict(n_faces=257, n_scratch=8)],
          "mpmhip_track4d_scale_ratio_backward": [dict(d_scales=None), dict(d_verts=None, vert_start=None, vert_items=None, d_stencil=None),
                                                  dict(d_verts=None, d_scales=None)]}[name]
    for kw in ok:
        assert changed(**kw) == L.ERR_NO_DEVICE, kw
    assert buf.raw == before                                                      # nothing was written through any pointer
